// What the two scoring units share: gmm.hip (dense scoring and the f32 tile walk: gmm_f32.hpp, gmm_split.hpp) and
// gmm_band.hip (lazy, windowed scoring).  The kernel parameter block, the band arithmetic of a windowed launch, the register
// reductions of the log-sum-exp, the split-operand scoring pieces (product order, block log-sum-exp, online merge,
// small-slot epilogue, staged flush), the feature split of the f16 / bf16 operand paths, and the two host helpers every
// dispatcher uses.  Everything device-side sits in an unnamed namespace, as the kernels do: each unit compiles its own copy.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "ctx.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct GmmParams {
  int dim, kpad, num_rows;  // num_rows = index of the dummy row
  const float *w; const float *gc; const int32_t *row0; const int32_t *nblk; const int32_t *slot;
  const uint4 *wb;   // bf16×3 split of the packed rows, 32-row blocks of [step][split][half][row] 16-byte units (or NULL)
  const uint4 *wh;   // f16×2 split of the column-scaled rows, same block layout with two pieces (or NULL)
  const float *gch;  // gconsts × S for the f16 kernel
  const float *fscale;   // [kpad] feature column scales S·2^-e_k for the f16 kernel
  float acc_scale_inv;   // 1 / S
  int *redo;         // [n_utt × tiles] tiles the f16 kernel declined (scaled feature outside the f16 range)
  int redo_mode;     // 0: score everything; 2: score only the tiles flagged in redo
  int *redo_count;   // number of flagged tiles (device scalar, zeroed per launch): the redo sweep returns at once when 0
  const float *feats; const int64_t *frame_off;
  const int32_t *pdf_list; const int64_t *pdf_off; const int32_t *class_counts; const int64_t *ll_off;
  unsigned long long *trace;   // debug (mfa_debug_gmm_trace): per workgroup {start, end, hw id, blocks} or NULL
  int skip_cc0;                // gmm_bf16_kernel: 1 = the single-block 32-row class was scored by gmm_split_single_kernel
  int skip_single;             // 1: the 32-row classes (0 and 1) are left to the split kernels; 2: the 16/8/4-row classes too
  const int32_t *first_frame;  // parallel to pdf_list (ascending inside each class) or NULL: see mfa_gmm_score_batch
  float *out;
  float min_log_diff;  // logf(FLT_EPSILON), computed on the host so device and oracle use the same constant
  int n_utt, tiles;    // tiles = 256-frame tiles per utterance (ceil(max_frames / 256)); items = (utterance, tile)
  int *queue;          // this launch's per-XCD item counters: [0..8), gmm_kernel also [8..16) for its second phase; zeroed per call
  const int *max_ff;   // largest first_frame of the batch (device scalar)
  // ---- lazy (windowed) scoring, mfa_gmm_score_window: one wavefront scores the 64 frames [b_t_begin + 64 r, +64) of one
  // utterance for the pdfs inside the band the decoder published for this window
  int b_mode;                  // 1: band mode
  int b_t_begin, b_sub;        // window start; 64-frame sub-tiles per window
  const int32_t *b_band;       // [n_utt][2] {min longest-path depth of a live token, max BFS depth reachable in the window}
  const int32_t *b_utt_list; const int32_t *b_n_list;
  const int32_t *b_done; int b_done_stride, b_done_word;
  // utterances one window behind the launch (their speculative window failed and is scored again, with the proven band, by the
  // next launch): lag word of the decoder's per-utterance state, frames per window
  const int32_t *b_lag; int b_lag_stride, b_lag_word, b_lag_frames;
  const int32_t *last_depth;   // parallel to pdf_list: running max (inside a class) of the longest-path depth of the pdf's sources
  int b_skip0;                 // f32 band kernel: classes 0..4 were scored by gmm_band_kernel (it keeps 5: single Gaussians, f32-exact)
  int b_chunk, b_nchunk;       // gmm_band_kernel: columns per wavefront (0 = the whole band) and chunks per sub-tile
  const uint4 *xsplit;         // band kernel: pre-split f16 operands [tile][2][kSteps][2][64 lanes] (gmm_presplit_kernel) or NULL
  const int *xsplit_bad;       // [tile]: 1 = a scaled feature of the tile left the f16 range (the bf16×3 pass takes it)
  const int32_t *col_row0;     // band kernel: row0[pdf_list[j]] of every column of the batch (gmm_col_rows_kernel)
  const int32_t *col_own_last; // band kernel: deepest source state (BFS depth) of every column's own arcs (gmm_col_own_last_kernel);
                               //   last_depth above is its running maximum along the run
  int32_t *ranges;             // [n_utt][kRangeSlots][2] band index ranges of the window (gmm_band_ranges_kernel)
  // Grouped plans (mfa_build_score_plan_grouped): class 0 of every utterance is laid out in `groups` runs (pdf id mod groups),
  // each ordered by first depth.  gmm_band_kernel then runs `groups` wavefronts per sub-tile, wavefront x — in a workgroup
  // with blockIdx % groups == x, i.e. (groups = 8) always on the same XCD — scoring run x: that XCD's L2 only ever sees
  // an eighth of the model.
  int groups;                  // 0/1: ungrouped
  const int32_t *group_counts; // [n_utt][groups]
  int b_split;                 // 1: this launch's grid holds `groups` workgroups per four sub-tiles (gmm_band_kernel)
  int b_hi_slack;              // band mode: arcs taken off the band's upper depth bound (speculative look-ahead), 0 = none
  int col_nb_packed;           // 1: col_row0 of a pdf of several blocks carries (blocks − 1) in its five low bits (rows of
                               //    the 32-row classes are multiples of 32; models whose largest pdf has ≤ 1 024 Gaussians)
};

// Band of one (utterance, window): pdf j of a class is needed iff first_frame[j] <= hi and last_depth[j] >= lo; both keys
// are non-decreasing along a class, so the needed pdfs are the index range [count(last_depth < lo), count(first_frame <= hi)).
struct Band { int lo, hi; };
__device__ __forceinline__ int band_lag(const GmmParams &p, int utt) {
  return (p.b_lag && p.b_t_begin > 0) ? (p.b_lag[(size_t)utt * p.b_lag_stride + p.b_lag_word] != 0 ? 1 : 0) : 0;
}
// first frame of the utterance's window in this launch
__device__ __forceinline__ int band_t_begin(const GmmParams &p, int utt) { return p.b_t_begin - band_lag(p, utt) * p.b_lag_frames; }
__device__ __forceinline__ Band band_of(const GmmParams &p, int utt) {
  Band b;
  const int lag = band_lag(p, utt);
  if (p.b_t_begin - lag * p.b_lag_frames <= 0) { b.lo = 0; b.hi = 64 * p.b_sub - 1; }   // only the start state is live: BFS depth 0
  else { b.lo = p.b_band[2 * utt]; b.hi = p.b_band[2 * utt + 1]; }
  // speculative look-ahead (the decoder checks what it reads) — not for a window that is being redone: the proven band
  if (p.b_hi_slack > 0 && !lag && b.hi != INT32_MAX) b.hi -= p.b_hi_slack;
  return b;
}
// gmm_band_kernel launches over a grouped plan: workgroup → (index of its four sub-tiles, run of class 0).  Consecutive
// workgroups go to consecutive XCDs, so the run's XCD is blockIdx % 8.  With 16 runs an XCD serves two of them — x and
// x + 8 — one after the other: the first half of the grid is runs 0..7, the second half runs 8..15, so that at any time an
// XCD's L2 is asked for one sixteenth of the model.  (Measured on the 51 MB model of BASELINE configs[2]: 12.8 ms per step
// against 11.2 with eight runs — sixteen wavefronts per sub-tile pay sixteen start-up chains; eight is the default.)
__device__ __forceinline__ int2 band_split_block(const GmmParams &p) {
  if (p.groups <= 8) return make_int2((int)(blockIdx.x / (unsigned)p.groups), (int)(blockIdx.x % (unsigned)p.groups));
  const unsigned half = gridDim.x >> 1, phase = blockIdx.x >= half ? 1u : 0u, rem = blockIdx.x - phase * half;
  return make_int2((int)(rem >> 3), (int)(phase * 8u + (rem & 7u)));
}
// wavefront item → (utterance, 64-frame sub-tile[, chunk]) of a band-mode launch; false: nothing to do
__device__ __forceinline__ bool band_witem(const GmmParams &p, int witem, int &utt, int &r, int *chunk = nullptr) {
  if (chunk) { const int q = witem / p.b_nchunk; *chunk = witem - q * p.b_nchunk; witem = q; }
  const int item = witem / p.b_sub;
  r = witem - item * p.b_sub;
  const int n_items = p.b_n_list ? *p.b_n_list : p.n_utt;
  if (item >= n_items) return false;
  utt = p.b_utt_list ? p.b_utt_list[item] : item;
  if (p.b_t_begin > 0 && p.b_done && p.b_done[(size_t)utt * p.b_done_stride + p.b_done_word] != 0) return false;
  return true;
}
// full grids (one wavefront per item): the item follows from the workgroup
__device__ __forceinline__ bool band_item(const GmmParams &p, int wave, int &utt, int &r, int *chunk = nullptr) {
  return band_witem(p, (p.b_split ? band_split_block(p).x : (int)blockIdx.x) * 4 + wave, utt, r, chunk);
}
// Strided grids (list passes, redo sweeps: launches that find work for a handful of wavefronts, or none): a small fixed
// grid whose wavefronts walk the items first, first + stride, … < n_witems — the items of a full grid, counted on the
// device.  Grouped plans keep their rule: workgroup b scores run b % groups (the grid is a multiple of `groups`), so run
// x still meets XCD x only.  (With 16 runs an XCD serves x and x + 8 at the same time here; the full grid runs them one
// after the other, band_split_block, so that its L2 sees a sixteenth of the model at a time.  Eight runs is the default.)
struct BandWalk { int first, stride, n_witems, grp; };
__device__ __forceinline__ BandWalk band_walk(const GmmParams &p, int wave, bool chunks) {
  BandWalk w;
  const unsigned runs = p.b_split ? (unsigned)p.groups : 1u;
  w.grp = (int)(blockIdx.x % runs);
  w.first = (int)(blockIdx.x / runs) * 4 + wave;
  w.stride = (int)(gridDim.x / runs) * 4;
  const int n_items = p.b_n_list ? *p.b_n_list : p.n_utt;
  w.n_witems = n_items * p.b_sub * (chunks ? p.b_nchunk : 1);
  return w;
}

// one past the last index (i0 + lane) whose bit is set in a 64-lane ballot, 0 if none
__device__ __forceinline__ int prefix_end(unsigned long long mask, int i0) { return mask ? i0 + 64 - __clzll((long long)mask) : 0; }

// row index (within a 32-row MFMA block) held by accumulator register r of a lane in half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// partner lane's value across the two 32-lane halves: one v_permlane32_swap instead of a round trip through the LDS
// crossbar (ds_bpermute)
__device__ __forceinline__ float swap32(float v, int h) {
#if __has_builtin(__builtin_amdgcn_permlane32_swap)
  unsigned u = __float_as_uint(v);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(h ? r[0] : r[1]);
#else
  return __shfl_xor(v, 32);
#endif
}

// log-sum-exp pieces (Kaldi LogSumExp semantics)
template <int R0, int R1>
__device__ __forceinline__ float reg_max(const f32x16 &v) {
  float m = v[R0];
#pragma unroll
  for (int r = R0 + 1; r < R1; r++) m = fmaxf(m, v[r]);
  return m;
}
// split-operand paths: Σ_r exp(v[r] − mx) without Kaldi's cutoff (terms below max + ln ε add < 4e-6 to the sum in total —
// inside those paths' tolerance, and mathematically the exact log-sum-exp), two terms per packed instruction: 16 exp2,
// 8 v_pk_add_f32, 8 v_pk_mul_f32, 8 packed adds per tile instead of ≈110 instructions.  The difference is formed BEFORE the
// multiplication by log2 e: fma(v, log2e, −mx·log2e) would carry the rounding of mx·log2e (2^-24·|mx|) into every term —
// 5e-6 on the result at |mx| = 100 and an overflow to inf for an outlier frame with |mx| ≳ 1e9.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float reg_expsum_fast(const f32x16 &v, float mx, float l2e = 1.44269504088896341f) {
  const f32x2 lv = {l2e, l2e};
  const f32x2 mv = {mx, mx};
  f32x2 e[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const f32x2 x = {v[2 * r], v[2 * r + 1]};
    const f32x2 arg = (x - mv) * lv;
    e[r].x = __builtin_amdgcn_exp2f(arg.x);
    e[r].y = __builtin_amdgcn_exp2f(arg.y);
  }
#pragma unroll
  for (int w = 1; w < 8; w <<= 1)
#pragma unroll
    for (int r = 0; r + w < 8; r += 2 * w) e[r] += e[r + w];
  return e[0].x + e[0].y;
}

// LL = max + ln(sum) with the hardware log2 (1 ulp on a value ≤ 7, i.e. ≲4e-7 absolute).
__device__ __forceinline__ float finish(float mx, float sum) {
  return fmaf(__builtin_amdgcn_logf(sum), 0.693147180559945309f, mx);
}

// ---- the split-operand scoring pieces: ONE definition of the arithmetic the dense kernels (gmm_split.hpp) and the band
// kernel (gmm_band.hip) promise to agree on to the bit — product order, block log-sum-exp, online merge, small-slot
// epilogue — and of the staged-column flush.  A kernel that keeps a copy of its own says so at the copy.
template <int kPieces>   // 3: bf16 triples; 2: column-scaled f16 pairs
struct SplitOps {
  static constexpr bool kHalf = kPieces == 2;
  using op8 = std::conditional_t<kHalf, f16x8, bf16x8>;
  // six (three) products per 16 k-values, smallest terms first: product t multiplies A piece pa(t) by B piece pb(t)
  static constexpr int kProd = kHalf ? 3 : 6;
  static constexpr int pa(int t) { constexpr int v[6] = {kHalf ? 1 : 2, kHalf ? 0 : 1, 0, 1, 0, 0}; return v[t]; }
  static constexpr int pb(int t) { constexpr int v[6] = {0, 1, kHalf ? 0 : 2, 0, 1, 0}; return v[t]; }
  // The products of 16-k step s for both frame tiles: a = the block's pieces of that step, b = the wavefront's x̃ operands.
  // The two tiles alternate so that consecutive MFMAs never wait on each other's accumulator; the first product of step 0
  // takes `init` (the gconsts) as its addend.  after(t, n) runs behind each MFMA (gmm_split_single_kernel's epilogue chunks).
  // gmm_band_kernel spells this loop out itself (see the note there): the table above is what the two must share.
  template <int kSteps, typename After>
  __device__ __forceinline__ static void mfma_step(const op8 (&a)[kPieces], const op8 (&b)[2][kSteps][kPieces], f32x16 (&acc)[2],
                                                   const f32x16 &init, int s, After &&after) {
#pragma unroll
    for (int t6 = 0; t6 < kProd; t6++)
#pragma unroll
      for (int n = 0; n < 2; n++) {
        const f32x16 &cin = (s == 0 && t6 == 0) ? init : acc[n];
        if constexpr (kHalf) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[pa(t6)], b[n][s][pb(t6)], cin, 0, 0, 0);
        else acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa(t6)], b[n][s][pb(t6)], cin, 0, 0, 0);
        after(t6, n);
      }
  }
  template <int kSteps>
  __device__ __forceinline__ static void mfma_step(const op8 (&a)[kPieces], const op8 (&b)[2][kSteps][kPieces], f32x16 (&acc)[2],
                                                   const f32x16 &init, int s) {
    mfma_step(a, b, acc, init, s, [](int, int) {});
  }
};

// The accumulator seed of a 32-row block, gconst of row acc_row(r, h) in register r, from the block's 32 gconsts in LDS
// (four aligned 16-byte loads per lane).  gmm_band_kernel seeds from registers it loaded a block earlier, in its own words.
__device__ __forceinline__ f32x16 init_from_gconst(const float *gc_blk, int h) {
  f32x16 init;
#pragma unroll
  for (int qq = 0; qq < 4; qq++) {
    const float4 gq = *reinterpret_cast<const float4 *>(&gc_blk[8 * qq + 4 * h]);
    init[4 * qq] = gq.x; init[4 * qq + 1] = gq.y; init[4 * qq + 2] = gq.z; init[4 * qq + 3] = gq.w;
  }
  return init;
}

// (max, Σ exp(x − max)) over the 32 rows of a block for this lane's frame, in accumulator units (× S: l2e_s = log2 e / S)
struct Lse { float m, s; };
__device__ __forceinline__ Lse block_lse(const f32x16 &acc, int h, float l2e_s) {
  float m = reg_max<0, 16>(acc);
  m = fmaxf(m, swap32(m, h));
  float sv = reg_expsum_fast(acc, m, l2e_s);
  sv += swap32(sv, h);
  return {m, sv};
}
// online log-sum-exp of a pdf of several blocks: folds a block's (m, s) into the running pair (M, S)
__device__ __forceinline__ void lse_merge(float &M, float &S, float m, float s, float l2e_s) {
  const float mn = fmaxf(M, m);
  S = S * __builtin_amdgcn_exp2f((M - mn) * l2e_s) + s * __builtin_amdgcn_exp2f((m - mn) * l2e_s);
  M = mn;
}

// The small-slot classes: 32 / kSlot pdfs share a (gathered) 32-row block, the log-sum-exp runs over the kSlot rows of each
// pdf and the block yields 32 / kSlot score columns, staged from column colbase on in the rows of this lane's two frames.
// Accumulator register r of half-wave h is row (r & 3) + 8 (r >> 2) + 4 h of the block.
template <int kSlot>
__device__ __forceinline__ void small_slot_scores(const f32x16 (&acc)[2], float *stage, int col, int colbase, int h, float inv_s,
                                                  float l2e_s) {
  auto group_max = [&](const f32x16 &v, int r0, int cnt) {
    float m = v[r0];
#pragma unroll
    for (int rr = 1; rr < cnt; rr++) m = fmaxf(m, v[r0 + rr]);
    return m;
  };
  // Σ exp(x − m) over `cnt` registers from r0, pairwise; m: their maximum
  auto group_expsum = [&](const f32x16 &v, int r0, int cnt, float m) {
    float e[8];
#pragma unroll
    for (int rr = 0; rr < cnt; rr++) e[rr] = __builtin_amdgcn_exp2f((v[r0 + rr] - m) * l2e_s);
#pragma unroll
    for (int w = 1; w < cnt; w <<= 1)
#pragma unroll
      for (int rr = 0; rr + w < cnt; rr += 2 * w) e[rr] += e[rr + w];
    return e[0];
  };
#pragma unroll
  for (int n = 0; n < 2; n++) {
    float *srow = stage + (32 * n + col) * 33 + colbase;
    if constexpr (kSlot == 16) {                   // pdf k: rows 16k..16k+15 = registers [8k, 8k+8) of both halves
      float ll[2];
#pragma unroll
      for (int k2 = 0; k2 < 2; k2++) {
        float m = group_max(acc[n], 8 * k2, 8);
        m = fmaxf(m, swap32(m, h));
        float sv = group_expsum(acc[n], 8 * k2, 8, m);
        sv += swap32(sv, h);
        ll[k2] = finish(m * inv_s, sv);
      }
      srow[h] = h ? ll[1] : ll[0];                 // each half-wave stores one of the two columns
    } else if constexpr (kSlot == 8) {             // pdf k: rows 8k..8k+7 = registers [4k, 4k+4) of both halves
      float ll[4];
#pragma unroll
      for (int k2 = 0; k2 < 4; k2++) {
        float m = group_max(acc[n], 4 * k2, 4);
        m = fmaxf(m, swap32(m, h));
        float sv = group_expsum(acc[n], 4 * k2, 4, m);
        sv += swap32(sv, h);
        ll[k2] = finish(m * inv_s, sv);
      }
      srow[h] = h ? ll[1] : ll[0];
      srow[2 + h] = h ? ll[3] : ll[2];
    } else {                                       // kSlot 4: pdf 2i + h: rows 8i + 4h .. +3 = registers [4i, 4i+4)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float m = group_max(acc[n], 4 * i, 4);
        const float sv = group_expsum(acc[n], 4 * i, 4, m);
        srow[2 * i + h] = finish(m * inv_s, sv);
      }
    }
  }
}

// `count` staged columns of a wavefront's [64 frames][33] staging tile, the first of them score column first_col of the
// utterance's [T][P] matrix → HBM as 128-byte row segments (a lane-per-frame store would touch 64 lines per instruction).
// Streaming stores: the scores are written once and read once by the decoder; keeping them out of the Infinity Cache
// leaves room for the model rows.  Wavefront-scope fences on both sides: the stage is the wavefront's own.
// (gmm_band_kernel's flush_cols is a copy of this body: see the note there.)
__device__ __forceinline__ void flush_staged(const float *stage, float *out, int P, int t_base, int T, int first_col, int count,
                                             int col, int h) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
  for (int i = 0; i < 32; i++) {
    const int r = h + 2 * i, t = t_base + r;
    if (col < count && t < T) __builtin_nontemporal_store(stage[r * 33 + col], &out[(size_t)t * P + first_col + col]);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// x̃ = [x, x²] of a wavefront's two 32-frame tiles (frames t_base + 32 n + col, clamped into the utterance), split into
// the MFMA's B operands: b[tile][step][piece], lane = (frame col, k-half h).  kPieces = 3: bf16 triples (v = v1 + v2 + v3,
// round to nearest even each).  kPieces = 2: f16 pairs of the column-scaled value; returns true when a scaled value
// leaves the f16 range (or is NaN) — the caller then hands the whole tile to the bf16×3 pass.
template <int kSteps, int kPieces, typename Op8>
__device__ __forceinline__ bool split_features(const GmmParams &p, int64_t f0, int T, int t_base, int col, int h,
                                               Op8 (&b)[2][kSteps][kPieces]) {
  bool bad = false;
#pragma unroll
  for (int n = 0; n < 2; n++) {
    int t = t_base + 32 * n + col;
    t = t < T ? t : T - 1;
    t = t < 0 ? 0 : t;
    const float *x = p.feats + (f0 + t) * p.dim;
    const bool vec8 = (p.dim & 7) == 0;   // every group of 8 operand columns then lies wholly in x, in x² or in the padding
#pragma unroll
    for (int s = 0; s < kSteps; s++) {
      float xv8[8], fs8[8];
      {
        const int k0 = 16 * s + 8 * h;
        if (vec8) {   // two 16-byte loads per group instead of eight 4-byte ones (same values)
          const int i0 = k0 < p.dim ? k0 : (k0 < 2 * p.dim ? k0 - p.dim : 0);
          const float4 lo4 = *reinterpret_cast<const float4 *>(x + i0), hi4 = *reinterpret_cast<const float4 *>(x + i0 + 4);
          xv8[0] = lo4.x; xv8[1] = lo4.y; xv8[2] = lo4.z; xv8[3] = lo4.w; xv8[4] = hi4.x; xv8[5] = hi4.y; xv8[6] = hi4.z; xv8[7] = hi4.w;
          if constexpr (kPieces == 2) {
            const float4 f0_ = *reinterpret_cast<const float4 *>(p.fscale + k0), f1_ = *reinterpret_cast<const float4 *>(p.fscale + k0 + 4);
            fs8[0] = f0_.x; fs8[1] = f0_.y; fs8[2] = f0_.z; fs8[3] = f0_.w; fs8[4] = f1_.x; fs8[5] = f1_.y; fs8[6] = f1_.z; fs8[7] = f1_.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const int k = k0 + e;
            xv8[e] = x[k < p.dim ? k : (k < 2 * p.dim ? k - p.dim : 0)];
            if constexpr (kPieces == 2) fs8[e] = p.fscale[k];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int k = 16 * s + 8 * h + e;
        const float xv = xv8[e];
        const float v = k < p.dim ? xv : (k < 2 * p.dim ? xv * xv : 0.0f);
        if constexpr (kPieces == 2) {
          const float sv = v * fs8[e];
          bad |= !(fabsf(sv) <= 65000.0f);
          const _Float16 v1 = (_Float16)sv;
          b[n][s][0][e] = v1; b[n][s][1][e] = (_Float16)(sv - (float)v1);
        } else {
          const __bf16 v1 = (__bf16)v;
          const float r1 = v - (float)v1;
          const __bf16 v2 = (__bf16)r1;
          const float r2 = r1 - (float)v2;
          b[n][s][0][e] = v1; b[n][s][1][e] = v2; b[n][s][2][e] = (__bf16)r2;
        }
      }
    }
  }
  return bad;
}

}  // namespace

// ---- host side
// Which split-operand passes a launch may use.  MFA_GMM_BF16=0 keeps every class on the exact-f32 kernels, MFA_GMM_F16=0
// skips the f16×2 pass (bf16×3 scores everything).  Read at every call: tests and the benchmark flip them inside one process.
struct GmmSplitPasses { bool bf16, f16; };
inline GmmSplitPasses gmm_split_passes(const mfa_ctx *c) {
  auto off = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
  const bool bf16 = !off("MFA_GMM_BF16") && c->d_wb;
  return {bf16, bf16 && !off("MFA_GMM_F16") && c->d_wh};
}
// The MFMA kernels are instantiated for packed rows of 80 or 96 floats: five or six 16-k steps (kernels <5, …> / <6, …>;
// the f32 kernels count 8-k groups, <10> / <12>).  f receives the step count as a std::integral_constant.
template <typename F>
inline void gmm_with_steps(int kpad, F &&f) {
  if (kpad == 80) f(std::integral_constant<int, 5>{});
  else f(std::integral_constant<int, 6>{});
}

// Band-mode launch of the f32 tile walk (gmm_band_f32_kernel, gmm_f32.hpp in gmm.hip's unit) for mfa_gmm_score_window (gmm_band.hip).  `params`
// points to the launch's GmmParams: the type lives in each unit's unnamed namespace (the kernels' symbol names carry it),
// so a function that crosses units cannot name it.  `strided`: `grid` is a small fixed grid whose wavefronts walk the items.
void mfa_gmm_launch_band_f32(mfa_ctx *c, const void *params, dim3 grid, bool strided);
