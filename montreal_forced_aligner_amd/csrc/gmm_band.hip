// Lazy (windowed) scoring of the diagonal-GMM acoustic model: the path every alignment runs on.  Kernels in this file:
//   gmm_band_kernel         the band's pdfs of 2..32·n Gaussians (slot classes 0..4) on v_mfma_f32_32x32x16_{f16,bf16}: an
//                           f16×2 pass, then a bf16×3 pass over the sub-tiles the first one declined;
//   gmm_presplit_kernel     once per batch: the f16 operand pieces of every 64-frame tile, in the band kernel's register layout;
//   gmm_col_rows_kernel     once per batch: the first packed model row of every score column;
//   gmm_col_own_last_kernel once per batch: every score column's own last depth (class 0 skips columns below the band with it);
//   gmm_band_ranges_kernel  once per window: the band's index range in every class (and run of class 0) of every utterance.
// Single-Gaussian pdfs (and everything under MFA_GMM_BF16=0) go to gmm_band_f32_kernel, the exact-f32 tile walk, which lives
// next to its score_tile in gmm.hip's unit (gmm_f32.hpp) and is reached through mfa_gmm_launch_band_f32.  mfa_gmm_score_window (end of file)
// decides the launches; mfa_gmm_presplit prepares a batch.  Shared pieces: gmm_common.hpp.
//
// Kaldi evaluates its decodable lazily: a score exists only if a live token's arc asked for it.  The dense kernels (gmm.hip)
// score every pdf of the utterance's graph for every frame from the pdf's first reachable frame on — measured, ≈9× more
// cells than the decoder reads.  Here the decoder runs in windows of K frames and publishes, at each window end, the band
// of graph depths its live tokens can reach within K arcs; gmm_band_kernel scores, for the window's frames, only the pdfs
// whose arcs leave states inside that band.
//
// With so few frames per (utterance, pdf) there is nothing to share a model block across: one wavefront owns one
// (utterance, 64-frame sub-tile), keeps its x̃ operands in registers (as the dense kernels do) and streams the band's model
// blocks straight from L2 / Infinity Cache into its A registers — 10 coalesced 1 KiB loads per 32-row block, each operand
// register re-loaded for the next block as soon as the MFMAs that read it have been issued.  Per block: 30 (60) MFMAs,
// the log-sum-exp, one staged score column.  Arithmetic per cell is that of gmm_split_single_kernel exactly (same operand
// split, same product order, same epilogue expressions — gmm_common.hpp's, bar the copies this kernel names in its body):
// a cell scored here is bit-identical to the dense kernel's.
// Bound: the 10 KiB (15 KiB) of operands per block and 64 frames — fabric bandwidth, not the matrix pipe.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "gmm_common.hpp"

namespace {

// Lazy scoring, once per batch: the first packed model row of every score column (saves the pdf id → row lookup, one
// dependent load per model block and in every wavefront's start-up chain).
__global__ void gmm_col_rows_kernel(GmmParams p, int32_t *out) {
  const int utt = blockIdx.x;
  const int64_t l0 = p.pdf_off[utt], l1 = p.pdf_off[utt + 1];
  for (int64_t j = l0 + threadIdx.x; j < l1; j += blockDim.x) {
    const int pdf = p.pdf_list[j];
    int r = p.row0[pdf];
    if (p.col_nb_packed) { const int nb = p.nblk[pdf]; if (nb > 1) r |= nb - 1; }
    out[j] = r;
  }
}

// Lazy scoring, once per batch: every score column's OWN last depth — the largest BFS depth of a state one of the column's arcs
// leaves.  The plan's last_depth is the running maximum of this along a run (which makes the band an index range); the band
// kernel tests the column's own value inside that range and skips what no token can ask for.  One workgroup per utterance;
// epsilon input arcs (the tail of a state's arcs when the batch has d_state_nemit) emit no column.
__global__ void gmm_col_own_last_kernel(mfa_graph_batch g, const int32_t *state_depth, const int64_t *pdf_off, int32_t *out) {
  const int utt = blockIdx.x;
  const int64_t l0 = pdf_off[utt];
  const int P = (int)(pdf_off[utt + 1] - l0);
  for (int j = threadIdx.x; j < P; j += blockDim.x) out[l0 + j] = 0;
  __syncthreads();
  const int64_t so = g.d_state_off[utt], ab = g.d_arc_base[utt];
  const int S = (int)(g.d_state_off[utt + 1] - so);
  const int32_t *arc_off = g.d_arc_off + so + utt;
  const int32_t *nemit = g.d_state_nemit ? g.d_state_nemit + so : nullptr;
  for (int s_ = threadIdx.x; s_ < S; s_ += blockDim.x) {
    const int d = state_depth[2 * (so + s_)];
    const int a0 = arc_off[s_], a1 = nemit ? a0 + nemit[s_] : arc_off[s_ + 1];
    for (int a = a0; a < a1; a++) {
      const int c = g.d_arc_col[ab + a];
      if ((unsigned)c < (unsigned)P) atomicMax(&out[l0 + c], d);
    }
  }
}

// Lazy scoring, once per window: the band's index range [lo, hi) in every run of class 0 (slots 0..groups-1; one run when the
// plan is not grouped), in classes 2, 3, 4 and in class 1 (the slots after the runs'), relative to the class's first column — what every scoring
// wavefront of the sub-tile would otherwise search for itself (two dependent memory trips each).  One wavefront per utterance.
constexpr int kRunSlots = kMfaRunSlots;   // slots 0..kRunSlots-1: runs of class 0; then classes 2, 3, 4; then class 1; then class 5
constexpr int kRangeSlots = kMfaRangeSlots;
__global__ __launch_bounds__(256) void gmm_band_ranges_kernel(GmmParams p) {
  const int lane = threadIdx.x & 63;
  const int utt = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (utt >= p.n_utt) return;
  if (p.b_t_begin > 0 && p.b_done && p.b_done[(size_t)utt * p.b_done_stride + p.b_done_word] != 0) return;
  const int64_t l0 = p.pdf_off[utt];
  const int32_t *cc6 = p.class_counts + (size_t)utt * 6;
  const Band bd = band_of(p, utt);
  const int runs = p.groups > 1 ? p.groups : 1;
  int32_t *out = p.ranges + (size_t)utt * kRangeSlots * 2;
  int off = 0;
  for (int slot = 0; slot < kRangeSlots; slot++) {
    int cnt = 0, base = 0;     // the run searched, its first column relative to the class, the class's first column in `off`
    if (slot < kRunSlots) {
      if (slot >= runs) continue;
      if (p.groups > 1) { const int32_t *gc = p.group_counts + (size_t)utt * p.groups; for (int g = 0; g < slot; g++) base += gc[g]; cnt = gc[slot]; }
      else cnt = cc6[0];
      off = 0;
    } else if (slot == kRunSlots + 3) {
      off = cc6[0];
      cnt = cc6[1];
    } else if (slot == kRunSlots + 4) {
      off = cc6[0] + cc6[1] + cc6[2] + cc6[3] + cc6[4];
      cnt = cc6[5];
    } else {
      const int cls = slot - kRunSlots + 2;
      off = cc6[0] + cc6[1];
      for (int k = 2; k < cls; k++) off += cc6[k];
      cnt = cc6[cls];
    }
    int nh = 0, nl = 0;
    for (int i0 = 0; i0 < cnt; i0 += 256) {
      int ff[4], ld[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = min(i0 + 64 * u + lane, cnt - 1);
        ff[u] = p.first_frame[l0 + off + base + i]; ld[u] = p.last_depth[l0 + off + base + i];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool in = i0 + 64 * u + lane < cnt;
        nh += __popcll(__ballot(in && ff[u] <= bd.hi));
        nl += __popcll(__ballot(in && ld[u] < bd.lo));
      }
    }
    if (lane == 0) { out[2 * slot] = base + min(nl, nh); out[2 * slot + 1] = base + nh; }
  }
}

// Index of the 64-frame tile `tile` of utterance `utt` in the pre-split operand buffer: ⌊frame_off/64⌋ + utt + tile is
// monotone and leaves every utterance room for ⌈T/64⌉ tiles without a separate offset table.
__device__ __forceinline__ int64_t xsplit_tile_index(int64_t frame_off_u, int utt, int tile) { return (frame_off_u >> 6) + utt + tile; }

// Lazy scoring pre-pass: the f16 hi/lo operands [x, x²]·scale of every 64-frame tile, in the register layout the band
// kernel's MFMAs read (b[n][step][piece] of lane l at ((n·kSteps + step)·2 + piece)·64 + l), so that a wavefront starts
// a window with twenty coalesced 1 KiB loads instead of 160 strided 4-byte loads and the split arithmetic — the values are
// those of split_features bit for bit.  One wavefront per tile; tiles_per_utt is a multiple of four, so a workgroup's four
// wavefronts hold the sub-tiles of one 256-frame tile of one utterance, and the range flag is that tile's: a scaled feature
// out of the f16 range hands all four sub-tiles to the bf16×3 pass, as the dense kernels' 256-frame items do — a cell
// then carries the same bits whichever path scored it.
template <int kSteps>
__global__ __launch_bounds__(256) void gmm_presplit_kernel(GmmParams p, uint4 *out, int *bad_out, int tiles_per_utt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t item = (int64_t)blockIdx.x * 4 + wave;
  const int utt = (int)(item / tiles_per_utt), tile = (int)(item - (int64_t)utt * tiles_per_utt);
  const int64_t f0 = utt < p.n_utt ? p.frame_off[utt] : 0;
  const int T = utt < p.n_utt ? (int)(p.frame_off[utt + 1] - f0) : 0;
  const bool live = tile * 64 < T;
  const int64_t ti = xsplit_tile_index(f0, utt, tile);
  bool bad = false;
  if (live) {
    f16x8 b[2][kSteps][2];
    bad = split_features<kSteps, 2>(p, f0, T, tile * 64, lane & 31, lane >> 5, b);
    uint4 *dst = out + ti * (2 * kSteps * 2 * 64) + lane;
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int s_ = 0; s_ < kSteps; s_++)
#pragma unroll
        for (int q = 0; q < 2; q++) dst[((n * kSteps + s_) * 2 + q) * 64] = __builtin_bit_cast(uint4, b[n][s_][q]);
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (live && lane == 0) bad_out[ti] = any_bad ? 1 : 0;
}

// Phase accounting of gmm_band_kernel for -DGMM_BAND_STAMPS builds (buffer from mfa_debug_gmm_trace, summed over the f16
// pass's wavefronts with work).  trace[0..2]: 100 MHz ticks of {item + band search, feature split, block loops}, [3]:
// wavefronts, [4]: class-0 blocks; trace[8..11]: shader-clock cycles of the class-0 block loop's {MFMA phase (issue + operand
// waits), lookup wait, log-sum-exp + stage, flush}.  The default build compiles every call to nothing.
#ifdef GMM_BAND_STAMPS
struct BandStamps {
  unsigned long long wall[4], cyc[5], ph[4] = {0, 0, 0, 0};
  __device__ __forceinline__ void mark(int k) { wall[k] = wall_clock64(); }
  __device__ __forceinline__ void mark_loads_landed(int k) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); mark(k); }
  __device__ __forceinline__ void cycle(int k) { cyc[k] = clock64(); }
  __device__ __forceinline__ void cycle_lds_landed(int k) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); cycle(k); }
  __device__ __forceinline__ void block_done() {
#pragma unroll
    for (int k = 0; k < 4; k++) ph[k] += cyc[k + 1] - cyc[k];
  }
  __device__ __forceinline__ void add_block_phases(const GmmParams &p, bool on) {
    if (!p.trace || !on) return;
#pragma unroll
    for (int k = 0; k < 4; k++) atomicAdd(&p.trace[8 + k], ph[k]);
  }
  __device__ __forceinline__ void add_kernel_phases(const GmmParams &p, bool on, int blocks) {
    if (!p.trace || !on) return;
    mark(3);
#pragma unroll
    for (int k = 0; k < 3; k++) atomicAdd(&p.trace[k], wall[k + 1] - wall[k]);
    atomicAdd(&p.trace[3], 1ull); atomicAdd(&p.trace[4], (unsigned long long)blocks);
  }
};
#else
struct BandStamps {
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void mark_loads_landed(int) {}
  __device__ __forceinline__ void cycle(int) {}
  __device__ __forceinline__ void cycle_lds_landed(int) {}
  __device__ __forceinline__ void block_done() {}
  __device__ __forceinline__ void add_block_phases(const GmmParams &, bool) {}
  __device__ __forceinline__ void add_kernel_phases(const GmmParams &, bool, int) {}
};
#endif

// The band kernel: see the head of this file.  One wavefront per (utterance, 64-frame sub-tile[, run of class 0 | chunk]).
// kStrided = false, the per-window launches of the first tier: a full grid, the wavefront's one item follows from its
// workgroup (band_item).  kStrided = true, every scoring launch of a list pass and every window's bf16×3 redo sweep —
// launches that find work for a handful of wavefronts, or for none: a small fixed grid (mfa_list_grid) whose wavefronts
// walk the items first, first + stride, … (band_walk).  A full grid there is workgroups that claim four wavefronts of
// ≈200 VGPRs and 33 KB of LDS to read one word and leave.  Same items, same arithmetic; the wavefront's stage passes from
// one item to the next behind the flush's wavefront-scope fences.  The body is one `do` block, left with `continue`:
// for kStrided = false it runs once and compiles to the code the kernel had before it could walk.
template <int kSteps, int kPieces, bool kStrided = false>
__global__ __launch_bounds__(256, 2) void gmm_band_kernel(GmmParams p) {
  using Ops = SplitOps<kPieces>;
  using op8 = typename Ops::op8;
  constexpr bool kHalf = Ops::kHalf;
  constexpr int kUnits = kSteps * kPieces * 2 * 32;    // 16-byte units per block
  __shared__ float stage_all[4][64 * 33];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *stage = stage_all[wave];
  BandWalk walk = {0, 0, 0, 0};
  if constexpr (kStrided) walk = band_walk(p, wave, true);
  const int grp = kStrided ? walk.grp : (p.b_split ? band_split_block(p).y : 0);   // the run of class 0 this wavefront scores
  // The walk.  A redo sweep without a list (utterance = item: the item's flag is redo[witem]) reads the flags of 64 items
  // at a time, one per lane, and visits only the flagged ones — one memory trip per 64 items instead of three dependent
  // ones per item (done word, frame offsets, flag).  A visited item still passes every exit below, its flag among them.
  const bool sweep = kStrided && !kHalf && p.redo_mode == 2 && p.b_utt_list == nullptr;
  int witem = walk.first - walk.stride, blk = (walk.first - walk.stride) * 64;
  unsigned long long flagged = 0ull;
  auto next_item = [&]() -> bool {
    if (!sweep) { witem += walk.stride; return witem < walk.n_witems; }
    while (flagged == 0ull) {
      blk += walk.stride * 64;
      if (blk >= walk.n_witems) return false;
      flagged = __ballot(blk + lane < walk.n_witems && p.redo[blk + lane] != 0);
    }
    witem = blk + __ffsll((long long)flagged) - 1;
    flagged &= flagged - 1ull;
    return true;
  };
  if (kStrided && !next_item()) return;
  do {
    BandStamps stamps;
    stamps.mark(0);
    int utt, r, chunk = 0;
    if (!(kStrided ? band_witem(p, witem, utt, r, &chunk) : band_item(p, wave, utt, r, &chunk))) continue;
    const int64_t f0 = p.frame_off[utt];
    const int T = (int)(p.frame_off[utt + 1] - f0);
    const int t_base = band_t_begin(p, utt) + 64 * r;
    if (t_base >= T) continue;
    int *redo_flag = p.redo + ((size_t)utt * p.b_sub + r) * p.b_nchunk + chunk;
    if (!kHalf && p.redo_mode == 2 && *redo_flag == 0) continue;        // only what the f16 pass declined
    const int col = lane & 31, h = lane >> 5;
    const int64_t l0 = p.pdf_off[utt];
    const int P = (int)(p.pdf_off[utt + 1] - l0);
    const int32_t *list = p.pdf_list + l0;
    const int32_t *cc6 = p.class_counts + (size_t)utt * 6;
    // The pre-split operands depend on nothing but the sub-tile: requested first, they travel while the band is looked up
    // (volatile: the loads stay here instead of sinking below the early exit).
    op8 b[2][kSteps][kPieces];
    bool bad = false;
    const bool presplit = kHalf && p.xsplit != nullptr;
    if (presplit) {
      const int64_t ti = xsplit_tile_index(f0, utt, t_base >> 6);
      const uint4 *src = p.xsplit + ti * (2 * kSteps * 2 * 64) + lane;
#pragma unroll
      for (int n = 0; n < 2; n++)
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++)
#pragma unroll
          for (int q = 0; q < kPieces; q++) {
            // (measured: non-temporal loads here keep more of the model in L2 — FETCH_SIZE 30 → 24.5 GB per step — but the
            // kernel is 3 % slower, the throughput unchanged)
            uint4 v;
            const volatile uint4 *a4 = src + ((n * kSteps + s_) * 2 + (q & 1)) * 64;
            v.x = a4->x; v.y = a4->y; v.z = a4->z; v.w = a4->w;
            b[n][s_][q] = __builtin_bit_cast(op8, v);
          }
      bad = p.xsplit_bad[ti] != 0;
    }
    // band range [lo, hi) of every class this kernel scores: 0 (one 32-row block per pdf), 1 (several blocks per pdf) and 2, 3, 4
    // (16-, 8-, 4-row slots); class 5 (single Gaussians) is the f32 band kernel's
    int lo_c[5], hi_c[5], base_c[5];
    // the band's lower depth bound, read as gmm_band_ranges_kernel reads it (lag windows included): class 0 tests every
    // column's own last depth against it
    const int band_lo = band_of(p, utt).lo;
    {   // looked up once per utterance and window by gmm_band_ranges_kernel
      const int32_t *rg = p.ranges + (size_t)utt * kRangeSlots * 2;
      int off = 0;
#pragma unroll
      for (int cls = 0; cls < 5; cls++) {
        const int slot = cls == 0 ? grp : (cls == 1 ? kRunSlots + 3 : kRunSlots + cls - 2);
        base_c[cls] = off; off += cc6[cls];
        lo_c[cls] = rg[2 * slot]; hi_c[cls] = rg[2 * slot + 1];
      }
    }
    if (p.b_chunk > 0) {                                 // list passes: this wavefront's share of the band (class 0 in chunks,
      lo_c[0] += chunk * p.b_chunk;                      // the small-slot classes with chunk 0)
      hi_c[0] = min(hi_c[0], lo_c[0] + p.b_chunk);
      if (chunk != 0) { hi_c[2] = lo_c[2]; hi_c[3] = lo_c[3]; hi_c[4] = lo_c[4]; }
    }
    if (p.b_split) {
      // the small-slot classes have no runs: the virtual blocks (32 / slot pdfs each) of their three bands, laid end to end,
      // are cut into `groups` pieces, one per wavefront of the sub-tile — all of them on run 0's wavefront would be all of
      // them on one XCD, and a piece of every class on every wavefront (the first version) was three pipelines to fill and
      // drain per wavefront, three or four blocks each: a piece now lies inside one class, rarely two
      int nb_c[5], tot = 0;
#pragma unroll
      for (int cls = 2; cls < 5; cls++) {
        const int kp = cls == 2 ? 2 : (cls == 3 ? 4 : 8);
        nb_c[cls] = (hi_c[cls] + kp - 1) / kp - lo_c[cls] / kp;
        if (lo_c[cls] >= hi_c[cls]) nb_c[cls] = 0;
        tot += nb_c[cls];
      }
      const int per = (tot + p.groups - 1) / p.groups;
      const int w0 = grp * per, w1 = min(tot, w0 + per);
      int pos = 0;
#pragma unroll
      for (int cls = 2; cls < 5; cls++) {
        const int kp = cls == 2 ? 2 : (cls == 3 ? 4 : 8);
        const int jb0 = lo_c[cls] / kp;
        const int a = jb0 + max(w0 - pos, 0), b = jb0 + min(w1 - pos, nb_c[cls]);
        pos += nb_c[cls];
        if (a >= b) hi_c[cls] = lo_c[cls];
        else { lo_c[cls] = max(lo_c[cls], a * kp); hi_c[cls] = min(hi_c[cls], b * kp); }
      }
    }
    // class 1 (pdfs of more than 32 Gaussians, few): its band's columns go round the sub-tile's wavefronts one by one
    const int step1 = p.b_split ? p.groups : (p.b_chunk > 0 ? p.b_nchunk : 1);
    const int first1 = lo_c[1] + (p.b_split ? grp : (p.b_chunk > 0 ? chunk : 0));
    const int lo = lo_c[0], hi = hi_c[0];
    if (lo >= hi && first1 >= hi_c[1] && lo_c[2] >= hi_c[2] && lo_c[3] >= hi_c[3] && lo_c[4] >= hi_c[4]) {
      if (kHalf && lane == 0) *redo_flag = 0;
      continue;
    }
    stamps.mark(1);
    if (!presplit) bad = split_features<kSteps, kPieces>(p, f0, T, t_base, col, h, b);
    stamps.mark_loads_landed(2);
    if constexpr (kHalf) {
      const bool any_bad = __ballot(bad) != 0ull;
      if (lane == 0) *redo_flag = any_bad ? 1 : 0;
      if (any_bad) continue;                                             // a scaled feature left the f16 range: bf16×3 pass
    }
    const float inv_s = kHalf ? p.acc_scale_inv : 1.0f;
    const float l2e_s = 1.44269504088896341f * inv_s;
    float *out = p.out + p.ll_off[utt];
    // Three pieces this kernel keeps in its own words, because the instruction text of its hot instantiations (<5, 2> and
    // <6, 2>, full grid) changes — by a scalar instruction's place or two — when it calls the shared ones: the product loop of
    // a step (SplitOps::mfma_step; the order table is the shared one), the accumulator seed from the gconst registers
    // (init_from_gconst) and this flush (flush_staged), all in gmm_common.hpp.  Change them together.
    constexpr int kProd = Ops::kProd;
    // the staged columns whose bit is set in `cols` (bit 0: score column c0 of the utterance's matrix) → HBM as 128-byte row
    // segments; a column without its bit was not staged and keeps what the matrix held
    auto flush_cols = [&](int c0, uint32_t cols) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const bool mine = ((cols >> col) & 1u) != 0u;
#pragma unroll 4
      for (int i = 0; i < 32; i++) {
        const int rr = h + 2 * i, t = t_base + rr;
        if (mine && t < T) __builtin_nontemporal_store(stage[rr * 33 + col], &out[(size_t)t * P + c0 + col]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    };

    // ---------------------------------------------------------------- class 0: one pdf per 32-row block
    int blocks0 = 0;                                             // blocks visited (the stamps' count)
    if (lo < hi) {
      const uint4 *wsrc = (kHalf ? p.wh : p.wb) + lane;
      const float *gsrc = (kHalf ? p.gch : p.gc) + 4 * h;
      const int last = hi - 1;
      // First model row per column, precomputed per batch: ONE load.  The pdf id → row chain it replaces (row0[list[j]]) made
      // the second load wait for the first — the youngest entry of the in-order vmcnt queue — i.e. drained every outstanding
      // operand load of the next block at the top of each block.
      const int32_t *crow = p.col_row0 + l0;
      const int32_t *cown = p.col_own_last + l0;
      // The range is walked in staging windows of 32 columns (the flush unit) from `lo`.  Per window, lane i holds column
      // j0 + i's row word and own last depth — one coalesced trip — and the wavefront derives two masks from them:
      //   need: columns a token can ask for — own last depth ≥ the band's lower bound.  The range keeps a column as long as
      //         an earlier column of the run spans further (last_depth is a running maximum); a token on state s has
      //         band.lo ≤ depth(s), an arc of column c leaving s has depth(s) ≤ own_last(c): own_last(c) < band.lo is never read;
      //   uniq: of those, the first occurrence of each row word.  A pdf met again more than a cluster span deeper has a
      //         second column in the same run (pdf mod groups): the same block, the same 64 scores.
      // The block loop visits the bits of uniq; a repeat gets the staged scores of its first occurrence before the flush
      // (the bits a second evaluation would give), and the flush stores the needed columns only.
      auto win_words = [&](int j0, int &rw, int &ol) {           // (past the range: the last column again, masked by win_masks)
        const int idx = min(j0 + col, last);
        rw = crow[idx]; ol = cown[idx];
      };
      auto win_masks = [&](int j0, int rw, int ol, int &first, uint32_t &need) -> uint32_t {
        need = (uint32_t)__ballot(lane < hi - j0 && lane < 32 && ol >= band_lo);
        first = col;
        for (uint32_t m = need; m != 0u; m &= m - 1u) {          // ascending: the lowest needed column with this lane's row word
          const int k = __builtin_ctz(m);
          if (__builtin_amdgcn_readlane(rw, k) == rw && k < first) first = k;
        }
        return (uint32_t)__ballot(lane < 32 && ((need >> col) & 1u) != 0u && first == col);
      };
      int j0 = lo, rw, ol, first;
      uint32_t need, uniq;
      win_words(j0, rw, ol);
      uniq = win_masks(j0, rw, ol, first, need);
      while (uniq == 0u && j0 + 32 < hi) { j0 += 32; win_words(j0, rw, ol); uniq = win_masks(j0, rw, ol, first, need); }
      op8 a[kSteps][kPieces];
      f32x4 g[4];
      if (uniq != 0u) {
        const int blk = __builtin_amdgcn_readlane(rw, __builtin_ctz(uniq)) >> 5;
        const uint4 *src = wsrc + (size_t)blk * kUnits;
#pragma unroll
        for (int q = 0; q < 4; q++) g[q] = *reinterpret_cast<const f32x4 *>(gsrc + (size_t)blk * 32 + 8 * q);
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++)
#pragma unroll
          for (int q = 0; q < kPieces; q++) a[s_][q] = __builtin_bit_cast(op8, src[(s_ * kPieces + q) * 64]);
      }
      while (uniq != 0u) {                                       // one staging window with blocks to score per round
        // the next window's words, requested ahead of this window's operand loads (the oldest entries of the in-order vmcnt
        // queue by the time the window's last block asks for them)
        int j0_n = j0 + 32, rw_n, ol_n, first_n = 0;
        uint32_t need_n = 0u, uniq_n = 0u;
        win_words(j0_n, rw_n, ol_n);
        uint32_t rest = uniq;
        blocks0 += __builtin_popcount(uniq);
        do {
        stamps.cycle(0);
        const int c = __builtin_ctz(rest);                       // staged column = the bit's position
        rest &= rest - 1u;
        int blk_next;                                            // the next visited block: of this window, or the first of the next
        if (rest != 0u) blk_next = __builtin_amdgcn_readlane(rw, __builtin_ctz(rest)) >> 5;
        else {
          if (j0_n < hi) {
            uniq_n = win_masks(j0_n, rw_n, ol_n, first_n, need_n);
            while (uniq_n == 0u && j0_n + 32 < hi) { j0_n += 32; win_words(j0_n, rw_n, ol_n); uniq_n = win_masks(j0_n, rw_n, ol_n, first_n, need_n); }
          }
          // (nothing follows: the same block again, unused)
          blk_next = (uniq_n != 0u ? __builtin_amdgcn_readlane(rw_n, __builtin_ctz(uniq_n)) : __builtin_amdgcn_readlane(rw, c)) >> 5;
        }
        f32x16 init, acc[2];
#pragma unroll
        for (int rr = 0; rr < 16; rr++) init[rr] = g[rr >> 2][rr & 3];
        const uint4 *src = wsrc + (size_t)blk_next * kUnits;
        const float *gn = gsrc + (size_t)blk_next * 32;
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++) {
#pragma unroll
          for (int t6 = 0; t6 < kProd; t6++)
#pragma unroll
            for (int n = 0; n < 2; n++) {
              const f32x16 &cin = (s_ == 0 && t6 == 0) ? init : acc[n];
              if constexpr (kHalf) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s_][Ops::pa(t6)], b[n][s_][Ops::pb(t6)], cin, 0, 0, 0);
              else acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s_][Ops::pa(t6)], b[n][s_][Ops::pb(t6)], cin, 0, 0, 0);
            }
          // this step's operand registers (and, after the first step, the gconst registers) are free: next block's rows.
          // (A second operand set — two blocks in flight per wavefront — was measured: 12.70 vs 12.76 ms per step; the
          //  kernel is bound by what the fabric delivers, ≈6.5 TB/s of 10 KiB blocks gathered from a 51 MB table.)
          if (s_ == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) g[q] = *reinterpret_cast<const f32x4 *>(gn + 8 * q);
          }
#pragma unroll
          for (int q = 0; q < kPieces; q++) a[s_][q] = __builtin_bit_cast(op8, src[(s_ * kPieces + q) * 64]);
          __builtin_amdgcn_sched_barrier(0);
        }
        stamps.cycle(1);
        stamps.cycle(2);
        const Lse lse0 = block_lse(acc[0], h, l2e_s), lse1 = block_lse(acc[1], h, l2e_s);
        stage[(32 * h + col) * 33 + c] = finish((h ? lse1.m : lse0.m) * inv_s, h ? lse1.s : lse0.s);
        stamps.cycle_lds_landed(3);
        if (rest == 0u) {
          // repeats: every lane copies its own staged row (row 32 h + col = lane) from the first occurrence's column —
          // lane-local LDS traffic, program order suffices
          for (uint32_t m = need & ~uniq; m != 0u; m &= m - 1u) {
            const int k = __builtin_ctz(m);
            stage[lane * 33 + k] = stage[lane * 33 + __builtin_amdgcn_readlane(first, k)];
          }
          flush_cols(j0, need);
        }
        stamps.cycle(4);
        stamps.block_done();
        } while (rest != 0u);
        j0 = j0_n; rw = rw_n; first = first_n; need = need_n; uniq = uniq_n;
      }
      stamps.add_block_phases(p, lane == 0 && kHalf);
    }

    // ---------------------------------------------------------------- class 1: several 32-row blocks per pdf
    // Online log-sum-exp over the pdf's blocks (running max M and sum S against it, per frame): (M, S) ← (max(M, m_b),
    // S·2^((M − M')·l2e) + s_b·2^((m_b − M')·l2e)).  Products and per-block reductions are class 0's; pad rows carry gconst
    // −1e30 and vanish in the sum.  No software pipeline: a trained model has a few such pdfs per band, if any.
    // Software pipeline as class 0's: the operands of the next block — the pdf's next one, or the first block of this
    // wavefront's next column — are requested as soon as a step's MFMAs have been issued; the column's (row, blocks) word is
    // looked up one column ahead.
    if (first1 < hi_c[1]) {
      const uint4 *wsrc = (kHalf ? p.wh : p.wb) + lane;
      const float *gsrc = (kHalf ? p.gch : p.gc) + 4 * h;
      const int32_t *crow1 = p.col_row0 + l0 + base_c[1];
      const int last1 = hi_c[1] - 1;
      auto col_word = [&](int jj) { return crow1[min(jj, last1)]; };     // row | (blocks − 1) when packed
      auto blocks_of = [&](int word, int jj) {
        return p.col_nb_packed ? (word & 31) + 1 : __builtin_amdgcn_readfirstlane(p.nblk[list[base_c[1] + min(jj, last1)]]);
      };
      int j1 = first1;
      int word = __builtin_amdgcn_readfirstlane(col_word(j1));
      int nb = blocks_of(word, j1), blk = word >> 5, bk = 0;
      int word_n = col_word(j1 + step1);                                 // stays a vector register until its column opens
      op8 a[kSteps][kPieces];
      f32x4 g[4];
      {
        const uint4 *src = wsrc + (size_t)blk * kUnits;
#pragma unroll
        for (int q = 0; q < 4; q++) g[q] = *reinterpret_cast<const f32x4 *>(gsrc + (size_t)blk * 32 + 8 * q);
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++)
#pragma unroll
          for (int q = 0; q < kPieces; q++) a[s_][q] = __builtin_bit_cast(op8, src[(s_ * kPieces + q) * 64]);
      }
      float M[2] = {0.0f, 0.0f}, S[2] = {0.0f, 0.0f};
      for (;;) {
        const bool last_blk = bk + 1 == nb;
        const bool more_cols = j1 + step1 < hi_c[1];
        int blk_n = blk + 1;                                             // (past the pdf's last block only when nothing follows:
        if (last_blk) blk_n = more_cols ? __builtin_amdgcn_readfirstlane(word_n) >> 5 : blk;   //  then the same block again, unused)
        f32x16 init, acc[2];
#pragma unroll
        for (int rr = 0; rr < 16; rr++) init[rr] = g[rr >> 2][rr & 3];
        const uint4 *src = wsrc + (size_t)blk_n * kUnits;
        const float *gn = gsrc + (size_t)blk_n * 32;
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++) {
#pragma unroll
          for (int t6 = 0; t6 < kProd; t6++)
#pragma unroll
            for (int n = 0; n < 2; n++) {
              const f32x16 &cin = (s_ == 0 && t6 == 0) ? init : acc[n];
              if constexpr (kHalf) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s_][Ops::pa(t6)], b[n][s_][Ops::pb(t6)], cin, 0, 0, 0);
              else acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s_][Ops::pa(t6)], b[n][s_][Ops::pb(t6)], cin, 0, 0, 0);
            }
          if (s_ == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) g[q] = *reinterpret_cast<const f32x4 *>(gn + 8 * q);
          }
#pragma unroll
          for (int q = 0; q < kPieces; q++) a[s_][q] = __builtin_bit_cast(op8, src[(s_ * kPieces + q) * 64]);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int n = 0; n < 2; n++) {
          const Lse l = block_lse(acc[n], h, l2e_s);
          if (bk == 0) { M[n] = l.m; S[n] = l.s; }
          else lse_merge(M[n], S[n], l.m, l.s, l2e_s);
        }
        blk = blk_n;
        if (!last_blk) { bk++; continue; }
        const int t = t_base + 32 * h + col;
        if (t < T) __builtin_nontemporal_store(finish((h ? M[1] : M[0]) * inv_s, h ? S[1] : S[0]), &out[(size_t)t * P + base_c[1] + j1]);
        if (!more_cols) break;
        j1 += step1;
        word = __builtin_amdgcn_readfirstlane(word_n);
        nb = blocks_of(word, j1); bk = 0;
        word_n = col_word(j1 + step1);
      }
    }

    // ---------------------------------------------------------------- classes 2, 3, 4: 32 / slot pdfs per virtual block
    // As gmm_split_small_kernel: the pdfs the list puts next to each other are gathered into one 32-row block (lane ↔ row
    // ρ = lane mod 32 → pdf ρ / slot, its row ρ mod slot; rows past the range come from the model's dummy row), the MFMAs
    // are those of class 0, the log-sum-exp runs over the slot's rows of each pdf — per pdf the very same expressions, so a
    // cell scored here carries the dense kernel's bits.  The gather costs nothing extra: every lane loads through its own
    // row pointer anyway.
    auto run_small = [&](auto slot_c, int base, int lo_s, int hi_s) {
      constexpr int kSlot = decltype(slot_c)::value, kPdfs = 32 / kSlot;
      if (lo_s >= hi_s) return;
      const uint4 *wsrc = kHalf ? p.wh : p.wb;
      const float *gsrc = kHalf ? p.gch : p.gc;
      const int rho = lane & 31, my_k = rho / kSlot, my_r = rho % kSlot;
      const int jb0 = lo_s / kPdfs, jb1 = (hi_s + kPdfs - 1) / kPdfs;
      auto row_of = [&](int jb) -> int {                 // this lane's packed row in virtual block jb (two dependent loads)
        const int idx = min(jb, jb1 - 1) * kPdfs + my_k;
        return idx < hi_s ? p.col_row0[l0 + base + idx] + my_r : p.num_rows;
      };
      auto src_of = [&](int row) { return wsrc + (size_t)(row >> 5) * kUnits + (row & 31) + 32 * h; };
      op8 a[kSteps][kPieces];
      int row_cur = row_of(jb0), row_next = row_of(jb0 + 1);
      float gcv = gsrc[row_cur];
      {
        const uint4 *src = src_of(row_cur);
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++)
#pragma unroll
          for (int q = 0; q < kPieces; q++) a[s_][q] = __builtin_bit_cast(op8, src[(s_ * kPieces + q) * 64]);
      }
      const int col0 = base + jb0 * kPdfs;               // score column of the first staged column
      for (int jb = jb0; jb < jb1; jb++) {
        const int row_n2 = row_of(jb + 2);               // in flight during this block
        f32x16 init, acc[2];
#pragma unroll
        for (int rr = 0; rr < 16; rr++) init[rr] = __shfl(gcv, acc_row(rr, h));
        const uint4 *src = src_of(row_next);
#pragma unroll
        for (int s_ = 0; s_ < kSteps; s_++) {
#pragma unroll
          for (int t6 = 0; t6 < kProd; t6++)
#pragma unroll
            for (int n = 0; n < 2; n++) {
              const f32x16 &cin = (s_ == 0 && t6 == 0) ? init : acc[n];
              if constexpr (kHalf) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s_][Ops::pa(t6)], b[n][s_][Ops::pb(t6)], cin, 0, 0, 0);
              else acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s_][Ops::pa(t6)], b[n][s_][Ops::pb(t6)], cin, 0, 0, 0);
            }
          if (s_ == 0) gcv = gsrc[row_next];
#pragma unroll
          for (int q = 0; q < kPieces; q++) a[s_][q] = __builtin_bit_cast(op8, src[(s_ * kPieces + q) * 64]);
          __builtin_amdgcn_sched_barrier(0);
        }
        row_next = row_n2;
        small_slot_scores<kSlot>(acc, stage, col, ((jb - jb0) * kPdfs) & 31, h, inv_s, l2e_s);
        const int done = (jb - jb0 + 1) * kPdfs;         // staged columns since col0 (whole blocks)
        if ((done & 31) == 0 || jb == jb1 - 1) {
          const int first = (done - 1) & ~31;            // first staged column of the open window
          const int valid = min(done, hi_s - jb0 * kPdfs) - first;   // columns of pdfs inside the class's range
          flush_cols(col0 + first, valid >= 32 ? ~0u : (1u << valid) - 1u);
        }
      }
    };
    run_small(std::integral_constant<int, 16>{}, base_c[2], lo_c[2], hi_c[2]);
    run_small(std::integral_constant<int, 8>{}, base_c[3], lo_c[3], hi_c[3]);
    run_small(std::integral_constant<int, 4>{}, base_c[4], lo_c[4], hi_c[4]);
    stamps.add_kernel_phases(p, lane == 0 && kHalf, blocks0);
    if constexpr (kStrided) {                            // the stage goes to the wavefront's next item
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  } while (kStrided && next_item());
}

}  // namespace

// Block counts of multi-block pdfs ride in the five low bits of their columns' row words when every pdf has at most 32 blocks
// (MFA_GMM_PACK_NB=0: never — the lookup path, for tests)
static int col_nb_packed_for(const mfa_ctx *c) {
  const char *e = getenv("MFA_GMM_PACK_NB");
  if (e && e[0] == '0') return 0;
  return c->max_nblk <= 32 ? 1 : 0;
}

int mfa_gmm_lazy_supported(mfa_ctx *c) { return c->gmm_ready && (c->kpad == 80 || c->kpad == 96); }

// Pre-split f16 operands of the whole batch (see gmm_presplit_kernel); mfa_gmm_score_window then hands them to the band kernel.
int mfa_gmm_presplit(mfa_ctx *c, const MfaLazyScoring *lazy, const mfa_graph_batch *g, const int64_t *d_frame_off, int n_utt,
                     int64_t total_frames) {
  c->xsplit_ready = false;
  {   // first model row of every score column of the batch (the band kernels read nothing else to find a block), and the
      // column's own last depth.  The latter comes from what the decoder is handed anyway — the graph batch's arcs and their
      // columns, the plan's state depths — rather than from a new output of mfa_build_score_plan*: no exported signature and
      // nothing in the host's packing changes, and it is one launch per batch over arrays already on the device.
    const int64_t cols_cap = (int64_t)n_utt * std::max(1, lazy->plan.max_cols);
    if (c->d_col_row0.reserve(c, (size_t)cols_cap * sizeof(int32_t), "the score columns' row table")) return -1;
    if (c->d_col_own_last.reserve(c, (size_t)cols_cap * sizeof(int32_t), "the score columns' own last depths")) return -1;
    hipLaunchKernelGGL(gmm_col_own_last_kernel, dim3(n_utt), dim3(256), 0, c->stream, *g, lazy->plan.d_state_depth, lazy->plan.d_pdf_off,
                       c->d_col_own_last.ptr<int32_t>());
    GmmParams q;
    memset(&q, 0, sizeof(q));
    q.row0 = c->d_row0.ptr<int32_t>(); q.pdf_list = lazy->plan.d_pdf_list; q.pdf_off = lazy->plan.d_pdf_off; q.n_utt = n_utt;
    q.nblk = c->d_nblk.ptr<int32_t>(); q.col_nb_packed = col_nb_packed_for(c);
    hipLaunchKernelGGL(gmm_col_rows_kernel, dim3(n_utt), dim3(256), 0, c->stream, q, c->d_col_row0.ptr<int32_t>());
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  if (!gmm_split_passes(c).f16) return 0;   // no f16 pass (its operands exist for rows of 80 or 96 floats only): nothing to prepare
  const int64_t tiles = (total_frames >> 6) + n_utt + 1;
  if (c->d_xsplit.reserve(c, (size_t)tiles * 2 * 6 * 2 * 64 * 16, "the pre-split feature operands") ||
      c->d_xsplit_bad.reserve(c, (size_t)tiles * sizeof(int), "the pre-split tiles' range flags")) return -1;
  GmmParams p;
  memset(&p, 0, sizeof(p));
  p.dim = c->dim; p.kpad = c->kpad; p.feats = lazy->d_feats; p.frame_off = d_frame_off; p.n_utt = n_utt; p.fscale = c->d_fscale.ptr<float>();
  const int tiles_per_utt = ((lazy->max_frames + 255) / 256) * 4;   // whole 256-frame tiles: a workgroup each (gmm_presplit_kernel)
  const int64_t waves = (int64_t)n_utt * tiles_per_utt;
  const dim3 grid((unsigned)((waves + 3) / 4));
  KernelTimer kt(c, MFA_K_GMM);
  gmm_with_steps(c->kpad, [&](auto steps) {
    hipLaunchKernelGGL((gmm_presplit_kernel<steps()>), grid, dim3(256), 0, c->stream, p, c->d_xsplit.ptr<uint4>(), c->d_xsplit_bad.ptr<int>(), tiles_per_utt);
  });
  MFA_HIP_CHECK(c, hipGetLastError());
  c->xsplit_ready = true;
  return 0;
}

const int32_t *mfa_band_ranges(mfa_ctx *c) { return c->d_band_ranges.ptr<int32_t>(); }

int mfa_gmm_score_window(mfa_ctx *c, const MfaLazyScoring *lazy, const MfaWindowScore *ws, const int64_t *d_frame_off,
                         int n_utt, const int64_t *d_ll_off, float *d_loglikes) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  if (!mfa_gmm_lazy_supported(c)) return c->fail("lazy scoring needs a model of at most 48 dimensions");
  if (ws->window <= 0 || ws->window % 64 != 0) return c->fail("scoring window must be a multiple of 64 frames");
  GmmParams p;
  memset(&p, 0, sizeof(p));
  p.dim = c->dim; p.kpad = c->kpad; p.num_rows = c->num_rows;
  p.w = c->d_w.ptr<float>(); p.gc = c->d_gc.ptr<float>(); p.row0 = c->d_row0.ptr<int32_t>(); p.nblk = c->d_nblk.ptr<int32_t>(); p.slot = c->d_slot.ptr<int32_t>();
  p.feats = lazy->d_feats; p.frame_off = d_frame_off; p.pdf_list = lazy->plan.d_pdf_list; p.pdf_off = lazy->plan.d_pdf_off;
  p.class_counts = lazy->plan.d_class_counts; p.ll_off = d_ll_off; p.out = d_loglikes;
  p.min_log_diff = logf(1.1920928955078125e-07f);
  p.first_frame = lazy->plan.d_pdf_first_frame; p.last_depth = lazy->plan.d_pdf_last_depth;
  p.n_utt = n_utt; p.tiles = 0;
  p.acc_scale_inv = 1.0f;
  p.trace = (unsigned long long *)c->gmm_trace;
  p.b_hi_slack = ws->hi_slack > 0 ? ws->hi_slack : 0;
  p.b_mode = 1; p.b_t_begin = ws->t_begin; p.b_sub = ws->window / 64; p.b_band = ws->band;
  p.b_utt_list = ws->utt_list; p.b_n_list = ws->n_list;
  p.b_done = ws->done; p.b_done_stride = ws->done_stride; p.b_done_word = ws->done_word;
  p.b_lag = ws->lag; p.b_lag_stride = ws->lag_stride; p.b_lag_word = ws->lag_word; p.b_lag_frames = ws->window;
  const int64_t waves = (int64_t)n_utt * p.b_sub;
  const dim3 grid((unsigned)((waves + 3) / 4));
  p.groups = lazy->plan.groups > 1 && lazy->plan.d_group_counts ? lazy->plan.groups : 0;
  p.group_counts = p.groups ? lazy->plan.d_group_counts : nullptr;
  p.b_chunk = (ws->cols_per_wave > 0 && !p.groups) ? ws->cols_per_wave : 0;   // (a grouped plan already spreads the band over `groups` wavefronts)
  p.b_nchunk = p.b_chunk > 0 ? (lazy->plan.max_cols + p.b_chunk - 1) / p.b_chunk : 1;
  const int64_t split_waves = waves * p.b_nchunk;
  p.b_split = p.groups > 1 ? 1 : 0;
  const dim3 split_grid((unsigned)((split_waves + 3) / 4) * (unsigned)(p.b_split ? p.groups : 1));
  const GmmSplitPasses passes = gmm_split_passes(c);
  // Launches that find work for a handful of wavefronts or for none — everything a list pass scores, and each window's
  // redo sweep — walk their items on a small fixed grid (mfa_list_grid) instead of asking for one wavefront per item.
  const bool list_pass = ws->utt_list != nullptr;
  const int walk = mfa_list_grid(c);
  if (walk <= 0) return -1;
  const unsigned runs = p.b_split ? (unsigned)p.groups : 1u;
  const unsigned full_per_run = std::max(1u, (unsigned)((split_waves + 3) / 4));
  const dim3 walk_grid(std::min(((unsigned)walk + runs - 1) / runs, full_per_run) * runs);
  const dim3 walk_grid_f32(std::min((unsigned)walk, std::max(1u, grid.x)));
  KernelTimer kt(c, MFA_K_GMM);
  {   // the band's index ranges, once per utterance (instead of once per scoring wavefront)
    if (c->d_band_ranges.reserve(c, (size_t)n_utt * kRangeSlots * 2 * sizeof(int32_t), "the band's index ranges")) return -1;
    p.ranges = c->d_band_ranges.ptr<int32_t>();
    hipLaunchKernelGGL(gmm_band_ranges_kernel, dim3((unsigned)((n_utt + 3) / 4)), dim3(256), 0, c->stream, p);
  }
  const bool split_classes = c->has_single32 || c->has_multi_block || c->has_slot_class[1] || c->has_slot_class[2] || c->has_slot_class[3];
  if (passes.bf16 && split_classes) {
    if (c->d_gmm_redo.reserve(c, (size_t)split_waves * sizeof(int), "the scoring redo list")) return -1;
    p.redo = c->d_gmm_redo.ptr<int>();
    p.wb = c->d_wb.ptr<const uint4>();
    p.col_row0 = c->d_col_row0.ptr<int32_t>(); p.col_own_last = c->d_col_own_last.ptr<int32_t>();
    p.col_nb_packed = col_nb_packed_for(c);
    if (passes.f16) {
      p.wh = c->d_wh.ptr<const uint4>(); p.gch = c->d_gch.ptr<float>(); p.fscale = c->d_fscale.ptr<float>();
      p.acc_scale_inv = 1.0f / c->gmm_acc_scale;
      p.redo_mode = 0;
      if (c->xsplit_ready) { p.xsplit = c->d_xsplit.ptr<const uint4>(); p.xsplit_bad = c->d_xsplit_bad.ptr<int>(); }
      gmm_with_steps(c->kpad, [&](auto steps) {
        if (list_pass) hipLaunchKernelGGL((gmm_band_kernel<steps(), 2, true>), walk_grid, dim3(256), 0, c->stream, p);
        else hipLaunchKernelGGL((gmm_band_kernel<steps(), 2>), split_grid, dim3(256), 0, c->stream, p);
      });
      p.redo_mode = 2;   // the sub-tiles the f16 pass flagged
    }
    gmm_with_steps(c->kpad, [&](auto steps) {
      if (list_pass || p.redo_mode == 2) hipLaunchKernelGGL((gmm_band_kernel<steps(), 3, true>), walk_grid, dim3(256), 0, c->stream, p);
      else hipLaunchKernelGGL((gmm_band_kernel<steps(), 3>), split_grid, dim3(256), 0, c->stream, p);
    });
    p.redo_mode = 0;
    p.b_skip0 = 1;
  }
  p.b_split = 0;   // (the f32 band kernel keeps one wavefront per sub-tile and walks the runs of class 0 itself)
  const bool f32_classes = c->has_slot_class[4];   // single Gaussians stay on the f32 pipe (bit-exact); everything else was scored above
  if (!p.b_skip0 || f32_classes) mfa_gmm_launch_band_f32(c, &p, list_pass ? walk_grid_f32 : grid, list_pass);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}
