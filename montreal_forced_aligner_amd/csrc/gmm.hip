// Diagonal-GMM acoustic scoring on gfx950's matrix pipe: the model packer (mfa_load_gmm), dense scoring of whole utterances
// (mfa_gmm_score_batch) and the exact-f32 tile walk both scoring modes use.  Kernels in this file:
//   gmm_kernel               exact-f32 MFMA (v_mfma_f32_32x32x2_f32): single-Gaussian pdfs, and everything under
//                            MFA_GMM_BF16=0 — the description below is this kernel's;
//   gmm_band_f32_kernel      the same tile walk (score_tile) launched over the band items of a lazy-scoring window
//                            (mfa_gmm_launch_band_f32, for gmm_band.hip);
//   gmm_split_single_kernel  pdfs that are one 32-row block (17–32 Gaussians): float32 products from two f16 (or three
//                            bf16) operand pieces on v_mfma_f32_32x32x16_{f16,bf16}, blocks shared through LDS;
//   gmm_split_small_kernel   the 16-, 8- and 4-row slot classes as gathered virtual 32-row blocks on the same pipe;
//   gmm_bf16_kernel          pdfs of more than 32 Gaussians: runs of blocks merged by an online log-sum-exp;
//   gmm_naive_kernel         one thread per (frame, pdf): feature dims beyond 48, and MFA_GMM_NAIVE=1 as a cross-check;
//   gmm_max_first_frame_kernel  the batch's largest first-reachable frame, for gmm_kernel's phase split.
// mfa_gmm_score_batch (end of file) decides which launches a model and the environment call for.  Lazy (windowed) scoring
// is gmm_band.hip; what the two units share is gmm_common.hpp.
// Replaces DecodableAmDiagGmmScaled::LogLikelihood / gmm_compute_likes (MFA/alignment/multiprocessing.py:846-853, :1415;
// Kaldi gmm/decodable-am-diag-gmm.cc, VectorBase<float>::LogSumExp).
//
// Per Gaussian:  ll = gconst + Σ_d means_invvars[d]·x[d] + Σ_d (−½ inv_vars[d])·x[d]²   — a [rows × 2D]·[2D × frames]
// contraction.  The MFMA accumulates a k-ordered fmaf chain starting from C = gconst, i.e. bit for bit the oracle's chain.
// Per pdf:       LL = max + log Σ_{ll ≥ max+ln ε} exp(ll − max)  (Kaldi: expf, double sum, log; here: hardware exp2/log2
//                and a float32 tree sum — within 1 ulp of the Kaldi value at score magnitudes ≥ 16, see reg_expsum).
//
// Packed model (built once in mfa_load_gmm): every pdf owns `slot` consecutive rows (slot ∈ {1,4,8,16,32·n}; pad rows have
// zero weights and gconst −1e30 so they fall under the cutoff).  Rows are stored in blocks of 32, operand-major
// (mfa_packed_offset in ctx.hpp): one 16-byte load per lane yields the A operands of four consecutive MFMA steps (lane l
// feeds A[row l&31][k = 2s + (l>>5)]), and the 32 lanes of a half-wavefront read 512 contiguous bytes.
// One 32-row MFMA block then serves 32/slot pdfs of the utterance's (slot-sorted) pdf list; rows ↔ accumulator registers:
// row = (r&3) + 8(r>>2) + 4(l>>5), so 4-row slots reduce inside a lane and 8/16/32-row slots add one cross-half shuffle.
//
// Work decomposition: 1-D grid of (utterance, 256-frame tile) workgroups dealt XCD-aware; a wavefront owns NT×32 frames,
// keeps their x̃ = [x, x²] operands in registers (the B side) and streams the utterance's model rows (the A side,
// L2/MALL-resident).  With reachability information (first_frame) a wavefront only walks the prefix of each class that
// its frames can be asked for.
// Output: [T][P_u] row-major, the layout the Viterbi kernel gathers from.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "gmm_common.hpp"

namespace {

constexpr float kPadGconst = -1.0e30f;   // gconst of pad rows: they fall under the log-sum-exp cutoff

// (f32 kernels: a wavefront owns kNT 32-frame tiles; a workgroup is kWaves wavefronts — template parameters)

// one past the last index (i0 + lane) whose bit is set in a 64-lane ballot, 0 if none
__device__ __forceinline__ int prefix_end(unsigned long long mask, int i0) { return mask ? i0 + 64 - __clzll((long long)mask) : 0; }

// address of the 4-float piece (operand group 0, half h) of a packed row: see mfa_packed_offset in ctx.hpp
__device__ __forceinline__ const float *row_ptr(const float *w, int kpad, int row, int h) {
  return w + (size_t)(row >> 5) * 32 * kpad + (h * 32 + (row & 31)) * 4;
}

template <int M8, int kNT>
struct Tile {
  // One wavefront: B operands for kNT frame tiles, generic block evaluation.
  float b[kNT][4 * M8];

  __device__ __forceinline__ void load_b(const GmmParams &p, int64_t f0, int T, int t_base, int lane) {
    const int col = lane & 31, h = lane >> 5;
#pragma unroll
    for (int n = 0; n < kNT; n++) {
      int t = t_base + 32 * n + col;
      t = t < T ? t : T - 1;
      const float *x = p.feats + (f0 + t) * p.dim;
      // branch-free (independent loads, one round trip): clamp the index, then select x, x² or the zero pad
#pragma unroll
      for (int s = 0; s < 4 * M8; s++) {
        const int k = 2 * s + h;
        const int idx = k < p.dim ? k : (k < 2 * p.dim ? k - p.dim : 0);
        const float xv = x[idx];
        b[n][s] = k < p.dim ? xv : (k < 2 * p.dim ? xv * xv : 0.0f);
      }
    }
  }

  // acc[n] = gconst(rows) + W(block rows) · x̃(tile n).  arow: this lane's A row (already offset by 4h floats);
  // gcv: gconst of the row this lane (lane&31) addresses.
  // arow: this lane's piece of operand group 0 (row_ptr below); group m lies 2·32·4 floats further on
  __device__ __forceinline__ static void load_a(const float *arow, f32x4 (&a)[M8]) {
#pragma unroll
    for (int m = 0; m < M8; m++) a[m] = *reinterpret_cast<const f32x4 *>(arow + 256 * m);
  }
  __device__ __forceinline__ void block(const float *arow, float gcv, int lane, f32x16 (&acc)[kNT]) const {
    f32x4 a[M8];
    load_a(arow, a);
    run(a, gcv, lane, acc);
  }
  // gconst of the accumulator rows of a contiguous, 4-row-aligned 32-row block: four 16-byte loads (rows 8q+4h..+3)
  __device__ __forceinline__ static void load_gc32(const float *gc_block, int h, f32x4 (&g)[4]) {
#pragma unroll
    for (int q = 0; q < 4; q++) g[q] = *reinterpret_cast<const f32x4 *>(gc_block + 8 * q + 4 * h);
  }
  __device__ __forceinline__ void run32(const f32x4 (&a)[M8], const f32x4 (&g)[4], f32x16 (&acc)[kNT]) const {
    f32x16 init;
#pragma unroll
    for (int r = 0; r < 16; r++) init[r] = g[r >> 2][r & 3];
    mfma(a, init, acc);
  }
  __device__ __forceinline__ void run(const f32x4 (&a)[M8], float gcv, int lane, f32x16 (&acc)[kNT]) const {
    const int h = lane >> 5;
    f32x16 init;
#pragma unroll
    for (int r = 0; r < 16; r++) init[r] = __shfl(gcv, acc_row(r, h));
    mfma(a, init, acc);
  }
  __device__ __forceinline__ void mfma(const f32x4 (&a)[M8], const f32x16 &init, f32x16 (&acc)[kNT]) const {
#pragma unroll
    for (int n = 0; n < kNT; n++) acc[n] = init;
#pragma unroll
    for (int m = 0; m < M8; m++) {
#pragma unroll
      for (int cc = 0; cc < 4; cc++) {
#pragma unroll
        for (int n = 0; n < kNT; n++)
          acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][cc], b[n][4 * m + cc], acc[n], 0, 0, 0);
      }
    }
  }
};

// log-sum-exp pieces (Kaldi LogSumExp semantics); reg_max, reg_expsum_fast and finish are in gmm_common.hpp
// Σ_r exp(v[r] − mx) over the rows r ∈ [R0, R1) that pass Kaldi's cutoff (v[r] ≥ max + ln ε).
// exp(x) = 2^(x·log2 e) on the hardware exp2 (≈1 ulp); the rounding of the product x·log2 e adds |x|·6e-8 relative
// error to a term, which only matters for terms that are themselves ≤ e^x of the sum — below 1e-7 of the total.
// The ≤16 terms per lane are added in float32 as a balanced tree (error ≲ 4 ulp of the sum, i.e. ≲ 2.5e-7 absolute on
// the log-likelihood — an order of magnitude below half an ulp of a float32 score of magnitude ≥ 16).  Round 1 summed
// in float64 after a 6-instruction exponential: measured, that epilogue cost as much VALU time as the MFMAs it follows.
template <int R0, int R1>
__device__ __forceinline__ float reg_expsum(const f32x16 &v, float mx, float cutoff) {
  constexpr int n = R1 - R0;
  float e[n];
#pragma unroll
  for (int r = 0; r < n; r++) {
    const float t = __builtin_amdgcn_exp2f((v[R0 + r] - mx) * 1.44269504088896341f);
    e[r] = v[R0 + r] >= cutoff ? t : 0.0f;
  }
#pragma unroll
  for (int w = 1; w < n; w <<= 1)
#pragma unroll
    for (int r = 0; r + w < n; r += 2 * w) e[r] += e[r + w];
  return e[0];
}

// One work item = (utterance, 64-frame tile): score_tile walks the utterance's pdf list for those frames.
template <int M8, int kNT>
__device__ __forceinline__ void score_tile(const GmmParams &p, int utt, int t_base, int lane, float *stage, int rec_index) {
  constexpr int kFramesPerWave = 32 * kNT;
  unsigned long long t_start = 0;
  if (p.trace) t_start = wall_clock64();
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  if (t_base >= T) return;
  const int col = lane & 31, h = lane >> 5;
  const int64_t l0 = p.pdf_off[utt];
  const int P = (int)(p.pdf_off[utt + 1] - l0);
  const int32_t *list = p.pdf_list + l0;
  const int32_t *cc6 = p.class_counts + (size_t)utt * 6;
  // class_counts[u] = {32-row single-block, 32-row multi-block, 16, 8, 4, 1}
  const int32_t cc[5] = {cc6[0] + cc6[1], cc6[2], cc6[3], cc6[4], cc6[5]};
  // need[c]: how many pdfs of class c this wavefront's frames can be asked for.  Without reachability information that
  // is all of them; with it, the pdfs whose first possible frame lies at or before the tile's last frame — a prefix of
  // the class, because the host ordered each class by that frame.
  int need[6], lo_[6];
  {
    int t_last = min(T, t_base + kFramesPerWave) - 1;
    int d_lo = 0;
    if (p.b_mode) { const Band bd = band_of(p, utt); t_last = bd.hi; d_lo = bd.lo; }
    int off = 0;
#pragma unroll
    for (int cls = 0; cls < 6; cls++) {
      const int cnt = cc6[cls];
      int nd = cnt, lw = 0;
      if (cls == 0 && p.groups > 1) { need[0] = 0; lo_[0] = 0; off += cnt; continue; }   // grouped plan: searched run by run below
      if (p.first_frame) {
        nd = 0;
        for (int i0 = 0; i0 < cnt; i0 += 64) {
          const int i = i0 + lane;
          const bool ok = i < cnt && p.first_frame[l0 + off + i] <= t_last;
          nd = max(nd, prefix_end(__ballot(ok), i0));   // = the count for a class ordered by first frame; a superset prefix when
                                                        // the caller passes a grouped plan's lists without its run counts
          if (p.b_mode) lw += __popcll(__ballot(i < cnt && p.last_depth[l0 + off + i] < d_lo));
        }
      }
      need[cls] = nd;
      lo_[cls] = min(lw, nd);
      off += cnt;
    }
  }
  float *out = p.out + p.ll_off[utt];
  // skip_single: the 32-row pdfs (single- and multi-block) are scored by gmm_bf16_kernel; only the small-slot classes are
  // left for this launch
  if (p.skip_single >= 2) { need[2] = 0; need[3] = 0; need[4] = 0; }   // slots 16 / 8 / 4 went to gmm_split_small_kernel
  if (p.skip_single && need[2] + need[3] + need[4] + need[5] == 0) return;
  if (p.b_skip0) {   // band mode after gmm_band_kernel: single Gaussians are left
    need[1] = 0; need[2] = 0; need[3] = 0; need[4] = 0; lo_[1] = 0; lo_[2] = 0; lo_[3] = 0; lo_[4] = 0;
    if (need[5] - lo_[5] == 0) return;
  }

  Tile<M8, kNT> tile;
  tile.load_b(p, f0, T, t_base, lane);
  f32x16 acc[kNT];
  // Class 0 is one run ordered by first depth, or (grouped plan) `groups` runs — searched and walked one after the other.
  const bool skip0 = p.skip_single || p.b_skip0;
  const int nruns = p.groups > 1 ? p.groups : 1;
  int run_off = 0;
  for (int run = 0; run < nruns; run++) {
  int n_single = skip0 ? 0 : need[0];
  int first32 = lo_[0];         // band mode: the class-0 range starts here (0 otherwise)
  if (p.groups > 1 && !skip0) {
    const int cnt = p.group_counts[(size_t)utt * p.groups + run];
    int nd = cnt, lw = 0;
    if (p.first_frame) {
      int t_last = min(T, t_base + kFramesPerWave) - 1, d_lo = 0;
      if (p.b_mode) { const Band bd = band_of(p, utt); t_last = bd.hi; d_lo = bd.lo; }
      nd = 0;
      for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        nd += __popcll(__ballot(i < cnt && p.first_frame[l0 + run_off + i] <= t_last));
        if (p.b_mode) lw += __popcll(__ballot(i < cnt && p.last_depth[l0 + run_off + i] < d_lo));
      }
    }
    first32 = run_off + min(lw, nd); n_single = run_off + nd;
    run_off += cnt;
  }

  // ---- single-block 32-row pdfs (the bulk of a context-dependent model): one pdf per MFMA block.
  // Software pipeline, no extra registers: as soon as the MFMAs that read operand group a[m] of block j have been issued,
  // the same registers are re-loaded with block j+1's rows, so every load has a whole block period (≈5k cycles of MFMA
  // issue plus the epilogue) to come back from L2 / Infinity Cache.  The packed-row lookups (pdf id → first row) run
  // two and three blocks ahead, so they never sit on the critical path.
  // (Round-1 measurements, tools/mfma_f32_microbench2.hip: operands requested just in time 116 TFLOP/s, one block
  // ahead 143 TFLOP/s.)
  if (n_single > first32) {
    const int last = n_single - 1;
    auto pdf_at = [&](int jj) { return __builtin_amdgcn_readfirstlane(list[min(jj, last)]); };
    auto row_of = [&](int pdf) { return __builtin_amdgcn_readfirstlane(p.row0[pdf]); };
    const float *wl = p.w + (h * 32 + col) * 4;  // this lane's piece inside a block (blocks start at multiples of 32 rows)
    f32x4 a[M8], g[4];
    int r1 = row_of(pdf_at(first32 + 1));
    int pdf2 = pdf_at(first32 + 2);
    {
      const int r0 = row_of(pdf_at(first32));
      // same issue order as inside the loop (gconst rows, then operand groups): the compiler's vmcnt bookkeeping at the
      // loop head is the merge of both paths, and a different order here makes it wait for every outstanding load
      Tile<M8, kNT>::load_gc32(p.gc + r0, h, g);
      __builtin_amdgcn_sched_barrier(0);
      Tile<M8, kNT>::load_a(wl + (size_t)r0 * p.kpad, a);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (int j = first32; j < n_single; j++) {
      {
        f32x16 init;
#pragma unroll
        for (int r = 0; r < 16; r++) init[r] = g[r >> 2][r & 3];
#pragma unroll
        for (int n = 0; n < kNT; n++) acc[n] = init;
      }
      // The lookups are vector loads (the compiler cannot prove the lists are not aliased by `out`), issued first so that
      // they are the oldest entries of the in-order vmcnt queue: reading them back after the MFMA phase then waits for
      // nothing younger.
      const int x_r2 = p.row0[pdf2];
      const int x_pdf3 = list[min(j + 3, last)];
      __builtin_amdgcn_sched_barrier(0);
      const float *wn = wl + (size_t)r1 * p.kpad;
      Tile<M8, kNT>::load_gc32(p.gc + r1, h, g);
#pragma unroll
      for (int m = 0; m < M8; m++) {
#pragma unroll
        for (int cc4 = 0; cc4 < 4; cc4++) {
#pragma unroll
          for (int n = 0; n < kNT; n++)
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][cc4], tile.b[n][4 * m + cc4], acc[n], 0, 0, 0);
        }
        a[m] = *reinterpret_cast<const f32x4 *>(wn + 256 * m);
        __builtin_amdgcn_sched_barrier(0);
      }
      r1 = __builtin_amdgcn_readfirstlane(x_r2);
      pdf2 = __builtin_amdgcn_readfirstlane(x_pdf3);
      float mx[kNT], sum[kNT];
#pragma unroll
      for (int n = 0; n < kNT; n++) {
        float m = reg_max<0, 16>(acc[n]);
        m = fmaxf(m, swap32(m, h));
        float sv = reg_expsum<0, 16>(acc[n], m, m + p.min_log_diff);
        sv += swap32(sv, h);
        mx[n] = m; sum[n] = sv;
      }
      if constexpr (kNT == 2) {
        // both halves hold every tile's (max, sum): half h finishes tile h (one log per lane).
        // Stage [64 frames][32 pdfs] in LDS and flush whole 128-byte row segments: a lane-per-frame store would touch 64
        // different lines per instruction and (measured, round 1) inflate HBM write traffic 11x with partial lines.
        const float v = finish(h ? mx[1] : mx[0], h ? sum[1] : sum[0]);
        const int jj = (j - first32) & 31;
        stage[(32 * h + col) * 33 + jj] = v;
        if (jj == 31 || j == last) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          const int j0 = j - jj, cnt = jj + 1;
          const int c = lane & 31;
#pragma unroll 4
          for (int i = 0; i < 32; i++) {
            const int r = (lane >> 5) + 2 * i, t = t_base + r;
            // streaming store: the scores are written once and read once by the decoder; keeping them out of the
            // Infinity Cache leaves room for the 51 MB of model rows every workgroup keeps re-reading
            if (c < cnt && t < T) __builtin_nontemporal_store(stage[r * 33 + c], &out[(size_t)t * P + j0 + c]);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
      } else {
#pragma unroll
        for (int n = 0; n < kNT; n++) {
          const int t = t_base + 32 * n + col;
          if (h == (n & 1) && t < T) out[(size_t)t * P + j] = finish(mx[n], sum[n]);
        }
      }
    }
  }
  }   // runs of class 0

  // ---- 32-row pdfs with more than 32 Gaussians: several blocks, two passes (max, then the sum against that max)
  const int n32 = cc[0];
  for (int j = cc6[0] + lo_[1]; j < cc6[0] + (p.skip_single ? 0 : need[1]); j++) {
    const int pdf = list[j];
    const int r0 = p.row0[pdf], nb = p.nblk[pdf];
    float mx[kNT], sum[kNT];
#pragma unroll
    for (int n = 0; n < kNT; n++) { mx[n] = -INFINITY; sum[n] = 0.0f; }
    for (int blk = 0; blk < nb; blk++) {
      const int rr = r0 + 32 * blk + col;
      tile.block(row_ptr(p.w, p.kpad, rr, h), p.gc[rr], lane, acc);
#pragma unroll
      for (int n = 0; n < kNT; n++) {
        float m = reg_max<0, 16>(acc[n]);
        m = fmaxf(m, __shfl_xor(m, 32));
        mx[n] = fmaxf(mx[n], m);
      }
    }
    for (int blk = 0; blk < nb; blk++) {
      const int rr = r0 + 32 * blk + col;
      tile.block(row_ptr(p.w, p.kpad, rr, h), p.gc[rr], lane, acc);
#pragma unroll
      for (int n = 0; n < kNT; n++) {
        float sv = reg_expsum<0, 16>(acc[n], mx[n], mx[n] + p.min_log_diff);
        sv += swap32(sv, h);
        sum[n] += sv;
      }
    }
#pragma unroll
    for (int n = 0; n < kNT; n++) {
      const int t = t_base + 32 * n + col;
      if (h == (n & 1) && t < T) out[(size_t)t * P + j] = finish(mx[n], sum[n]);
    }
  }

  // ---- smaller slots: 32/slot pdfs share one MFMA block
  int base = n32;
  // slot 16
  for (int j = lo_[2] & ~1; j < need[2]; j += 2) {
    const int which = col >> 4, within = col & 15;
    const int idx = j + which;
    const int row = idx < cc[1] ? p.row0[list[base + idx]] + within : p.num_rows;
    tile.block(row_ptr(p.w, p.kpad, row, h), p.gc[row], lane, acc);
#pragma unroll
    for (int n = 0; n < kNT; n++) {
      int t = t_base + 32 * n + col;
      float m0 = reg_max<0, 8>(acc[n]), m1 = reg_max<8, 16>(acc[n]);
      m0 = fmaxf(m0, __shfl_xor(m0, 32)); m1 = fmaxf(m1, __shfl_xor(m1, 32));
      float s0 = reg_expsum<0, 8>(acc[n], m0, m0 + p.min_log_diff), s1 = reg_expsum<8, 16>(acc[n], m1, m1 + p.min_log_diff);
      s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32);
      if (h == 0 && t < T) {
        out[(size_t)t * P + base + j] = finish(m0, s0);
        if (j + 1 < cc[1]) out[(size_t)t * P + base + j + 1] = finish(m1, s1);
      }
    }
  }
  base += cc[1];
  // slot 8
  for (int j = lo_[3] & ~3; j < need[3]; j += 4) {
    const int which = col >> 3, within = col & 7;
    const int idx = j + which;
    const int row = idx < cc[2] ? p.row0[list[base + idx]] + within : p.num_rows;
    tile.block(row_ptr(p.w, p.kpad, row, h), p.gc[row], lane, acc);
#pragma unroll
    for (int n = 0; n < kNT; n++) {
      int t = t_base + 32 * n + col;
      float m[4]; float s[4];
      m[0] = reg_max<0, 4>(acc[n]); m[1] = reg_max<4, 8>(acc[n]); m[2] = reg_max<8, 12>(acc[n]); m[3] = reg_max<12, 16>(acc[n]);
#pragma unroll
      for (int q = 0; q < 4; q++) m[q] = fmaxf(m[q], __shfl_xor(m[q], 32));
      s[0] = reg_expsum<0, 4>(acc[n], m[0], m[0] + p.min_log_diff); s[1] = reg_expsum<4, 8>(acc[n], m[1], m[1] + p.min_log_diff);
      s[2] = reg_expsum<8, 12>(acc[n], m[2], m[2] + p.min_log_diff); s[3] = reg_expsum<12, 16>(acc[n], m[3], m[3] + p.min_log_diff);
#pragma unroll
      for (int q = 0; q < 4; q++) s[q] += __shfl_xor(s[q], 32);
      if (h == 0 && t < T) {
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (j + q < cc[2]) out[(size_t)t * P + base + j + q] = finish(m[q], s[q]);
      }
    }
  }
  base += cc[2];
  // slot 4: rows 8q+4h..8q+4h+3 live in registers 4q..4q+3 of one lane → pdf index 2q+h, no shuffle
  for (int j = lo_[4] & ~7; j < need[4]; j += 8) {
    const int which = col >> 2, within = col & 3;
    const int idx = j + which;
    const int row = idx < cc[3] ? p.row0[list[base + idx]] + within : p.num_rows;
    tile.block(row_ptr(p.w, p.kpad, row, h), p.gc[row], lane, acc);
#pragma unroll
    for (int n = 0; n < kNT; n++) {
      int t = t_base + 32 * n + col;
      float m[4]; float s[4];
      m[0] = reg_max<0, 4>(acc[n]); m[1] = reg_max<4, 8>(acc[n]); m[2] = reg_max<8, 12>(acc[n]); m[3] = reg_max<12, 16>(acc[n]);
      s[0] = reg_expsum<0, 4>(acc[n], m[0], m[0] + p.min_log_diff); s[1] = reg_expsum<4, 8>(acc[n], m[1], m[1] + p.min_log_diff);
      s[2] = reg_expsum<8, 12>(acc[n], m[2], m[2] + p.min_log_diff); s[3] = reg_expsum<12, 16>(acc[n], m[3], m[3] + p.min_log_diff);
      if (t < T) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          int pi = j + 2 * q + h;
          if (pi < cc[3]) out[(size_t)t * P + base + pi] = finish(m[q], s[q]);
        }
      }
    }
  }
  base += cc[3];
  // slot 1: every row is its own single-Gaussian pdf: LL = ll (max + log(1) exactly)
  for (int j = lo_[5] & ~31; j < need[5]; j += 32) {
    const int idx = j + col;
    const int row = idx < cc[4] ? p.row0[list[base + idx]] : p.num_rows;
    tile.block(row_ptr(p.w, p.kpad, row, h), p.gc[row], lane, acc);
#pragma unroll
    for (int n = 0; n < kNT; n++) {
      int t = t_base + 32 * n + col;
      if (t < T) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          int pi = j + acc_row(r, h);
          if (pi < cc[4]) out[(size_t)t * P + base + pi] = acc[n][r];
        }
      }
    }
  }
  if (p.trace && lane == 0) {
    unsigned long long *rec = p.trace + (size_t)rec_index * 4;
    rec[0] = t_start; rec[1] = wall_clock64();
    rec[2] = ((unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11))) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (3 << 11)) << 32);
    rec[3] = (unsigned long long)(need[0] + need[1]);
  }
}

// Persistent scoring kernel.  Round-1 timeline of the one-workgroup-per-tile version (tools/gmm_timeline.py): the hardware
// deals workgroups to CUs in a fixed round-robin order — every CU received exactly 32 of the 8192 workgroups and, the
// tile index being periodic in the grid, always the SAME tile type — so CUs with cheap tiles idled (slot occupancy 82 %)
// and skipping unreachable cells bought no time at all.  Here the grid is just enough workgroups to fill the chip
// (2 per CU) and work is pulled from queues (atomic counters) until they run dry, in two phases:
//   phase 1, workgroup items (utterance, 256-frame tile) for the tiles whose four 64-frame sub-tiles all need the whole
//     pdf list: the four wavefronts take one sub-tile each and walk the list at the same pace, so the model rows they
//     stream come through the CU's L1 once, not four times (measured: 5.3 µs per 32-row block against 5.9 µs when every
//     wavefront streams its own rows);
//   phase 2, wavefront items (utterance, 64-frame tile) for the leading tiles, where reachability makes the sub-tiles
//     unequal (a workgroup item would idle three wavefronts behind the fourth); being short, they also fill the tail.
// One queue per XCD and phase, holding the utterances u ≡ xcd (mod 8): all tiles of an utterance stream the same rows
// through that XCD's private L2 (cdna_hip_programming.md T1); the XCD a workgroup runs on is read from XCC_ID.  Items go
// utterance by utterance, last frames first.  A workgroup whose queue is empty takes items from the other XCDs' queues,
// so a phase ends within one item.  Every wavefront leaves a loop once all eight counters have passed their item counts:
// the grid always drains.
template <int M8, int kNT, int kMinWaves, int kWaves>
__global__ __launch_bounds__(64 * kWaves, kMinWaves) void gmm_kernel(GmmParams p) {
  constexpr int kFramesPerWave = 32 * kNT, kFramesPerTile = kFramesPerWave * kWaves;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // per-wavefront output staging tile (written lane-per-frame, read row-wise by the same wavefront)
  __shared__ float stage_all[kWaves][64 * 33];
  __shared__ int s_item;
  const int my_xcd = (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u);
  // leading tiles whose first sub-tile cannot yet see every pdf (first possible frame beyond that sub-tile's last frame)
  int light = 0;
  if (p.first_frame) {
    const int mff = __builtin_amdgcn_readfirstlane(*p.max_ff);
    light = mff >= kFramesPerWave ? min(p.tiles, (mff - (kFramesPerWave - 1) + kFramesPerTile - 1) / kFramesPerTile) : 0;
  }
  const int heavy = p.tiles - light;
  // Opaque copies inside the loops: without them the compiler hoists every lane-dependent address out of the item loop
  // and keeps it in registers for the kernel's lifetime (measured: 256 VGPRs + 240 bytes of scratch instead of 217 VGPRs).
  if (heavy > 0) {
    for (int hop = 0; hop < 8; hop++) {
      const int q = (my_xcd + hop) & 7;
      const int n_items = ((p.n_utt - q + 7) >> 3) * heavy;   // utterances q, q+8, q+16, ...
      for (;;) {
        __syncthreads();                             // every wavefront is done with the previous item (and has read s_item)
        if (threadIdx.x == 0) s_item = atomicAdd(&p.queue[q], 1);
        __syncthreads();
        const int item = s_item;
        if (item >= n_items) break;                  // uniform over the workgroup
        int lane_i = lane, wave_i = wave;
        asm volatile("" : "+v"(lane_i), "+v"(wave_i));
        wave_i = __builtin_amdgcn_readfirstlane(wave_i);
        const int v = item / heavy, tl = p.tiles - 1 - item % heavy;
        score_tile<M8, kNT>(p, v * 8 + q, (tl * kWaves + wave_i) * kFramesPerWave, lane_i, stage_all[wave_i],
                            ((v * 8 + q) * p.tiles + tl) * kWaves + wave_i);
      }
    }
  }
  if (light > 0) {
    const int per_utt = light * kWaves;
    for (int hop = 0; hop < 8; hop++) {
      const int q = (my_xcd + hop) & 7;
      const int n_items = ((p.n_utt - q + 7) >> 3) * per_utt;
      for (;;) {
        int item = 0;
        if (lane == 0) item = atomicAdd(&p.queue[8 + q], 1);
        item = __builtin_amdgcn_readfirstlane(item);
        if (item >= n_items) break;                  // uniform over the wavefront
        int lane_i = lane, wave_i = wave;
        asm volatile("" : "+v"(lane_i), "+v"(wave_i));
        wave_i = __builtin_amdgcn_readfirstlane(wave_i);
        const int v = item / per_utt, r = per_utt - 1 - item % per_utt;
        score_tile<M8, kNT>(p, v * 8 + q, r * kFramesPerWave, lane_i, stage_all[wave_i], (v * 8 + q) * p.tiles * kWaves + r);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// bf16×3 scoring of the single-block 32-row pdfs on v_mfma_f32_32x32x16_bf16 (the default for that slot class;
// MFA_GMM_BF16=0 sends it back to the bit-exact f32 kernel).
// A float32 value is the exact sum of three bf16 pieces (8 + 8 + 8 mantissa bits), x = x1 + x2 + x3, and a product of two
// bf16 values is exact in float32, so   x·w ≈ x1w1 + (x1w2 + x2w1) + (x1w3 + x2w2 + x3w1)   with a relative error of
// ≈2^-24 per term — the error of ONE float32 rounding (tools/mfma_bf16_layout_test.hip: 5.0e-8 of Σ|terms| against
// float64).  Six bf16 MFMAs of 32 cycles cover 16 k-values that cost eight f32 MFMAs of 64 cycles: 2.7× the f32 rate.
// What changes is the order of the accumulation, so scores agree with the fmaf-chain oracle to float32 rounding noise
// (≲2e-4 absolute on |score| ≈ 100; north_star's bar is 1e-3), not bit for bit like the f32 path.
//
// At this MFMA rate a wavefront cannot stream its own copy of the model rows (4× the L1/L2 traffic of the f32 kernel per
// unit time), so the kernel is organised like a GEMM: the workgroup's four wavefronts (64 frames each, x̃ split once into
// registers: 120 VGPRs) share every 32-row block through LDS, double-buffered — while block j is multiplied out of one
// buffer, block j+1 travels global → registers → the other buffer; one barrier per block.
// General form (models that contain multi-block pdfs); gmm_split_single_kernel below is the lean form for single-block pdfs.

// One 32-row model block (split operands in LDS: [step][piece][half][row] 16-byte units; its 32 gconsts) times a
// wavefront's two frame tiles → acc.  Operand pieces of step s+1 are read from LDS while step s is multiplied; six (three)
// products per 16 k-values, smallest terms first; the two tiles alternate so that consecutive MFMAs never wait on each
// other's accumulator; the gconsts enter as the first MFMA's addend.
template <int kSteps, int kPieces, typename Op8>
__device__ __forceinline__ void multiply_block(const uint4 *a_blk, const float *gc_blk, const Op8 (&b)[2][kSteps][kPieces],
                                               f32x16 (&acc)[2], int col, int h) {
  constexpr bool kHalf = kPieces == 2;
  f32x16 init;
#pragma unroll
  for (int qq = 0; qq < 4; qq++) {
    const float4 gq = *reinterpret_cast<const float4 *>(&gc_blk[8 * qq + 4 * h]);
    init[4 * qq] = gq.x; init[4 * qq + 1] = gq.y; init[4 * qq + 2] = gq.z; init[4 * qq + 3] = gq.w;
  }
  auto read_a = [&](int s, Op8 (&a)[kPieces]) {
#pragma unroll
    for (int qq = 0; qq < kPieces; qq++) a[qq] = __builtin_bit_cast(Op8, a_blk[((s * kPieces + qq) * 2 + h) * 32 + col]);
  };
  Op8 a_cur[kPieces], a_nxt[kPieces];
  read_a(0, a_cur);
  constexpr int kProd = kHalf ? 3 : 6;
  constexpr int pa[6] = {kHalf ? 1 : 2, kHalf ? 0 : 1, 0, 1, 0, 0}, pb[6] = {0, 1, kHalf ? 0 : 2, 0, 1, 0};
#pragma unroll
  for (int s = 0; s < kSteps; s++) {
    if (s + 1 < kSteps) read_a(s + 1, a_nxt);
#pragma unroll
    for (int t6 = 0; t6 < kProd; t6++)
#pragma unroll
      for (int n = 0; n < 2; n++) {
        const f32x16 &cin = (s == 0 && t6 == 0) ? init : acc[n];
        if constexpr (kHalf) acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_cur[pa[t6]], b[n][s][pb[t6]], cin, 0, 0, 0);
        else acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[pa[t6]], b[n][s][pb[t6]], cin, 0, 0, 0);
      }
#pragma unroll
    for (int qq = 0; qq < kPieces; qq++) a_cur[qq] = a_nxt[qq];
  }
}

// kPieces = 3: bf16 triples; kPieces = 2: scaled f16 pairs with the per-tile range fallback (see gmm_split_single_kernel).
template <int kSteps, int kPieces>   // 16-k steps per row: 5 for D ≤ 40, 6 for D ≤ 48
__global__ __launch_bounds__(256, 2) void gmm_bf16_kernel(GmmParams p) {
  constexpr bool kMulti = true;
  constexpr bool kHalf = kPieces == 2;
  using op8 = std::conditional_t<kHalf, f16x8, bf16x8>;
  constexpr int kNT = 2, kWaves = 4, kFramesPerWave = 64, kFramesPerTile = 256;
  constexpr int kUnits = kSteps * kPieces * 2 * 32;    // 16-byte units per block
  constexpr int kLoads = (kUnits + 255) / 256;         // units each thread moves per block
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float stage_all[kWaves][64 * 33];
  __shared__ uint4 a_lds[2][kUnits];
  __shared__ __attribute__((aligned(16))) float gc_lds[2][32];
  // Entry table of the item, staged in chunks (two dependent global loads per pdf must not sit in the block loop).  An
  // entry is one 32-row block: a single-block pdf is one entry; a pdf with more than 32 Gaussians is a run of entries
  // whose (max, sum) pairs are merged on the fly (online log-sum-exp) and emitted with its last block.
  constexpr int kBlkCache = 1024;
  constexpr int kFirst = 1 << 30, kLast = 1 << 31;
  __shared__ int blk_lds[kBlkCache];                  // 32-row block index
  __shared__ int col_lds[kBlkCache];                  // output column | kFirst | kLast
  __shared__ int s_item;
  float *stage = stage_all[wave];
  if (!kHalf && p.redo_mode == 2 && *p.redo_count == 0) return;   // uniform: the f16 pass declined nothing
  const int my_xcd = (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u);
  for (int hop = 0; hop < 8; hop++) {
    const int q = (my_xcd + hop) & 7;
    const int n_items = ((p.n_utt - q + 7) >> 3) * p.tiles;
    for (;;) {
      __syncthreads();
      if (threadIdx.x == 0) s_item = atomicAdd(&p.queue[q], 1);
      __syncthreads();
      const int item = s_item;
      if (item >= n_items) break;
      int lane = lane0;                                // opaque per item: keeps lane-dependent addresses out of long-lived registers
      asm volatile("" : "+v"(lane));
      const int col = lane & 31, h = lane >> 5;
      const int utt = (item / p.tiles) * 8 + q, tl = p.tiles - 1 - item % p.tiles;
      const int64_t f0 = p.frame_off[utt];
      const int T = (int)(p.frame_off[utt + 1] - f0);
      if (tl * kFramesPerTile >= T) continue;          // uniform over the workgroup
      if (!kHalf && p.redo_mode == 2 && p.redo[(size_t)utt * p.tiles + tl] == 0) continue;   // only what the f16 pass left
      const int t_base = (tl * kWaves + wave) * kFramesPerWave;
      const bool active = t_base < T;                  // a wavefront past the end still helps move blocks and joins barriers
      const int64_t l0 = p.pdf_off[utt];
      const int P = (int)(p.pdf_off[utt + 1] - l0);
      const int32_t *list = p.pdf_list + l0;
      const int cc0 = p.class_counts[(size_t)utt * 6], cc1 = kMulti ? p.class_counts[(size_t)utt * 6 + 1] : 0;
      // n0 / n1: single-block / multi-block pdfs the tile's LAST frame can be asked for — the prefixes the workgroup walks
      // together (block copies and barriers are collective).  n0_mine / n1_mine: the shorter prefixes this wavefront's own
      // 64 frames can be asked for; beyond them the wavefront only helps with the copies.
      int n0 = cc0, n1 = cc1, n0_mine = cc0, n1_mine = cc1;
      if (p.first_frame) {
        const int t_last = min(T, (tl + 1) * kFramesPerTile) - 1;
        const int t_mine = min(T, t_base + kFramesPerWave) - 1;
        n0 = n1 = n0_mine = n1_mine = 0;
        for (int i0 = 0; i0 < cc0 + cc1; i0 += 64) {
          const int i = i0 + lane;
          const int ff = i < cc0 + cc1 ? p.first_frame[l0 + i] : 0x7fffffff;
          const unsigned long long all = __ballot(ff <= t_last), mine = __ballot(ff <= t_mine);
          const unsigned long long c0m = __ballot(i < cc0);
          // class 0: the prefix up to the LAST pdf that can be asked for (= the count when the class is ordered by first
          // frame; a superset of what is needed when a grouped plan lays it out in several ordered runs)
          n0 = max(n0, prefix_end(all & c0m, i0)); n1 += __popcll(all & ~c0m);
          n0_mine = max(n0_mine, prefix_end(mine & c0m, i0)); n1_mine += __popcll(mine & ~c0m);
        }
      }
      if (p.skip_cc0) { n0 = 0; n0_mine = 0; }         // columns keep their places: multi-block pdfs start at column cc0
      // total entries: one per single-block pdf, nblk per multi-block pdf
      int e_multi = 0;
      for (int i0 = 0; i0 < n1; i0 += 64) {
        const int i = i0 + lane;
        int nb = i < n1 ? p.nblk[list[cc0 + i]] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o);
        e_multi += nb;
      }
      const int n_entries = n0 + e_multi;
      float *out = p.out + p.ll_off[utt];
      if (n_entries > 0) {
        // ---- x̃ = [x, x²] of this wavefront's 64 frames, split into bf16 triples: b[tile][step][piece], lane (frame, half)
        op8 b[kNT][kSteps][kPieces];
        // kHalf: `bad` = a scaled feature outside the f16 range (or NaN)
        const bool bad = split_features<kSteps, kPieces>(p, f0, T, t_base, col, h, b);
        if constexpr (kHalf) {
          if (__syncthreads_or(bad)) {                     // uniform: the whole tile goes to the bf16×3 pass
            if (threadIdx.x == 0) { p.redo[(size_t)utt * p.tiles + tl] = 1; atomicAdd(p.redo_count, 1); }
            continue;
          }
        }
        const uint4 *wsrc = kHalf ? p.wh : p.wb;
        const float *gsrc = kHalf ? p.gch : p.gc;
        const float inv_s = kHalf ? p.acc_scale_inv : 1.0f;
        const float l2e_s = 1.44269504088896341f * inv_s;  // inv_s is a power of two: scaling commutes with the rounding
        // Block copy global → registers (requested before block j is multiplied) → LDS (written after it).  The LDS-DMA form
        // (global_load_lds) measured the same when it overlapped and much worse when it did not: the compiler cannot tell the
        // two LDS buffers apart and drains vmcnt before every LDS read while a DMA write is in flight.
        uint4 mv[kLoads];
        float4 gmv = make_float4(0.f, 0.f, 0.f, 0.f);
        auto fetch = [&](int blk) {
          const uint4 *src = wsrc + (size_t)blk * kUnits;
#pragma unroll
          for (int i = 0; i < kLoads; i++) {
            const int u = threadIdx.x + 256 * i;
            mv[i] = u < kUnits ? src[u] : make_uint4(0, 0, 0, 0);
          }
          if (threadIdx.x < 8) gmv = *reinterpret_cast<const float4 *>(gsrc + (size_t)blk * 32 + 4 * threadIdx.x);
        };
        auto deposit = [&](int buf) {
#pragma unroll
          for (int i = 0; i < kLoads; i++) {
            const int u = threadIdx.x + 256 * i;
            if (u < kUnits) a_lds[buf][u] = mv[i];
          }
          if (threadIdx.x < 8) *reinterpret_cast<float4 *>(&gc_lds[buf][4 * threadIdx.x]) = gmv;
        };
        int multi_pdf = 0, multi_blk = 0;                  // thread 0's cursor into the multi-block pdfs
        int staged = 0, stage_col0 = 0;                    // columns waiting in the staging tile: stage_col0 .. +staged-1
        float mx_run[kNT], sum_run[kNT];
#pragma unroll
        for (int n = 0; n < kNT; n++) { mx_run[n] = -INFINITY; sum_run[n] = 0.0f; }
        auto flush = [&]() {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
          for (int i = 0; i < 32; i++) {
            const int r = h + 2 * i, t = t_base + r;
            if (col < staged && t < T) __builtin_nontemporal_store(stage[r * 33 + col], &out[(size_t)t * P + stage_col0 + col]);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          staged = 0;
        };
        for (int c0 = 0; c0 < n_entries; c0 += kBlkCache) {
        const int c1 = min(n_entries, c0 + kBlkCache);
        __syncthreads();                                   // previous chunk's table is no longer read
        for (int i = c0 + threadIdx.x; i < min(c1, n0); i += 256) {
          blk_lds[i - c0] = p.row0[list[i]] >> 5;
          if (kMulti) col_lds[i - c0] = i | kFirst | kLast;
        }
        if (kMulti && threadIdx.x == 0) {
          for (int e = max(c0, n0); e < c1; e++) {
            const int pdf = list[cc0 + multi_pdf], nb = p.nblk[pdf];
            blk_lds[e - c0] = (p.row0[pdf] >> 5) + multi_blk;
            col_lds[e - c0] = (cc0 + multi_pdf) | (multi_blk == 0 ? kFirst : 0) | (multi_blk == nb - 1 ? kLast : 0);
            if (++multi_blk == nb) { multi_blk = 0; multi_pdf++; }
          }
        }
        __syncthreads();
        auto block_of = [&](int jj) { return blk_lds[min(jj, c1 - 1) - c0]; };
        fetch(block_of(c0));
        deposit(0);
        __syncthreads();
        for (int j = c0; j < c1; j++) {
          const int buf = (j - c0) & 1;
          fetch(block_of(j + 1));                          // block j+1 (the chunk's last trip re-fetches its last block: harmless)
          const int ecol = kMulti ? col_lds[j - c0] : (j | kFirst | kLast);
          const int out_col = ecol & ~(kFirst | kLast);
          const bool mine = out_col < cc0 ? out_col < n0_mine : out_col - cc0 < n1_mine;
          if (active && mine) {
            f32x16 acc[kNT];
            multiply_block<kSteps, kPieces>(a_lds[buf], gc_lds[buf], b, acc, col, h);
            // ---- log-sum-exp epilogue and LDS-staged, coalesced score stores: as in score_tile
            float mx[kNT], sum[kNT];
#pragma unroll
            for (int n = 0; n < kNT; n++) {
              float m = reg_max<0, 16>(acc[n]);
              m = fmaxf(m, swap32(m, h));
              float sv = reg_expsum_fast(acc[n], m, l2e_s);
              sv += swap32(sv, h);
              mx[n] = m; sum[n] = sv;                        // mx stays in accumulator units (× S) until the pdf's last block
            }
            if (kMulti && !(ecol & kFirst)) {
              // online log-sum-exp: fold this block's (max, sum) into the pdf's running pair
#pragma unroll
              for (int n = 0; n < kNT; n++) {
                const float M = fmaxf(mx_run[n], mx[n]);
                sum[n] = sum_run[n] * __builtin_amdgcn_exp2f((mx_run[n] - M) * l2e_s) +
                         sum[n] * __builtin_amdgcn_exp2f((mx[n] - M) * l2e_s);
                mx[n] = M;
              }
            }
            if (kMulti) {
#pragma unroll
              for (int n = 0; n < kNT; n++) { mx_run[n] = mx[n]; sum_run[n] = sum[n]; }
            }
            if (ecol & kLast) {
              const float v = finish((h ? mx[1] : mx[0]) * inv_s, h ? sum[1] : sum[0]);
              if (staged > 0 && out_col != stage_col0 + staged) flush();   // a jump in the column sequence (class change)
              if (staged == 0) stage_col0 = out_col;
              stage[(32 * h + col) * 33 + staged] = v;
              if (++staged == 32) flush();
            }
          }
          deposit(buf ^ 1);
          __syncthreads();                               // block j+1 is in place; everybody is done with block j
        }
        }
        if (staged > 0) flush();
      }
    }
  }
}

// Lean instantiation for models WITHOUT multi-block pdfs (the headline configuration): every entry is a whole pdf, so there
// is no entry table beyond the block indices, no merge state, fixed 32-column staging phases, and the block copies go
// global → LDS directly (global_load_lds_dwordx4; here the compiler lets them overlap).  3 % faster than the general kernel
// on configs[2]; same arithmetic, same results.
//
// kPieces = 3: operands are bf16 triples, six products per 16 k-values (2^-24 per term, any exponent range).
// kPieces = 2: operands are f16 pairs, three products (a2·b1, a1·b2, a1·b1: 3·2^-22 per term worst case, half the matrix
//   work).  f16 has 5 exponent bits, so the operands are scaled by powers of two chosen from the model at load time
//   (mfa_load_gmm: weight column k × 2^e_k, feature column k × S·2^-e_k, accumulators therefore × S; all exact) and a tile
//   whose scaled features leave the f16 range is not scored here: it is flagged in p.redo and scored by the kPieces = 3
//   kernel, launched next with redo_mode 2.
template <int kSteps, int kPieces>   // 16-k steps per row: 5 for D ≤ 40, 6 for D ≤ 48
__global__ __launch_bounds__(256, 2) void gmm_split_single_kernel(GmmParams p) {
  constexpr int kNT = 2, kWaves = 4, kFramesPerWave = 64, kFramesPerTile = 256;
  constexpr bool kHalf = kPieces == 2;
  using op8 = std::conditional_t<kHalf, f16x8, bf16x8>;
  constexpr int kUnits = kSteps * kPieces * 2 * 32;    // 16-byte units per block
  constexpr int kLoads = (kUnits + 255) / 256;         // units each thread moves per block
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float stage_all[kWaves][64 * 33];
  __shared__ uint4 a_lds[2][kUnits];
  __shared__ __attribute__((aligned(16))) float gc_lds[2][32];
  constexpr int kBlkCache = 1024;                     // pdf → 32-row block index, staged per item (two dependent global
  __shared__ int blk_lds[kBlkCache];                  // loads per pdf must not sit in the block loop)
  __shared__ int s_item;
  float *stage = stage_all[wave];
  if (!kHalf && p.redo_mode == 2 && *p.redo_count == 0) return;   // uniform: the f16 pass declined nothing
  const int my_xcd = (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u);
  for (int hop = 0; hop < 8; hop++) {
    const int q = (my_xcd + hop) & 7;
    const int n_items = ((p.n_utt - q + 7) >> 3) * p.tiles;
    for (;;) {
      __syncthreads();
      if (threadIdx.x == 0) s_item = atomicAdd(&p.queue[q], 1);
      __syncthreads();
      const int item = s_item;
      if (item >= n_items) break;
      int lane = lane0;                                // opaque per item: keeps lane-dependent addresses out of long-lived registers
      asm volatile("" : "+v"(lane));
      const int col = lane & 31, h = lane >> 5;
      const int utt = (item / p.tiles) * 8 + q, tl = p.tiles - 1 - item % p.tiles;
      const int64_t f0 = p.frame_off[utt];
      const int T = (int)(p.frame_off[utt + 1] - f0);
      if (tl * kFramesPerTile >= T) continue;          // uniform over the workgroup
      if (!kHalf && p.redo_mode == 2 && p.redo[(size_t)utt * p.tiles + tl] == 0) continue;   // only what the f16 pass left
      const int t_base = (tl * kWaves + wave) * kFramesPerWave;
      const bool active = t_base < T;                  // a wavefront past the end still helps move blocks and joins barriers
      const int64_t l0 = p.pdf_off[utt];
      const int P = (int)(p.pdf_off[utt + 1] - l0);
      const int32_t *list = p.pdf_list + l0;
      const int n_all = p.class_counts[(size_t)utt * 6];
      // n_single: pdfs the tile's LAST frame can be asked for — the prefix the workgroup walks together (block copies and
      // barriers are collective).  n_mine: the shorter prefix this wavefront's own 64 frames can be asked for; beyond it
      // the wavefront only helps with the copies.
      int n_single = n_all, n_mine = n_all;
      if (p.first_frame) {
        const int t_last = min(T, (tl + 1) * kFramesPerTile) - 1;
        const int t_mine = min(T, t_base + kFramesPerWave) - 1;
        n_single = 0; n_mine = 0;
        for (int i0 = 0; i0 < n_all; i0 += 64) {
          const int i = i0 + lane;
          const int ff = i < n_all ? p.first_frame[l0 + i] : 0x7fffffff;
          n_single = max(n_single, prefix_end(__ballot(ff <= t_last), i0));   // (see gmm_bf16_kernel: superset for grouped plans)
          n_mine = max(n_mine, prefix_end(__ballot(ff <= t_mine), i0));
        }
      }
      float *out = p.out + p.ll_off[utt];
      if (n_single > 0) {
        // ---- x̃ = [x, x²] of this wavefront's 64 frames, split into bf16 triples: b[tile][step][piece], lane (frame, half)
        op8 b[kNT][kSteps][kPieces];
        // kHalf: `bad` = a scaled feature outside the f16 range (or NaN)
        const bool bad = split_features<kSteps, kPieces>(p, f0, T, t_base, col, h, b);
        if constexpr (kHalf) {
          if (__syncthreads_or(bad)) {                     // uniform: the whole tile goes to the bf16×3 pass
            if (threadIdx.x == 0) { p.redo[(size_t)utt * p.tiles + tl] = 1; atomicAdd(p.redo_count, 1); }
            continue;
          }
        }
        const uint4 *wsrc = kHalf ? p.wh : p.wb;
        const float *gsrc = kHalf ? p.gch : p.gc;
        const float inv_s = kHalf ? p.acc_scale_inv : 1.0f;
        const float l2e_s = 1.44269504088896341f * inv_s;  // inv_s is a power of two: (x·inv_s)·log2e == x·(log2e·inv_s)
        // Block copy global → LDS without a register stop (global_load_lds_dwordx4: every lane's 16 bytes land at a
        // wavefront-uniform LDS base + 16·lane, which is exactly the linear unit order of a block).
        typedef __attribute__((address_space(1))) const void *gptr_t;
        typedef __attribute__((address_space(3))) void *lptr_t;
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        auto fetch = [&](int blk, int buf) {
          const uint4 *src = wsrc + (size_t)blk * kUnits;
#pragma unroll
          for (int i = 0; i < kLoads; i++) {
            const int u0 = 64 * wave_u + 256 * i;        // first unit this wavefront moves in round i (uniform)
            if (u0 < kUnits)
              __builtin_amdgcn_global_load_lds((gptr_t)(src + u0 + lane), (lptr_t)&a_lds[buf][u0], 16, 0, 0);
          }
          if (wave_u == 0 && lane < 8)
            __builtin_amdgcn_global_load_lds((gptr_t)(gsrc + (size_t)blk * 32 + 4 * lane), (lptr_t)&gc_lds[buf][0], 16, 0, 0);
        };
        auto landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
        // ---- block loop, software-pipelined inside the wavefront.  An 8-pass MFMA holds the matrix pipe for 32 cycles but the
        // issue port for 4; a wavefront that issues its MFMAs back to back and its log-sum-exp afterwards leaves one of the
        // two idle in turn, and the two wavefronts of a SIMD fall into step (whoever leads is slowed by sharing, whoever lags
        // runs alone and catches up), so nothing overlaps.  Here the epilogue of block j-1 is cut into ≤ 7-instruction
        // chunks and one chunk follows each MFMA of block j in program order (sched_barrier pins it): every stretch of the
        // instruction stream keeps both the matrix pipe and the VALU busy.  Two accumulator sets alternate by block parity.
        f32x16 acc2[2][kNT];
#pragma unroll
        for (int q2 = 0; q2 < 2; q2++)
#pragma unroll
          for (int n = 0; n < kNT; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc2[q2][n][r] = 0.0f;
        float mxv[kNT] = {0.0f, 0.0f}, smv[kNT] = {1.0f, 1.0f}, tm[8];
        f32x2 ex[8];
        constexpr int kChunks = 27;
        // chunk c of the epilogue of the block held in pv; results are bit-identical to reg_max / reg_expsum_fast / finish
        auto epi = [&](int c, const f32x16 (&pv)[kNT], int column) {
          const int n = (c < 3 || (c >= 6 && c < 16)) ? 0 : 1;           // tile the chunk works on
          if (c == 0 || c == 3) {
#pragma unroll
            for (int r = 0; r < 8; r++) tm[r] = fmaxf(pv[n][r], pv[n][r + 8]);
          } else if (c == 1 || c == 4) {
#pragma unroll
            for (int r = 0; r < 4; r++) tm[r] = fmaxf(tm[r], tm[r + 4]);
            tm[0] = fmaxf(tm[0], tm[2]); tm[1] = fmaxf(tm[1], tm[3]);
            tm[0] = fmaxf(tm[0], tm[1]);
          } else if (c == 2 || c == 5) {
            mxv[n] = fmaxf(tm[0], swap32(tm[0], h));
          } else if ((c >= 6 && c < 14) || (c >= 16 && c < 24)) {
            const int g = c < 14 ? c - 6 : c - 16;
            const f32x2 x = {pv[n][2 * g], pv[n][2 * g + 1]};
            const f32x2 mv2 = {mxv[n], mxv[n]};
            const f32x2 lv = {l2e_s, l2e_s};
            const f32x2 arg = (x - mv2) * lv;
            ex[g].x = __builtin_amdgcn_exp2f(arg.x);
            ex[g].y = __builtin_amdgcn_exp2f(arg.y);
          } else if (c == 14 || c == 24) {
#pragma unroll
            for (int w = 1; w < 8; w <<= 1)
#pragma unroll
              for (int r = 0; r + w < 8; r += 2 * w) ex[r] += ex[r + w];
          } else if (c == 15 || c == 25) {
            const float sv = ex[0].x + ex[0].y;
            smv[n] = sv + swap32(sv, h);
          } else if (c == 26) {
            stage[(32 * h + col) * 33 + column] = finish((h ? mxv[1] : mxv[0]) * inv_s, h ? smv[1] : smv[0]);
          }
        };
        auto flush = [&](int jdone) {                        // columns [jdone − jdone%32, jdone] of the staged scores → HBM
          const int jj = jdone & 31;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          const int j0 = jdone - jj, cnt = jj + 1;
#pragma unroll 4
          for (int i = 0; i < 32; i++) {
            const int r = h + 2 * i, t = t_base + r;
            if (col < cnt && t < T) __builtin_nontemporal_store(stage[r * 33 + col], &out[(size_t)t * P + j0 + col]);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        };
        for (int c0 = 0; c0 < n_single; c0 += kBlkCache) {
        const int c1 = min(n_single, c0 + kBlkCache);
        __syncthreads();                                   // previous chunk's table is no longer read
        for (int i = c0 + threadIdx.x; i < c1; i += 256) blk_lds[i - c0] = p.row0[list[i]] >> 5;
        __syncthreads();
        auto block_of = [&](int jj) { return blk_lds[min(jj, c1 - 1) - c0]; };
        fetch(block_of(c0), 0);
        landed();
        __syncthreads();
        // one trip: block j (parity par: c0 is even, so par is also the LDS buffer) is multiplied into acc2[par] while the
        // epilogue of block j-1 runs out of acc2[par ^ 1]
        auto trip = [&](auto par_c, int j) {
          constexpr int par = decltype(par_c)::value;
          constexpr int buf = par;
          // A full window of 32 staged columns (its last one, block j-2's, was written during the previous trip) goes to
          // HBM at the START of a trip: stores share vmcnt with the block copy, and this way they have a whole trip to be
          // acknowledged before landed() waits on the counter — issued at the end of a trip they were waited for at once.
          if (active && j < n_mine && j > 1 && ((j - 2) & 31) == 31) flush(j - 2);
          fetch(block_of(j + 1), buf ^ 1);                 // block j+1 (the chunk's last trip re-fetches its last block: harmless)
          if (active && j < n_mine) {
            f32x16 (&cur)[kNT] = acc2[par];
            const f32x16 (&prev)[kNT] = acc2[par ^ 1];
            f32x16 init;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
              const float4 gq = *reinterpret_cast<const float4 *>(&gc_lds[buf][8 * qq + 4 * h]);
              init[4 * qq] = gq.x; init[4 * qq + 1] = gq.y; init[4 * qq + 2] = gq.z; init[4 * qq + 3] = gq.w;
            }
            const int column = j == 0 ? 32 : ((j - 1) & 31); // the first block of an item has no predecessor: padding column
            // operand pieces of step s+1 are read from LDS while step s is multiplied
            auto read_a = [&](int s, op8 (&a)[kPieces]) {
#pragma unroll
              for (int qq = 0; qq < kPieces; qq++)
                a[qq] = __builtin_bit_cast(op8, a_lds[buf][((s * kPieces + qq) * 2 + h) * 32 + col]);
            };
            op8 a_cur[kPieces], a_nxt[kPieces];
            read_a(0, a_cur);
            // six (three) products per 16 k-values, smallest terms first; the two tiles alternate so that consecutive MFMAs
            // never wait on each other's accumulator
            constexpr int kProd = kHalf ? 3 : 6;
            constexpr int kStride = (kSteps * kProd * kNT) / 30;   // MFMA slots per epilogue chunk
            constexpr int pa[6] = {kHalf ? 1 : 2, kHalf ? 0 : 1, 0, 1, 0, 0}, pb[6] = {0, 1, kHalf ? 0 : 2, 0, 1, 0};
#pragma unroll
            for (int s = 0; s < kSteps; s++) {
              if (s + 1 < kSteps) read_a(s + 1, a_nxt);
#pragma unroll
              for (int t6 = 0; t6 < kProd; t6++)
#pragma unroll
                for (int n = 0; n < kNT; n++) {
                  const f32x16 &cin = (s == 0 && t6 == 0) ? init : cur[n];
                  if constexpr (kHalf)
                    cur[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_cur[pa[t6]], b[n][s][pb[t6]], cin, 0, 0, 0);
                  else
                    cur[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[pa[t6]], b[n][s][pb[t6]], cin, 0, 0, 0);
                  const int slot = (s * kProd + t6) * kNT + n;
                  if (slot % kStride == 0 && slot / kStride < kChunks) epi(slot / kStride, prev, column);
                  __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
              for (int qq = 0; qq < kPieces; qq++) a_cur[qq] = a_nxt[qq];
            }
          }
          landed();
          __syncthreads();                                 // block j+1 is in place; everybody is done with block j
        };
        for (int j = c0; j < c1; j += 2) {
          trip(std::integral_constant<int, 0>{}, j);
          if (j + 1 < c1) trip(std::integral_constant<int, 1>{}, j + 1);
        }
        }
        if (active && n_mine > 0) {                          // drain: the last block's epilogue and the open columns
          const int jp = n_mine - 1;
          if (jp > 0 && ((jp - 1) & 31) == 31) flush(jp - 1);   // a window completed by the last trip is still staged
          if (jp & 1) {
#pragma unroll
            for (int c = 0; c < kChunks; c++) epi(c, acc2[1], jp & 31);
          } else {
#pragma unroll
            for (int c = 0; c < kChunks; c++) epi(c, acc2[0], jp & 31);
          }
          flush(jp);
        }
      }
    }
  }
}

// The same kernel for the small-slot classes: pdfs of at most kSlot ∈ {16, 8, 4} Gaussians occupy kSlot consecutive model
// rows (pad rows: zero weights, gconst −1e30), and 32 / kSlot of them — whichever the utterance's list puts next to each
// other — are gathered into one virtual 32-row block: global_load_lds takes a per-lane source address, so the copy costs
// what the contiguous one does.  The MFMAs are those of the 32-row class; the log-sum-exp runs over the kSlot rows of each
// pdf (accumulator registers [8k, 8k+8) of both half-waves for kSlot = 16, [4k, 4k+4) for 8, [4i, 4i+4) of ONE half-wave
// for 4) and a block yields 32 / kSlot score columns.  Not software-pipelined (the epilogues differ per class and these
// classes are a minority of the rows of a 32-Gaussian model; for MFA's released models they are the majority — next step).
template <int kSteps, int kPieces, int kSlot>
__global__ __launch_bounds__(256, 2) void gmm_split_small_kernel(GmmParams p) {
  constexpr int kNT = 2, kWaves = 4, kFramesPerWave = 64, kFramesPerTile = 256;
  constexpr bool kHalf = kPieces == 2;
  using op8 = std::conditional_t<kHalf, f16x8, bf16x8>;
  constexpr int kUnits = kSteps * kPieces * 2 * 32;    // 16-byte units per block
  constexpr int kLoads = (kUnits + 255) / 256;         // units each thread moves per block
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float stage_all[kWaves][64 * 33];
  __shared__ uint4 a_lds[2][kUnits];
  __shared__ __attribute__((aligned(16))) float gc_lds[2][64];
  constexpr int kPdfs = 32 / kSlot;                   // pdfs per virtual block = score columns per block
  constexpr int kCls = kSlot == 16 ? 2 : kSlot == 8 ? 3 : 4;   // position of this class in class_counts
  constexpr int kBlkCache = 1024;                     // pdf → first model row, staged per item (two dependent global loads
  __shared__ int blk_lds[kBlkCache];                  // per pdf must not sit in the block loop); a multiple of 32 pdfs
  __shared__ int s_item;
  float *stage = stage_all[wave];
  if (!kHalf && p.redo_mode == 2 && *p.redo_count == 0) return;   // uniform: the f16 pass declined nothing
  const int my_xcd = (int)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u);
  for (int hop = 0; hop < 8; hop++) {
    const int q = (my_xcd + hop) & 7;
    const int n_items = ((p.n_utt - q + 7) >> 3) * p.tiles;
    for (;;) {
      __syncthreads();
      if (threadIdx.x == 0) s_item = atomicAdd(&p.queue[q], 1);
      __syncthreads();
      const int item = s_item;
      if (item >= n_items) break;
      int lane = lane0;                                // opaque per item: keeps lane-dependent addresses out of long-lived registers
      asm volatile("" : "+v"(lane));
      const int col = lane & 31, h = lane >> 5;
      const int utt = (item / p.tiles) * 8 + q, tl = p.tiles - 1 - item % p.tiles;
      const int64_t f0 = p.frame_off[utt];
      const int T = (int)(p.frame_off[utt + 1] - f0);
      if (tl * kFramesPerTile >= T) continue;          // uniform over the workgroup
      if (!kHalf && p.redo_mode == 2 && p.redo[(size_t)utt * p.tiles + tl] == 0) continue;   // only what the f16 pass left
      const int t_base = (tl * kWaves + wave) * kFramesPerWave;
      const bool active = t_base < T;                  // a wavefront past the end still helps move blocks and joins barriers
      const int64_t l0 = p.pdf_off[utt];
      const int P = (int)(p.pdf_off[utt + 1] - l0);
      const int32_t *list = p.pdf_list + l0;
      const int32_t *cc6 = p.class_counts + (size_t)utt * 6;
      int base = cc6[0] + cc6[1];                      // columns of the classes in front of this one
#pragma unroll
      for (int q3 = 2; q3 < kCls; q3++) base += cc6[q3];
      const int n_all = cc6[kCls];
      if (n_all == 0) continue;                        // uniform
      // n_single: pdfs the tile's LAST frame can be asked for — the prefix the workgroup walks together (block copies and
      // barriers are collective).  n_mine: the shorter prefix this wavefront's own 64 frames can be asked for; beyond it
      // the wavefront only helps with the copies.
      int n_single = n_all, n_mine = n_all;
      if (p.first_frame) {
        const int t_last = min(T, (tl + 1) * kFramesPerTile) - 1;
        const int t_mine = min(T, t_base + kFramesPerWave) - 1;
        n_single = 0; n_mine = 0;
        for (int i0 = 0; i0 < n_all; i0 += 64) {
          const int i = i0 + lane;
          const int ff = i < n_all ? p.first_frame[l0 + base + i] : 0x7fffffff;
          n_single = max(n_single, prefix_end(__ballot(ff <= t_last), i0));   // (see gmm_bf16_kernel: superset for grouped plans)
          n_mine = max(n_mine, prefix_end(__ballot(ff <= t_mine), i0));
        }
      }
      float *out = p.out + p.ll_off[utt];
      if (n_single > 0) {
        // ---- x̃ = [x, x²] of this wavefront's 64 frames, split into bf16 triples: b[tile][step][piece], lane (frame, half)
        op8 b[kNT][kSteps][kPieces];
        // kHalf: `bad` = a scaled feature outside the f16 range (or NaN)
        const bool bad = split_features<kSteps, kPieces>(p, f0, T, t_base, col, h, b);
        if constexpr (kHalf) {
          if (__syncthreads_or(bad)) {                     // uniform: the whole tile goes to the bf16×3 pass
            if (threadIdx.x == 0) { p.redo[(size_t)utt * p.tiles + tl] = 1; atomicAdd(p.redo_count, 1); }
            continue;
          }
        }
        const uint4 *wsrc = kHalf ? p.wh : p.wb;
        const float *gsrc = kHalf ? p.gch : p.gc;
        const float inv_s = kHalf ? p.acc_scale_inv : 1.0f;
        const float l2e_s = 1.44269504088896341f * inv_s;  // inv_s is a power of two: (x·inv_s)·log2e == x·(log2e·inv_s)
        // Block copy global → LDS without a register stop (global_load_lds_dwordx4: every lane's 16 bytes land at a
        // wavefront-uniform LDS base + 16·lane, which is exactly the linear unit order of a block).
        typedef __attribute__((address_space(1))) const void *gptr_t;
        typedef __attribute__((address_space(3))) void *lptr_t;
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        // virtual block jb = pdfs [jb·kPdfs, (jb+1)·kPdfs) of the class; lane ↔ row ρ = lane mod 32 of every 32-unit group
        const int rho = lane & 31, my_k = rho / kSlot, my_r = rho % kSlot;
        auto fetch = [&](int jb, int buf, int c0, int c1) {
          const int idx = jb * kPdfs + my_k;               // pdf this lane's row belongs to (class-relative)
          const int row = idx < c1 ? blk_lds[idx - c0] + my_r : p.num_rows;   // past the needed prefix: the dummy row
          const uint4 *src = wsrc + (size_t)(row >> 5) * kUnits + (row & 31);
#pragma unroll
          for (int i = 0; i < kLoads; i++) {
            const int u0 = 64 * wave_u + 256 * i;        // first unit this wavefront moves in round i (uniform)
            if (u0 < kUnits)
              __builtin_amdgcn_global_load_lds((gptr_t)(src + ((u0 + lane) & ~31)), (lptr_t)&a_lds[buf][u0], 16, 0, 0);
          }
          if (wave_u == 0)
            __builtin_amdgcn_global_load_lds((gptr_t)(gsrc + row), (lptr_t)&gc_lds[buf][0], 4, 0, 0);
        };
        auto landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
        // ---- block loop: multiply, reduce per pdf, stage one column per pdf, flush every 32 columns
        const int nb_mine = (n_mine + kPdfs - 1) / kPdfs;   // virtual blocks this wavefront multiplies
        auto flush = [&](int col_last) {                     // columns [col_last − col_last%32, col_last] → HBM
          const int jj = col_last & 31;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          const int j0 = col_last - jj, cnt = min(jj + 1, n_mine - j0);
#pragma unroll 4
          for (int i = 0; i < 32; i++) {
            const int r = h + 2 * i, t = t_base + r;
            if (col < cnt && t < T) __builtin_nontemporal_store(stage[r * 33 + col], &out[(size_t)t * P + base + j0 + col]);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        };
        // Σ exp(x − m) over `cnt` registers from r0, pairwise; m: their maximum
        auto group_max = [&](const f32x16 &v, int r0, int cnt) {
          float m = v[r0];
#pragma unroll
          for (int r = 1; r < cnt; r++) m = fmaxf(m, v[r0 + r]);
          return m;
        };
        auto group_expsum = [&](const f32x16 &v, int r0, int cnt, float m) {
          float e[8];
#pragma unroll
          for (int r = 0; r < cnt; r++) e[r] = __builtin_amdgcn_exp2f((v[r0 + r] - m) * l2e_s);
#pragma unroll
          for (int w = 1; w < cnt; w <<= 1)
#pragma unroll
            for (int r = 0; r + w < cnt; r += 2 * w) e[r] += e[r + w];
          return e[0];
        };
        int pending = -1;                                  // last column of a staged window waiting to be written out
        for (int c0 = 0; c0 < n_single; c0 += kBlkCache) {
        const int c1 = min(n_single, c0 + kBlkCache);
        __syncthreads();                                   // previous chunk's table is no longer read
        for (int i = c0 + threadIdx.x; i < c1; i += 256) blk_lds[i - c0] = p.row0[list[base + i]];
        __syncthreads();
        const int jb0 = c0 / kPdfs, jb1 = (c1 + kPdfs - 1) / kPdfs;
        fetch(jb0, 0, c0, c1);
        landed();
        __syncthreads();
        for (int jb = jb0; jb < jb1; jb++) {
          const int buf = (jb - jb0) & 1;
          if (pending >= 0) { flush(pending); pending = -1; }   // a block early: see "score stores" in gmm_split_single_kernel
          fetch(min(jb + 1, jb1 - 1), buf ^ 1, c0, c1);
          if (active && jb < nb_mine) {
            f32x16 acc[kNT];
            multiply_block<kSteps, kPieces>(a_lds[buf], gc_lds[buf], b, acc, col, h);
            // ---- per-pdf log-sum-exp.  Accumulator register r of half-wave h is row (r & 3) + 8 (r >> 2) + 4 h.
            const int colbase = (jb * kPdfs) & 31;           // first staging column of this block
#pragma unroll
            for (int n = 0; n < kNT; n++) {
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
            const int col_last = min((jb + 1) * kPdfs, n_mine) - 1;   // last valid column this block produced
            if ((col_last & 31) == 31 || jb == nb_mine - 1) pending = col_last;
          }
          landed();
          __syncthreads();                                 // block jb+1 is in place; everybody is done with block jb
        }
        }
        if (pending >= 0) flush(pending);
      }
    }
  }
}

// Band-mode launch of the f32 kernel's tile walk over the (utterance, 64-frame sub-tile) items of a lazy-scoring window
// (gmm_band.hip): the classes gmm_band_kernel left (b_skip0: single-Gaussian pdfs, bit-exact), or every class under
// MFA_GMM_BF16=0.  It stays in this unit, next to score_tile and gmm_kernel: compiled without gmm_kernel beside it, the
// inlined tile walk gets another register assignment.
template <int M8>
__global__ __launch_bounds__(256, 2) void gmm_band_f32_kernel(GmmParams p) {
  __shared__ float stage_all[4][64 * 33];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int utt, r;
  if (!band_item(p, wave, utt, r)) return;
  score_tile<M8, 2>(p, utt, band_t_begin(p, utt) + 64 * r, lane, stage_all[wave], 0);
}

// The list passes' launch of the same walk: a small fixed grid, every wavefront taking the items first, first + stride, …
// (band_walk) — a list holds a handful of utterances, a full grid one wavefront per sub-tile of the whole batch.
template <int M8>
__global__ __launch_bounds__(256, 2) void gmm_band_f32_strided_kernel(GmmParams p) {
  __shared__ float stage_all[4][64 * 33];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const BandWalk w = band_walk(p, wave, false);
  for (int witem = w.first; witem < w.n_witems; witem += w.stride) {
    int utt, r;
    if (!band_witem(p, witem, utt, r)) continue;
    score_tile<M8, 2>(p, utt, band_t_begin(p, utt) + 64 * r, lane, stage_all[wave], 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // the stage goes to the next item
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// max over the batch of the pdfs' first possible frames → *max_ff (the persistent kernel derives its phase split from it)
__global__ void gmm_max_first_frame_kernel(const int32_t *first_frame, const int64_t *pdf_off, int n_utt, int *out) {
  const int64_t n = pdf_off[n_utt];
  int m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, first_frame[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(out, m);
}

// Straightforward one-thread-per-(frame,pdf) kernel: used for feature dims the MFMA kernel is not instantiated for and,
// with MFA_GMM_NAIVE=1, as an on-device cross-check of the MFMA path.  Same fmaf chain, same log-sum-exp.
__global__ void gmm_naive_kernel(GmmParams p) {
  const int utt = blockIdx.y;
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const int64_t l0 = p.pdf_off[utt];
  const int P = (int)(p.pdf_off[utt + 1] - l0);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)T * P) return;
  const int t = (int)(idx / P), j = (int)(idx % P);
  const int pdf = p.pdf_list[l0 + j];
  const int r0 = p.row0[pdf];
  const int rows = p.slot[pdf] == 32 ? 32 * p.nblk[pdf] : p.slot[pdf];  // pad rows carry gconst -1e30
  const float *x = p.feats + (f0 + t) * p.dim;
  float mx = -INFINITY;
  double sum = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    for (int r = 0; r < rows; r++) {
      float acc = p.gc[r0 + r];
      for (int k = 0; k < 2 * p.dim; k++) {
        float xv = k < p.dim ? x[k] : x[k - p.dim] * x[k - p.dim];
        acc = fmaf(p.w[mfa_packed_offset(r0 + r, k, p.kpad)], xv, acc);
      }
      if (pass == 0) mx = fmaxf(mx, acc);
      else if (acc >= mx + p.min_log_diff) sum += (double)expf(acc - mx);
    }
  }
  p.out[p.ll_off[utt] + (size_t)t * P + j] = (float)((double)mx + log(sum));
}

int slot_of(int g) { return g <= 1 ? 1 : g <= 4 ? 4 : g <= 8 ? 8 : g <= 16 ? 16 : 32; }
int class_index(int slot) { return slot == 32 ? 0 : slot == 16 ? 1 : slot == 8 ? 2 : slot == 4 ? 3 : 4; }

}  // namespace

extern "C" {

MFA_API int mfa_load_gmm(mfa_ctx *c, int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                         const float *h_means_invvars, const float *h_inv_vars) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (dim <= 0 || num_pdfs <= 0) return c->fail("mfa_load_gmm: bad dim/num_pdfs %d/%d", dim, num_pdfs);
  // the MFMA kernel is instantiated for rows of exactly 80 or 96 floats; wider models use the naive kernel
  const int kpad = 2 * dim <= 80 ? 80 : (2 * dim <= 96 ? 96 : ((2 * dim + 7) / 8) * 8);
  std::vector<int32_t> row0(num_pdfs + 1), nblk(num_pdfs), slot(num_pdfs);
  for (int p = 0; p < num_pdfs; p++) {
    int g = h_pdf_offsets[p + 1] - h_pdf_offsets[p];
    if (g <= 0) return c->fail("mfa_load_gmm: pdf %d has no Gaussians", p);
    slot[p] = slot_of(g);
    nblk[p] = slot[p] == 32 ? (g + 31) / 32 : 1;
  }
  // rows are handed out class by class (32, 16, 8, 4, 1): every pdf then starts at a multiple of its slot size, so the
  // gconst rows of a 32-row block can be fetched with aligned 16-byte loads
  int rows = 0;
  for (int cls : {32, 16, 8, 4, 1})
    for (int p = 0; p < num_pdfs; p++)
      if (slot[p] == cls) { row0[p] = rows; rows += cls == 32 ? 32 * nblk[p] : cls; }
  rows = (rows + 3) & ~3;
  row0[num_pdfs] = rows;
  // whole 32-row blocks, plus room for the dummy row `rows` (zero weights, gconst −1e30) that idle lanes address
  const int blocks = (rows + 1 + 31) / 32;
  std::vector<float> w((size_t)blocks * 32 * kpad, 0.0f), gc((size_t)blocks * 32, kPadGconst);
  for (int p = 0; p < num_pdfs; p++) {
    int g0 = h_pdf_offsets[p], g = h_pdf_offsets[p + 1] - g0;
    for (int i = 0; i < g; i++) {
      const float *mi = h_means_invvars + (size_t)(g0 + i) * dim, *iv = h_inv_vars + (size_t)(g0 + i) * dim;
      for (int k = 0; k < 2 * dim; k++)
        w[mfa_packed_offset(row0[p] + i, k, kpad)] = k < dim ? mi[k] : -0.5f * iv[k - dim];
      gc[row0[p] + i] = h_gconsts[g0 + i];
    }
  }
  // bf16×3 split for the opt-in bf16 kernel: blocks of [step][piece][half][row] × 8 bf16 (natural k order, zero padded)
  std::vector<uint16_t> wb;
  const int steps = kpad / 16;
  const bool want_bf16 = (kpad == 80 || kpad == 96);
  if (want_bf16) {
    wb.assign((size_t)blocks * steps * 3 * 2 * 32 * 8, 0);
    auto to_bf16 = [](float f) -> uint16_t {   // round to nearest even, as the device's v_cvt_pk_bf16_f32
      uint32_t u; memcpy(&u, &f, 4);
      u += 0x7FFFu + ((u >> 16) & 1u);
      return (uint16_t)(u >> 16);
    };
    auto from_bf16 = [](uint16_t b) -> float { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; };
    for (int row = 0; row < rows; row++) {
      for (int k = 0; k < 2 * dim; k++) {
        const float v = w[mfa_packed_offset(row, k, kpad)];
        const uint16_t v1 = to_bf16(v);
        const float r1 = v - from_bf16(v1);
        const uint16_t v2 = to_bf16(r1);
        const float r2 = r1 - from_bf16(v2);
        const uint16_t piece[3] = {v1, v2, to_bf16(r2)};
        const int s_ = k >> 4, hh = (k >> 3) & 1, e = k & 7;
        for (int qq = 0; qq < 3; qq++) {
          const size_t unit = (size_t)(row >> 5) * steps * 3 * 2 * 32 + (size_t)((s_ * 3 + qq) * 2 + hh) * 32 + (row & 31);
          wb[unit * 8 + e] = piece[qq];
        }
      }
    }
  }
  // f16×2 split (default scoring path of the 32-row classes without multi-block pdfs).  Column k of the weights is
  // multiplied by 2^e_k and column k of x̃ by S·2^-e_k, so every product — and the gconst, stored × S — carries the one
  // factor S and nothing is rounded differently.  The exponents balance the two operands inside the f16 range using the
  // model's own idea of how large a feature can get (|μ| + 10σ over all Gaussians); features beyond 65000 after scaling
  // are caught per tile on the device (see gmm_split_single_kernel).
  std::vector<uint16_t> wh;
  std::vector<float> fscale(kpad, 0.0f), gch;
  float acc_scale = 1.0f;
  if (want_bf16) {
    std::vector<double> wmax(2 * dim, 0.0), xmax(2 * dim, 0.0);
    for (int p = 0; p < num_pdfs; p++) {
      int g0 = h_pdf_offsets[p], g = h_pdf_offsets[p + 1] - g0;
      for (int i = 0; i < g; i++) {
        const float *mi = h_means_invvars + (size_t)(g0 + i) * dim, *iv = h_inv_vars + (size_t)(g0 + i) * dim;
        for (int k = 0; k < dim; k++) {
          const double v = iv[k], m = mi[k];
          if (std::isfinite(m)) wmax[k] = std::max(wmax[k], std::fabs(m));
          if (std::isfinite(v)) wmax[dim + k] = std::max(wmax[dim + k], 0.5 * std::fabs(v));
          if (std::isfinite(v) && std::isfinite(m) && v > 0) {
            const double reach = std::fabs(m / v) + 10.0 / std::sqrt(v);
            if (std::isfinite(reach)) { xmax[k] = std::max(xmax[k], reach); xmax[dim + k] = std::max(xmax[dim + k], reach * reach); }
          }
        }
      }
    }
    int log_s = 12;
    for (int k = 0; k < 2 * dim; k++)
      if (wmax[k] > 0 && xmax[k] > 0) log_s = std::min(log_s, (int)std::floor(26.0 - std::log2(wmax[k] * xmax[k])));
    log_s = std::max(log_s, -20);
    acc_scale = std::ldexp(1.0f, log_s);
    std::vector<int> e_w(2 * dim, 0);
    for (int k = 0; k < 2 * dim; k++) {
      if (!(wmax[k] > 0)) { fscale[k] = 0.0f; continue; }           // an all-zero weight column: x̃_k is irrelevant
      const double xm = xmax[k] > 0 ? xmax[k] : 1.0;
      int e = (int)std::lround(0.5 * (log_s + std::log2(xm) - std::log2(wmax[k])));
      while (std::ldexp(wmax[k], e) > 32768.0) e--;                 // never let the weights themselves leave the range
      e = std::max(-100, std::min(100, e));
      e_w[k] = e;
      fscale[k] = (float)std::ldexp(1.0, log_s - e);
    }
    wh.assign((size_t)blocks * steps * 2 * 2 * 32 * 8, 0);
    auto f16_bits = [](float f) -> uint16_t { _Float16 hv = (_Float16)f; uint16_t u; memcpy(&u, &hv, 2); return u; };
    for (int row = 0; row < rows; row++) {
      for (int k = 0; k < 2 * dim; k++) {
        const float v = std::ldexp(w[mfa_packed_offset(row, k, kpad)], e_w[k]);
        const _Float16 v1 = (_Float16)v;
        const float r1 = v - (float)v1;
        const uint16_t piece[2] = {f16_bits(v), f16_bits(r1)};
        const int s_ = k >> 4, hh = (k >> 3) & 1, e = k & 7;
        for (int qq = 0; qq < 2; qq++) {
          const size_t unit = (size_t)(row >> 5) * steps * 2 * 2 * 32 + (size_t)((s_ * 2 + qq) * 2 + hh) * 32 + (row & 31);
          wh[unit * 8 + e] = piece[qq];
        }
      }
    }
    gch.resize(gc.size());
    for (size_t i = 0; i < gc.size(); i++) gch[i] = gc[i] * acc_scale;
  }
  void *old[] = {c->d_w, c->d_gc, c->d_row0, c->d_nblk, c->d_slot, c->d_nrows, c->d_wb, c->d_wh, c->d_gch, c->d_fscale};
  c->d_wb = nullptr; c->d_wh = nullptr; c->d_gch = nullptr; c->d_fscale = nullptr;
  for (void *q : old) if (q) (void)hipFree(q);
  c->d_w = nullptr; c->d_gc = nullptr; c->d_row0 = nullptr; c->d_nblk = nullptr; c->d_slot = nullptr; c->d_nrows = nullptr;
  MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_w, w.size() * 4));
  MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_gc, gc.size() * 4));
  MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_row0, row0.size() * 4));
  MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_nblk, nblk.size() * 4));
  MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_slot, slot.size() * 4));
  MFA_HIP_CHECK(c, hipMemcpy(c->d_w, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  if (want_bf16) {
    MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_wb, wb.size() * 2));
    MFA_HIP_CHECK(c, hipMemcpy(c->d_wb, wb.data(), wb.size() * 2, hipMemcpyHostToDevice));
    MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_wh, wh.size() * 2));
    MFA_HIP_CHECK(c, hipMemcpy(c->d_wh, wh.data(), wh.size() * 2, hipMemcpyHostToDevice));
    MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_gch, gch.size() * 4));
    MFA_HIP_CHECK(c, hipMemcpy(c->d_gch, gch.data(), gch.size() * 4, hipMemcpyHostToDevice));
    MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_fscale, fscale.size() * 4));
    MFA_HIP_CHECK(c, hipMemcpy(c->d_fscale, fscale.data(), fscale.size() * 4, hipMemcpyHostToDevice));
    c->gmm_acc_scale = acc_scale;
  }
  MFA_HIP_CHECK(c, hipMemcpy(c->d_gc, gc.data(), gc.size() * 4, hipMemcpyHostToDevice));
  MFA_HIP_CHECK(c, hipMemcpy(c->d_row0, row0.data(), row0.size() * 4, hipMemcpyHostToDevice));
  MFA_HIP_CHECK(c, hipMemcpy(c->d_nblk, nblk.data(), nblk.size() * 4, hipMemcpyHostToDevice));
  MFA_HIP_CHECK(c, hipMemcpy(c->d_slot, slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
  c->dim = dim; c->kpad = kpad; c->num_pdfs = num_pdfs; c->num_rows = rows;
  c->h_slot = slot;
  c->h_nblk = nblk;
  c->h_row0.assign(row0.begin(), row0.begin() + num_pdfs);
  c->h_ngauss.resize(num_pdfs);
  for (int p = 0; p < num_pdfs; p++) c->h_ngauss[p] = h_pdf_offsets[p + 1] - h_pdf_offsets[p];
  if (c->d_w_stats) { (void)hipFree(c->d_w_stats); c->d_w_stats = nullptr; }   // belonged to the previous model's layout
  if (c->d_nrows) { (void)hipFree(c->d_nrows); c->d_nrows = nullptr; }
  c->all_pdfs_32row = true;
  c->has_multi_block = false;
  c->max_nblk = 1;
  for (int q = 0; q < 5; q++) c->has_slot_class[q] = false;
  c->has_single32 = false;
  for (int p = 0; p < num_pdfs; p++) {
    if (slot[p] != 32) c->all_pdfs_32row = false;
    if (nblk[p] > 1) c->has_multi_block = true;
    c->max_nblk = std::max(c->max_nblk, nblk[p]);
    if (slot[p] == 32 && nblk[p] == 1) c->has_single32 = true;
    c->has_slot_class[class_index(slot[p])] = true;
  }
  c->gmm_ready = true;
  return 0;
}

MFA_API int32_t mfa_gmm_slot(mfa_ctx *c, int32_t pdf) {
  if (!c->gmm_ready || pdf < 0 || pdf >= c->num_pdfs) return -1;
  return c->h_slot[pdf];
}

MFA_API int mfa_gmm_sort_pdf_list(mfa_ctx *c, int32_t *h_pdfs, int32_t n, int32_t *h_class_counts) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  std::vector<int32_t> bucket[6];
  for (int i = 0; i < n; i++) {
    int p = h_pdfs[i];
    if (p < 0 || p >= c->num_pdfs) return c->fail("pdf id %d out of range [0,%d)", p, c->num_pdfs);
    int ci = class_index(c->h_slot[p]);
    bucket[ci == 0 ? (c->h_nblk[p] == 1 ? 0 : 1) : ci + 1].push_back(p);
  }
  int k = 0;
  for (int b = 0; b < 6; b++) {
    h_class_counts[b] = (int32_t)bucket[b].size();
    for (int p : bucket[b]) h_pdfs[k++] = p;
  }
  return 0;
}

MFA_API int mfa_gmm_sort_pdf_list_keyed(mfa_ctx *c, int32_t *h_pdfs, int32_t *h_first_frame, int32_t n,
                                        int32_t *h_class_counts) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  std::vector<std::pair<int32_t, int32_t>> bucket[6];  // (key, pdf)
  for (int i = 0; i < n; i++) {
    int p = h_pdfs[i];
    if (p < 0 || p >= c->num_pdfs) return c->fail("pdf id %d out of range [0,%d)", p, c->num_pdfs);
    int ci = class_index(c->h_slot[p]);
    bucket[ci == 0 ? (c->h_nblk[p] == 1 ? 0 : 1) : ci + 1].push_back({h_first_frame[i], p});
  }
  int k = 0;
  for (int b = 0; b < 6; b++) {
    std::stable_sort(bucket[b].begin(), bucket[b].end(),
                     [](const std::pair<int32_t, int32_t> &x, const std::pair<int32_t, int32_t> &y) { return x.first < y.first; });
    h_class_counts[b] = (int32_t)bucket[b].size();
    for (auto &e : bucket[b]) { h_first_frame[k] = e.first; h_pdfs[k++] = e.second; }
  }
  return 0;
}

MFA_API int mfa_debug_gmm_trace(mfa_ctx *c, void *d_trace) {
  c->gmm_trace = d_trace;
  return 0;
}

MFA_API int mfa_gmm_score_batch(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                int32_t max_frames, const int32_t *d_pdf_list, const int64_t *d_pdf_off,
                                const int32_t *d_class_counts, const int32_t *d_pdf_first_frame, const int64_t *d_ll_off,
                                float *d_loglikes) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  if (n_utt <= 0 || max_frames <= 0) return 0;
  if (n_utt > 65535) return c->fail("at most 65535 utterances per scoring launch (got %d)", n_utt);
  GmmParams p;
  memset(&p, 0, sizeof(p));   // every field this function does not set (the band-mode ones) must read as "off"
  p.dim = c->dim; p.kpad = c->kpad; p.num_rows = c->num_rows;
  p.w = c->d_w; p.gc = c->d_gc; p.row0 = c->d_row0; p.nblk = c->d_nblk; p.slot = c->d_slot;
  p.feats = d_feats; p.frame_off = d_frame_off; p.pdf_list = d_pdf_list; p.pdf_off = d_pdf_off;
  p.class_counts = d_class_counts; p.ll_off = d_ll_off; p.out = d_loglikes;
  p.min_log_diff = logf(1.1920928955078125e-07f);
  p.first_frame = d_pdf_first_frame;
  p.trace = (unsigned long long *)c->gmm_trace;
  const char *naive = getenv("MFA_GMM_NAIVE");
  KernelTimer kt(c, MFA_K_GMM);
  if ((naive && naive[0] == '1') || c->kpad > 96) {
    // worst-case P is not known on the host side of this call: cover max_frames * num_pdfs threads per utterance
    int64_t per_utt = (int64_t)max_frames * c->num_pdfs;
    dim3 grid((unsigned)((per_utt + 255) / 256), n_utt);
    hipLaunchKernelGGL(gmm_naive_kernel, grid, dim3(256), 0, c->stream, p);
  } else {
    // 4 wavefronts per workgroup, 2 frame tiles (64 frames) per wavefront, two workgroups resident per CU (206 VGPRs).
    // Variants measured and dropped in round 1: 1 tile per wavefront (3 per SIMD: 30 TFLOP/s, spills), 8-wavefront
    // workgroups with or without a static s_setprio split (103 TFLOP/s), one wavefront per SIMD with 4 tiles and an
    // in-wavefront MFMA/epilogue software pipeline (97 TFLOP/s).
    constexpr int kFramesPerItem = 256;
    p.n_utt = n_utt;
    p.tiles = (max_frames + kFramesPerItem - 1) / kFramesPerItem;
    constexpr int kQueueInts = 64 + 8 * 16;   // counters of the main launches + six small-slot launches + the multi-block one
    if (!c->d_gmm_queue) MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_gmm_queue, kQueueInts * sizeof(int)));
    MFA_HIP_CHECK(c, hipMemsetAsync(c->d_gmm_queue, 0, kQueueInts * sizeof(int), c->stream));
    p.queue = c->d_gmm_queue;
    p.max_ff = c->d_gmm_queue + 16;
    if (d_pdf_first_frame)
      hipLaunchKernelGGL(gmm_max_first_frame_kernel, dim3(64), dim3(256), 0, c->stream, d_pdf_first_frame, d_pdf_off, n_utt,
                         c->d_gmm_queue + 16);
    if (c->num_cus <= 0) {
      hipDeviceProp_t prop;
      MFA_HIP_CHECK(c, hipGetDeviceProperties(&prop, c->device));
      c->num_cus = prop.multiProcessorCount;
    }
    const int64_t items = (int64_t)n_utt * p.tiles;
    const int64_t wgs = std::min<int64_t>((int64_t)c->num_cus * 2, items);
    dim3 grid((unsigned)std::max<int64_t>(wgs, 1));
    const GmmSplitPasses passes = gmm_split_passes(c);
    // one launch of a kernel template whose first parameter is the model's 16-k step count
    auto launch = [&](auto kernel_of) { gmm_with_steps(c->kpad, [&](auto steps) { hipLaunchKernelGGL(kernel_of(steps), grid, dim3(256), 0, c->stream, p); }); };
    p.wb = (const uint4 *)c->d_wb;
    p.wh = nullptr; p.gch = nullptr; p.fscale = nullptr; p.acc_scale_inv = 1.0f; p.redo = nullptr; p.redo_mode = 0; p.redo_count = nullptr; p.skip_cc0 = 0;
    p.skip_single = 0;
    if (passes.bf16) {   // default on; MFA_GMM_BF16=0 keeps every class on the f32 kernel
      // class 0 on the bf16×3 kernel, then the f32 kernel for whatever other slot classes the lists hold (second set of
      // queue counters; an item with nothing left returns at once)
      const bool f16_ok = passes.f16;
      const bool use_f16 = f16_ok && c->has_single32;   // single-block 32-row class on the lean f16 kernel
      p.skip_cc0 = 0;
      if (f16_ok) {
        // an f16×2 pass scores every tile it can and flags the others for the bf16×3 pass that follows it
        if (c->gmm_redo_cap < items) {
          if (c->d_gmm_redo) (void)hipFree(c->d_gmm_redo);
          c->d_gmm_redo = nullptr; c->gmm_redo_cap = 0;
          MFA_HIP_CHECK(c, hipMalloc((void **)&c->d_gmm_redo, items * sizeof(int)));
          c->gmm_redo_cap = items;
        }
        MFA_HIP_CHECK(c, hipMemsetAsync(c->d_gmm_redo, 0, items * sizeof(int), c->stream));
        p.wh = (const uint4 *)c->d_wh; p.gch = c->d_gch; p.fscale = c->d_fscale;
        p.acc_scale_inv = 1.0f / c->gmm_acc_scale;
        p.redo = c->d_gmm_redo; p.redo_mode = 0; p.redo_count = c->d_gmm_queue + 51;
      }
      if (use_f16) {
        launch([](auto steps) { return gmm_split_single_kernel<steps(), 2>; });
        p.redo_mode = 2;
        p.queue = c->d_gmm_queue + 34;
        launch([](auto steps) { return gmm_split_single_kernel<steps(), 3>; });
        p.redo_mode = 0;
        p.skip_cc0 = 1;
        p.queue = c->d_gmm_queue + 64 + 6 * 16;
      }
      if (c->has_multi_block) {                           // pdfs of more than 32 Gaussians (and, without f16, the whole 32-row class)
        if (f16_ok) {                                     // f16×2 pass, then the bf16×3 pass over the tiles it declined
          launch([](auto steps) { return gmm_bf16_kernel<steps(), 2>; });
          p.redo_mode = 2;
          p.queue = c->d_gmm_queue + 64 + 7 * 16;
        }
        launch([](auto steps) { return gmm_bf16_kernel<steps(), 3>; });
        p.redo_mode = 0;
      } else if (!use_f16 && c->has_single32) {
        launch([](auto steps) { return gmm_split_single_kernel<steps(), 3>; });
      }
      p.skip_single = 1;
      {
        // the 16- / 8- / 4-row classes on the same pipe (f16×2 pass, then the bf16×3 pass over declined tiles), each launch
        // with its own queue counters; classes the model does not have are not launched
        int qbase = 64;
        auto small = [&](auto slot_rows, int cls_idx) {
          if (!c->has_slot_class[cls_idx]) return;
          for (int pass = f16_ok ? 0 : 1; pass < 2; pass++) {
            p.redo_mode = f16_ok ? (pass == 0 ? 0 : 2) : 0;
            p.queue = c->d_gmm_queue + qbase; qbase += 16;
            if (pass == 0) launch([=](auto steps) { return gmm_split_small_kernel<steps(), 2, slot_rows()>; });
            else launch([=](auto steps) { return gmm_split_small_kernel<steps(), 3, slot_rows()>; });
          }
        };
        small(std::integral_constant<int, 16>{}, 1); small(std::integral_constant<int, 8>{}, 2); small(std::integral_constant<int, 4>{}, 3);
        p.skip_single = 2;
      }
      p.queue = c->d_gmm_queue + 17;
    }
    const bool only_split_classes = !c->has_slot_class[4] && p.skip_single == 2;   // no single-Gaussian pdfs left over
    if (p.skip_single && (c->all_pdfs_32row || only_split_classes)) {
      // every pdf of the model went to the split-operand kernels: nothing is left for the f32 kernel
    } else launch([](auto steps) { return gmm_kernel<2 * steps(), 2, 2, 4>; });
  }
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "dense scoring of %d utterances", n_utt);
  return 0;
}

}  // extern "C"

void mfa_gmm_launch_band_f32(mfa_ctx *c, const void *params, dim3 grid, bool strided) {
  const GmmParams &p = *static_cast<const GmmParams *>(params);
  gmm_with_steps(c->kpad, [&](auto steps) {
    if (strided) hipLaunchKernelGGL((gmm_band_f32_strided_kernel<2 * steps()>), grid, dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL((gmm_band_f32_kernel<2 * steps()>), grid, dim3(256), 0, c->stream, p);
  });
}
