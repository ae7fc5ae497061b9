// The exact-f32 tile walk of the acoustic scoring (included by gmm.hip only; the arithmetic and the packed-row layout are
// described at the head of gmm.hip).  In this file:
//   Tile, reg_expsum, score_tile  one wavefront's walk of an utterance's pdf list for 64 frames on v_mfma_f32_32x32x2_f32;
//   gmm_kernel                    the persistent dense launch of that walk;
//   gmm_band_f32_kernel, gmm_band_f32_strided_kernel  the same walk over the band items of a lazy-scoring window
//                                 (mfa_gmm_launch_band_f32 in gmm.hip, for gmm_band.hip).
// The band launches stay in one translation unit with gmm_kernel: compiled without it beside them, the inlined tile walk
// gets another register assignment.
#pragma once
#include "gmm_common.hpp"

namespace {

// address of the 4-float piece (operand group 0, half h) of a packed row: see mfa_packed_offset in gmm_pack.hpp
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

}  // namespace
