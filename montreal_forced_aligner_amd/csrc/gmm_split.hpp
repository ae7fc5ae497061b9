// The dense split-operand kernels of the acoustic scoring (included by gmm.hip only; launch plan: mfa_gmm_score_batch).
// float32 products from two f16 (or three bf16) operand pieces on v_mfma_f32_32x32x16_{f16,bf16}, model blocks shared by a
// workgroup's four wavefronts through LDS.  In this file:
//   gmm_bf16_kernel          the general form: pdfs of more than 32 Gaussians as runs of blocks, merged online;
//   gmm_split_single_kernel  the lean, software-pipelined form for pdfs that are one 32-row block (17–32 Gaussians);
//   gmm_split_small_kernel   the 16-, 8- and 4-row slot classes as gathered virtual 32-row blocks.
// The arithmetic they share with each other and with gmm_band_kernel — product order, log-sum-exp, small-slot epilogue,
// staged flush — is gmm_common.hpp's; what only these three share (item walk, reachable prefix, decline) is defined here.
#pragma once
#include <type_traits>

#include "gmm_common.hpp"

namespace {

// ---- what the three kernels share beyond gmm_common.hpp
// One work item = (utterance, 256-frame tile); a workgroup's four wavefronts take 64 frames of it each.
struct DenseItem {
  int utt, tl;          // utterance, tile
  int64_t f0; int T;    // first frame of the utterance in p.feats, its frame count
  int t_base;           // this wavefront's first frame
  bool active;          // false: the wavefront lies past the utterance's end; it still helps move blocks and joins barriers
  int64_t l0; int P;    // the utterance's pdf list in p.pdf_list, its length = the row stride of `out`
  const int32_t *list;
  float *out;
};
// The persistent item walk.  One queue per XCD holds the utterances u ≡ xcd (mod 8) — all tiles of an utterance stream the
// same rows through that XCD's private L2 — items going utterance by utterance, last frames first; a workgroup whose queue
// is empty takes items from the other XCDs' queues, and everybody leaves once all eight counters have passed their counts.
// body(item, lane) runs for every item that has frames and, in a redo sweep (bf16×3 after f16×2: kHalf false, redo_mode 2),
// was declined by the f16 pass; it is entered by the whole workgroup.  `lane` is opaque per item: that keeps lane-dependent
// addresses out of long-lived registers.  (gmm_split_single_kernel keeps a copy of this walk: see the note there.)
template <bool kHalf, typename Body>
__device__ __forceinline__ void for_each_dense_item(const GmmParams &p, int &s_item, Body &&body) {
  constexpr int kWaves = 4, kFramesPerWave = 64, kFramesPerTile = 256;
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      DenseItem it;
      it.utt = (item / p.tiles) * 8 + q; it.tl = p.tiles - 1 - item % p.tiles;
      it.f0 = p.frame_off[it.utt];
      it.T = (int)(p.frame_off[it.utt + 1] - it.f0);
      if (it.tl * kFramesPerTile >= it.T) continue;          // uniform over the workgroup
      if (!kHalf && p.redo_mode == 2 && p.redo[(size_t)it.utt * p.tiles + it.tl] == 0) continue;   // only what the f16 pass left
      it.t_base = (it.tl * kWaves + wave) * kFramesPerWave;
      it.active = it.t_base < it.T;
      it.l0 = p.pdf_off[it.utt];
      it.P = (int)(p.pdf_off[it.utt + 1] - it.l0);
      it.list = p.pdf_list + it.l0;
      it.out = p.out + p.ll_off[it.utt];
      body(it, lane);
    }
  }
}

// How much of a class ordered by first frame (first_frame[0 .. n)) a tile needs: .x = the pdfs its LAST frame t_last can be
// asked for — the prefix the workgroup walks together (block copies and barriers are collective) — and .y = the shorter
// prefix this wavefront's own frames (up to t_mine) can be asked for; beyond it the wavefront only helps with the copies.
// A prefix ends behind the last pdf that can be asked for: the count for an ordered class, a superset of what is needed
// when a grouped plan lays the class out in several ordered runs.  (gmm_split_single_kernel keeps a copy: see the note
// there; gmm_bf16_kernel searches its two classes in one pass, in its own form.)
__device__ __forceinline__ int2 reachable_prefix(const int32_t *first_frame, int n, int t_last, int t_mine, int lane) {
  int n_all = 0, n_mine = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int ff = i < n ? first_frame[i] : 0x7fffffff;
    n_all = max(n_all, prefix_end(__ballot(ff <= t_last), i0));
    n_mine = max(n_mine, prefix_end(__ballot(ff <= t_mine), i0));
  }
  return make_int2(n_all, n_mine);
}

// f16 pass: a scaled feature of the tile left the f16 range (`bad` in some lane) — the whole tile is flagged for the bf16×3
// pass and not scored here.  Collective; true = declined.  (gmm_split_single_kernel keeps a copy: see the note there.)
__device__ __forceinline__ bool decline_tile(const GmmParams &p, int utt, int tl, bool bad) {
  if (!__syncthreads_or(bad)) return false;
  if (threadIdx.x == 0) { p.redo[(size_t)utt * p.tiles + tl] = 1; atomicAdd(p.redo_count, 1); }
  return true;
}

// Operand tables and scales of a pass: the f16 pass reads the column-scaled tables, its accumulators carry the factor S.
struct SplitSource { const uint4 *w; const float *gc; float inv_s, l2e_s; };
template <bool kHalf>
__device__ __forceinline__ SplitSource split_source(const GmmParams &p) {
  const float inv_s = kHalf ? p.acc_scale_inv : 1.0f;
  // inv_s is a power of two: (x·inv_s)·log2e == x·(log2e·inv_s), the scaling commutes with the rounding
  return {kHalf ? p.wh : p.wb, kHalf ? p.gch : p.gc, inv_s, 1.44269504088896341f * inv_s};
}

// Block copies global → LDS without a register stop (global_load_lds_dwordx4: every lane's 16 bytes land at a
// wavefront-uniform LDS base + 16·lane, which is exactly the linear unit order of a block; a 4-byte form for gathered gconsts)
typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;
__device__ __forceinline__ void copies_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

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
  using Ops = SplitOps<kPieces>;
  const f32x16 init = init_from_gconst(gc_blk, h);
  auto read_a = [&](int s, Op8 (&a)[kPieces]) {
#pragma unroll
    for (int qq = 0; qq < kPieces; qq++) a[qq] = __builtin_bit_cast(Op8, a_blk[((s * kPieces + qq) * 2 + h) * 32 + col]);
  };
  Op8 a_cur[kPieces], a_nxt[kPieces];
  read_a(0, a_cur);
#pragma unroll
  for (int s = 0; s < kSteps; s++) {
    if (s + 1 < kSteps) read_a(s + 1, a_nxt);
    Ops::mfma_step(a_cur, b, acc, init, s);
#pragma unroll
    for (int qq = 0; qq < kPieces; qq++) a_cur[qq] = a_nxt[qq];
  }
}

// kPieces = 3: bf16 triples; kPieces = 2: scaled f16 pairs with the per-tile range fallback (see gmm_split_single_kernel).
template <int kSteps, int kPieces>   // 16-k steps per row: 5 for D ≤ 40, 6 for D ≤ 48
__global__ __launch_bounds__(256, 2) void gmm_bf16_kernel(GmmParams p) {
  using Ops = SplitOps<kPieces>;
  using op8 = typename Ops::op8;
  constexpr bool kHalf = Ops::kHalf;
  constexpr int kNT = 2, kWaves = 4, kFramesPerWave = 64, kFramesPerTile = 256;
  constexpr int kUnits = kSteps * kPieces * 2 * 32;    // 16-byte units per block
  constexpr int kLoads = (kUnits + 255) / 256;         // units each thread moves per block
  const int wave = threadIdx.x >> 6;
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
  for_each_dense_item<kHalf>(p, s_item, [&](const DenseItem &it, int lane) {
      const int col = lane & 31, h = lane >> 5;
      const int utt = it.utt, tl = it.tl, T = it.T, t_base = it.t_base, P = it.P;
      const int64_t f0 = it.f0, l0 = it.l0;
      const bool active = it.active;
      const int32_t *list = it.list;
      float *out = it.out;
      const int cc0 = p.class_counts[(size_t)utt * 6], cc1 = p.class_counts[(size_t)utt * 6 + 1];
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
      if (n_entries > 0) {
        // ---- x̃ = [x, x²] of this wavefront's 64 frames, split into bf16 triples: b[tile][step][piece], lane (frame, half)
        op8 b[kNT][kSteps][kPieces];
        // kHalf: `bad` = a scaled feature outside the f16 range (or NaN)
        const bool bad = split_features<kSteps, kPieces>(p, f0, T, t_base, col, h, b);
        if constexpr (kHalf) {
          if (decline_tile(p, utt, tl, bad)) return;      // uniform: the whole tile goes to the bf16×3 pass
        }
        const SplitSource src_ = split_source<kHalf>(p);
        const uint4 *wsrc = src_.w;
        const float *gsrc = src_.gc;
        const float inv_s = src_.inv_s, l2e_s = src_.l2e_s;
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
        auto flush = [&]() { flush_staged(stage, out, P, t_base, T, stage_col0, staged, col, h); staged = 0; };
        for (int c0 = 0; c0 < n_entries; c0 += kBlkCache) {
        const int c1 = min(n_entries, c0 + kBlkCache);
        __syncthreads();                                   // previous chunk's table is no longer read
        for (int i = c0 + threadIdx.x; i < min(c1, n0); i += 256) {
          blk_lds[i - c0] = p.row0[list[i]] >> 5;
          col_lds[i - c0] = i | kFirst | kLast;
        }
        if (threadIdx.x == 0) {
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
          const int ecol = col_lds[j - c0];
          const int out_col = ecol & ~(kFirst | kLast);
          const bool mine = out_col < cc0 ? out_col < n0_mine : out_col - cc0 < n1_mine;
          if (active && mine) {
            f32x16 acc[kNT];
            multiply_block<kSteps, kPieces>(a_lds[buf], gc_lds[buf], b, acc, col, h);
            // ---- log-sum-exp epilogue and LDS-staged, coalesced score stores: as in score_tile
            float mx[kNT], sum[kNT];                         // mx stays in accumulator units (× S) until the pdf's last block
#pragma unroll
            for (int n = 0; n < kNT; n++) { const Lse l = block_lse(acc[n], h, l2e_s); mx[n] = l.m; sum[n] = l.s; }
            if (!(ecol & kFirst)) {
              // online log-sum-exp: fold this block's (max, sum) into the pdf's running pair
#pragma unroll
              for (int n = 0; n < kNT; n++) {
                lse_merge(mx_run[n], sum_run[n], mx[n], sum[n], l2e_s);
                mx[n] = mx_run[n]; sum[n] = sum_run[n];
              }
            }
#pragma unroll
            for (int n = 0; n < kNT; n++) { mx_run[n] = mx[n]; sum_run[n] = sum[n]; }
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
  });
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
  using Ops = SplitOps<kPieces>;
  using op8 = typename Ops::op8;
  constexpr bool kHalf = Ops::kHalf;
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
  // This kernel spells out three pieces its two siblings take from the head of this file — the item walk
  // (for_each_dense_item), the reachable prefix (reachable_prefix) and the decline (decline_tile): calling them moves
  // instructions in its <5, 2> and <6, 2> instantiations, the dense path's hot ones.  Change them together.
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
          n_single = max(n_single, prefix_end(__ballot(ff <= t_last), i0));   // (a superset for grouped plans: see reachable_prefix)
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
        const SplitSource src_ = split_source<kHalf>(p);
        const uint4 *wsrc = src_.w;
        const float *gsrc = src_.gc;
        const float inv_s = src_.inv_s, l2e_s = src_.l2e_s;
        // block copy global → LDS without a register stop (gptr_t, lptr_t, copies_landed above)
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
          flush_staged(stage, out, P, t_base, T, jdone - jj, jj + 1, col, h);
        };
        for (int c0 = 0; c0 < n_single; c0 += kBlkCache) {
        const int c1 = min(n_single, c0 + kBlkCache);
        __syncthreads();                                   // previous chunk's table is no longer read
        for (int i = c0 + threadIdx.x; i < c1; i += 256) blk_lds[i - c0] = p.row0[list[i]] >> 5;
        __syncthreads();
        auto block_of = [&](int jj) { return blk_lds[min(jj, c1 - 1) - c0]; };
        fetch(block_of(c0), 0);
        copies_landed();
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
            const f32x16 init = init_from_gconst(gc_lds[buf], h);
            const int column = j == 0 ? 32 : ((j - 1) & 31); // the first block of an item has no predecessor: padding column
            // operand pieces of step s+1 are read from LDS while step s is multiplied
            auto read_a = [&](int s, op8 (&a)[kPieces]) {
#pragma unroll
              for (int qq = 0; qq < kPieces; qq++)
                a[qq] = __builtin_bit_cast(op8, a_lds[buf][((s * kPieces + qq) * 2 + h) * 32 + col]);
            };
            op8 a_cur[kPieces], a_nxt[kPieces];
            read_a(0, a_cur);
            // one epilogue chunk of block j-1 behind every kStride-th MFMA of block j, each pinned in program order
            constexpr int kStride = (kSteps * Ops::kProd * kNT) / 30;   // MFMA slots per epilogue chunk
#pragma unroll
            for (int s = 0; s < kSteps; s++) {
              if (s + 1 < kSteps) read_a(s + 1, a_nxt);
              Ops::mfma_step(a_cur, b, cur, init, s, [&](int t6, int n) {
                const int slot = (s * Ops::kProd + t6) * kNT + n;
                if (slot % kStride == 0 && slot / kStride < kChunks) epi(slot / kStride, prev, column);
                __builtin_amdgcn_sched_barrier(0);
              });
#pragma unroll
              for (int qq = 0; qq < kPieces; qq++) a_cur[qq] = a_nxt[qq];
            }
          }
          copies_landed();
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
  using Ops = SplitOps<kPieces>;
  using op8 = typename Ops::op8;
  constexpr bool kHalf = Ops::kHalf;
  constexpr int kUnits = kSteps * kPieces * 2 * 32;    // 16-byte units per block
  constexpr int kLoads = (kUnits + 255) / 256;         // units each thread moves per block
  const int wave = threadIdx.x >> 6;
  __shared__ float stage_all[kWaves][64 * 33];
  __shared__ uint4 a_lds[2][kUnits];
  __shared__ __attribute__((aligned(16))) float gc_lds[2][64];
  constexpr int kPdfs = 32 / kSlot;                   // pdfs per virtual block = score columns per block
  constexpr int kCls = kSlot == 16 ? 2 : kSlot == 8 ? 3 : 4;   // position of this class in class_counts
  constexpr int kBlkCache = 1024;                     // pdf → first model row, staged per item (two dependent global loads
  __shared__ int blk_lds[kBlkCache];                  // per pdf must not sit in the block loop); a multiple of 32 pdfs
  __shared__ int s_item;
  float *stage = stage_all[wave];
  for_each_dense_item<kHalf>(p, s_item, [&](const DenseItem &it, int lane) {
      const int col = lane & 31, h = lane >> 5;
      const int utt = it.utt, tl = it.tl, T = it.T, t_base = it.t_base, P = it.P;
      const int64_t f0 = it.f0, l0 = it.l0;
      const bool active = it.active;
      const int32_t *list = it.list;
      float *out = it.out;
      const int32_t *cc6 = p.class_counts + (size_t)utt * 6;
      int base = cc6[0] + cc6[1];                      // columns of the classes in front of this one
#pragma unroll
      for (int q3 = 2; q3 < kCls; q3++) base += cc6[q3];
      const int n_all = cc6[kCls];
      if (n_all == 0) return;                          // uniform
      // n_single: pdfs the tile's LAST frame can be asked for — the prefix the workgroup walks together (block copies and
      // barriers are collective).  n_mine: the shorter prefix this wavefront's own 64 frames can be asked for; beyond it
      // the wavefront only helps with the copies.
      int n_single = n_all, n_mine = n_all;
      if (p.first_frame) {
        const int2 pre = reachable_prefix(p.first_frame + l0 + base, n_all, min(T, (tl + 1) * kFramesPerTile) - 1,
                                          min(T, t_base + kFramesPerWave) - 1, lane);
        n_single = pre.x; n_mine = pre.y;
      }
      if (n_single > 0) {
        // ---- x̃ = [x, x²] of this wavefront's 64 frames, split into bf16 triples: b[tile][step][piece], lane (frame, half)
        op8 b[kNT][kSteps][kPieces];
        // kHalf: `bad` = a scaled feature outside the f16 range (or NaN)
        const bool bad = split_features<kSteps, kPieces>(p, f0, T, t_base, col, h, b);
        if constexpr (kHalf) {
          if (decline_tile(p, utt, tl, bad)) return;      // uniform: the whole tile goes to the bf16×3 pass
        }
        const SplitSource src_ = split_source<kHalf>(p);
        const uint4 *wsrc = src_.w;
        const float *gsrc = src_.gc;
        const float inv_s = src_.inv_s, l2e_s = src_.l2e_s;
        // block copy global → LDS without a register stop (gptr_t, lptr_t, copies_landed above)
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
        // ---- block loop: multiply, reduce per pdf, stage one column per pdf, flush every 32 columns
        const int nb_mine = (n_mine + kPdfs - 1) / kPdfs;   // virtual blocks this wavefront multiplies
        auto flush = [&](int col_last) {                     // columns [col_last − col_last%32, col_last] → HBM
          const int jj = col_last & 31, j0 = col_last - jj;
          flush_staged(stage, out, P, t_base, T, base + j0, min(jj + 1, n_mine - j0), col, h);
        };
        int pending = -1;                                  // last column of a staged window waiting to be written out
        for (int c0 = 0; c0 < n_single; c0 += kBlkCache) {
        const int c1 = min(n_single, c0 + kBlkCache);
        __syncthreads();                                   // previous chunk's table is no longer read
        for (int i = c0 + threadIdx.x; i < c1; i += 256) blk_lds[i - c0] = p.row0[list[base + i]];
        __syncthreads();
        const int jb0 = c0 / kPdfs, jb1 = (c1 + kPdfs - 1) / kPdfs;
        fetch(jb0, 0, c0, c1);
        copies_landed();
        __syncthreads();
        for (int jb = jb0; jb < jb1; jb++) {
          const int buf = (jb - jb0) & 1;
          if (pending >= 0) { flush(pending); pending = -1; }   // a block early: see "score stores" in gmm_split_single_kernel
          fetch(min(jb + 1, jb1 - 1), buf ^ 1, c0, c1);
          if (active && jb < nb_mine) {
            f32x16 acc[kNT];
            multiply_block<kSteps, kPieces>(a_lds[buf], gc_lds[buf], b, acc, col, h);
            // ---- per-pdf log-sum-exp
            small_slot_scores<kSlot>(acc, stage, col, (jb * kPdfs) & 31, h, inv_s, l2e_s);
            const int col_last = min((jb + 1) * kPdfs, n_mine) - 1;   // last valid column this block produced
            if ((col_last & 31) == 31 || jb == nb_mine - 1) pending = col_last;
          }
          copies_landed();
          __syncthreads();                                 // block jb+1 is in place; everybody is done with block jb
        }
        }
        if (pending >= 0) flush(pending);
      }
  });
}

}  // namespace
