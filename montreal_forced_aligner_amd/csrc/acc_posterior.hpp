// The posterior phase of the statistics kernels that weigh a frame by its Gaussians' posteriors: gmm_acc_kernel<false>,
// gmm_acc_kernel<true> (gmm_acc.hip) and mllt_acc_kernel (mllt_acc.hip: acc_posterior_phase, the rest written out there).
// All three run acc_posterior_phase, so γ has the same bits in every one of them.  The arithmetic is gmm_acc_math.hpp's.
// A workgroup of 256 threads works on a chunk of one pdf's segment of the sorted frame indices, a tile of kAccTile frames at a
// time.  The gather of a tile is two dependent global loads (sorted index, then the row): the next tile's rows are fetched
// into registers (acc_fetch) while this tile is worked on, and only stored to LDS (acc_stage_store) at the top of the next
// round.  Posterior phase (acc_posterior_phase): wavefront = 8 frames of the tile, lane = Gaussian (two rounds of 64), the
// weights of the round in LDS as [k][Gaussian].  The LDS arrays are the kernel's own and are passed by reference; the kernel
// keeps the __syncthreads() between the phases.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gmm_acc_math.hpp"
#include "gmm_pack.hpp"

constexpr int kAccTile = 32;        // frames staged in LDS at a time; 8 per wavefront in the posterior phase
constexpr int kAccMaxGauss = 128;   // two rounds of lane = Gaussian
constexpr int kAccMaxDim = 48;      // columns of a staged row; columns from the feature dim up to 48 read as 0
constexpr int kAccXStride = kAccMaxDim + 1;
constexpr int kAccStage = kAccTile * kAccMaxDim / 256;
static_assert(kAccTile == 4 * 8 && kAccMaxGauss == 2 * 64, "acc_posterior_phase tiling");
static_assert(kAccStage * 256 == kAccTile * kAccMaxDim, "every thread stages the same number of elements");

// The rows of the next tile, in registers.  kTwoFeats: also the same frames' rows of a second matrix.
template <bool kTwoFeats> struct AccStaged {
  float nx[kAccStage], nx2[kTwoFeats ? kAccStage : 1], nw = 0.0f;
};

// Rows [t0, min(t0 + kAccTile, s1)) of the sorted index; rows past the end read as 0.  feats_sum: read if kTwoFeats only.
template <bool kTwoFeats>
__device__ __forceinline__ void acc_fetch(AccStaged<kTwoFeats> &s, const float *feats, const float *feats_sum, const uint32_t *idx,
                                          const float *weight, int D, int t0, int s1, int tid) {
  const int nc = min(kAccTile, s1 - t0);
#pragma unroll
  for (int i = 0; i < kAccStage; i++) {
    const int e = tid + 256 * i, t = e / kAccMaxDim, k = e % kAccMaxDim;
    if constexpr (kTwoFeats) {
      const bool in = t < nc && k < D;
      const size_t at = in ? (size_t)idx[t0 + t] * D + k : 0;
      s.nx[i] = in ? feats[at] : 0.0f;
      s.nx2[i] = in ? feats_sum[at] : 0.0f;
    } else {
      s.nx[i] = t < nc && k < D ? feats[(size_t)idx[t0 + t] * D + k] : 0.0f;
    }
  }
  if (tid < kAccTile) s.nw = tid < nc ? weight[idx[t0 + tid]] : 0.0f;
}

// The fetched rows and weights to LDS.  x2_s: the second matrix's tile, used if kTwoFeats only.
template <bool kTwoFeats>
__device__ __forceinline__ void acc_stage_store(const AccStaged<kTwoFeats> &s, float (&x_s)[kAccTile][kAccXStride],
                                                float (*x2_s)[kAccXStride], float (&fw_s)[kAccTile], int tid) {
#pragma unroll
  for (int i = 0; i < kAccStage; i++) {
    const int e = tid + 256 * i;
    x_s[e / kAccMaxDim][e % kAccMaxDim] = s.nx[i];
    if constexpr (kTwoFeats) x2_s[e / kAccMaxDim][e % kAccMaxDim] = s.nx2[i];
  }
  if (tid < kAccTile) fw_s[tid] = s.nw;
}

// The gconsts of the lane's Gaussian of either round (rows r0.. of the packed model).
__device__ __forceinline__ void acc_gconsts(const float *gc, int r0, int ng, int lane, float (&gcv)[2]) {
#pragma unroll
  for (int rnd = 0; rnd < 2; rnd++) gcv[rnd] = lane + 64 * rnd < ng ? gc[r0 + lane + 64 * rnd] : 0.0f;
}

// The tile at sorted position t0 of the chunk that starts at s0, nc frames of it in use: from x_s and fw_s to post_s [frame]
// [Gaussian] = γ and fll_s [frame] = the frame's log-likelihood.  w, kpad: the packed model (gmm_pack.hpp layout), r0 the
// pdf's first row, ng its Gaussians.  The whole workgroup calls it; it synchronises the workgroup before it writes and after
// it has written a round's weights, not after its last write to post_s / fll_s.
// kZeroPastEnd: the rows of post_s from nc on are written as zeros (a kernel that reads whole steps of 4 frames).
template <bool kZeroPastEnd>
__device__ __forceinline__ void acc_posterior_phase(const float *w, int kpad, int r0, int ng, int D, const float (&gcv)[2], int t0,
                                                    int s0, int nc, const float (&x_s)[kAccTile][kAccXStride],
                                                    float (&w_s)[2 * kAccMaxDim][64], float (&post_s)[kAccTile][kAccMaxGauss],
                                                    const float (&fw_s)[kAccTile], float (&fll_s)[kAccTile], int tid, int lane, int wave,
                                                    int rounds) {
  float ll[8][2];
#pragma unroll
  for (int rnd = 0; rnd < 2; rnd++) {
    if (rnd < rounds) {
      if (rounds > 1 || t0 == s0) {   // one round: its weights stay for the whole chunk
        __syncthreads();              // the other round's readers are done
        for (int i = tid; i < 2 * D * 64; i += 256) {
          const int k = i >> 6, g = (i & 63) + 64 * rnd;
          w_s[k][i & 63] = g < ng ? w[mfa_packed_offset(r0 + g, k, kpad)] : 0.0f;
        }
      }
      __syncthreads();
      const bool have = lane + 64 * rnd < ng;
      float blk[8];                   // rows past the chunk's end are zeros: computed, never used
      gmm_acc_loglike_block<8>(gcv[rnd], D, &w_s[0][lane], 64, &w_s[D][lane], 64, x_s[wave * 8], kAccXStride, blk);
#pragma unroll
      for (int f = 0; f < 8; f++) ll[f][rnd] = have && wave * 8 + f < nc ? blk[f] : -INFINITY;
    } else {
#pragma unroll
      for (int f = 0; f < 8; f++) ll[f][rnd] = -INFINITY;
    }
  }
#pragma unroll
  for (int f = 0; f < 8; f++) {
    const int t = wave * 8 + f;
    if (t < nc) {                     // the same for the whole wavefront
      float mx = fmaxf(ll[f][0], ll[f][1]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      const float e0 = lane < ng ? expf(ll[f][0] - mx) : 0.0f, e1 = lane + 64 < ng ? expf(ll[f][1] - mx) : 0.0f;
      float sum = e0 + e1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      const float inv = 1.0f / sum, wgt = fw_s[t];
      post_s[t][lane] = gmm_acc_posterior(e0, inv, wgt);
      post_s[t][lane + 64] = gmm_acc_posterior(e1, inv, wgt);
      if (lane == 0) fll_s[t] = gmm_acc_frame_loglike(mx, sum);
    } else if constexpr (kZeroPastEnd) {
      post_s[t][lane] = 0.0f;
      post_s[t][lane + 64] = 0.0f;
    }
  }
}

// The tile's nc frames onto a Gaussian's occupancy (thread = Gaussian) and onto the two totals (thread 255), in frame order.
__device__ __forceinline__ void acc_occ_totals(const float (&post_s)[kAccTile][kAccMaxGauss], const float (&fw_s)[kAccTile],
                                               const float (&fll_s)[kAccTile], int nc, int tid, double &occ, double &tot_like,
                                               double &tot_count) {
  if (tid < kAccMaxGauss)
    for (int t = 0; t < nc; t++) occ += (double)post_s[t][tid];
  if (tid == 255)
    for (int t = 0; t < nc; t++) gmm_acc_total(fw_s[t], fll_s[t], tot_like, tot_count);
}

// One workgroup: the units' totals {Σ w·loglike, Σ w} in unit order onto the caller's two.  unit_base[P]: the number of units.
// (Not in acc_segments.hpp: a kernel in a header is compiled into every translation unit that includes it.)
static __global__ __launch_bounds__(256) void acc_totals_kernel(const double *unit_tot, const int32_t *unit_base, int P, double *tot) {
  __shared__ double s[256][2];
  const int n = unit_base[P];
  double a = 0.0, b = 0.0;
  if (threadIdx.x == 0) { a = tot[0]; b = tot[1]; }
  for (int u0 = 0; u0 < n; u0 += 256) {
    __syncthreads();
    const int u = u0 + threadIdx.x;
    if (u < n) { s[threadIdx.x][0] = unit_tot[2 * (size_t)u]; s[threadIdx.x][1] = unit_tot[2 * (size_t)u + 1]; }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < min(256, n - u0); i++) { a += s[i][0]; b += s[i][1]; }
  }
  if (threadIdx.x == 0 && n > 0) { tot[0] = a; tot[1] = b; }
}
