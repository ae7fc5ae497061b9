// The diagonal-UBM stage on gfx950: Gaussian selection (Kaldi gmm-gselect = DiagGmm::GaussianSelection) and the global GMM
// statistics over the selected Gaussians (gmm-global-acc-stats --gselect = AccumDiagGmm::AccumulateFromDiag), what the
// reference's DubmTrainer runs per job (MFA/ivector/trainer.py:105-388, ivector/multiprocessing.py:64-140, :233-280).
// Arithmetic contract: include/mfa_hip.h "Diagonal UBM"; the shared arithmetic: ubm_math.hpp and gmm_acc_math.hpp; the host
// twins: ubm_host.cpp.  The model comes with every call as three device arrays: no context state.
//
//   prepare  ubm_half_kernel: −½·inv_vars, the second weight row of the log-likelihood chain, to the workspace
//   select   ubm_gselect_kernel, one workgroup per tile of kTile frames: Gaussians in rounds of 64, lane = Gaussian, the round's
//            weights in LDS as [k][Gaussian] (ubm_score_tile); a wavefront owns kF frames and keeps each frame's sorted best
//            list in one 64-bit register per lane; the [frames][G] log-likelihoods exist in registers only
//   post     ubm_post_sparse_kernel (a wavefront per frame, lane = list entry) or ubm_post_dense_kernel (ubm_score_tile again,
//            the log-likelihoods parked in the γ scratch between the sweeps): γ, the frame's log-likelihood and weight
//   sums     ubm_sum_kernel, grid (slab of kSlab frames × block of 64 Gaussians): per tile of frames the γ are scattered into a
//            zeroed dense LDS tile [frame][Gaussian], the A operand of the f64 matrix instruction; B is the frame's row
//            (x | x·x | 1) in double, so occ comes with the ones column; the slab's partial to the workspace
//   reduce   ubm_reduce_kernel: the caller's value, then the slabs' partials in slab order; ubm_totals_kernel: the same for
//            the two totals
// The slabs of a batch run in passes sized to the workspace; the slab order makes the result independent of the passes.
#include <algorithm>

#include "acc_segments.hpp"
#include "ctx.hpp"
#include "ubm_math.hpp"

namespace {

constexpr int kTile = 64;                  // frames staged in LDS at a time by the scoring kernels
constexpr int kF = kTile / 4;              // … of which a wavefront owns 16
constexpr int kXStride = kUbmMaxDim + 1;
constexpr int kWStride = 65;               // a weight row holds 64 Gaussians; odd: the transposing store is conflict free
constexpr int kSlab = 2048;                // frames of the batch per partial (mfa_ubm_acc_slab_frames)
constexpr int kSumTile = 64;               // frames per dense γ tile of the sum kernel: 16 steps of the instruction's K = 4
constexpr int kGaussBlock = 64;            // Gaussians of a sum workgroup: 16 per wavefront
constexpr int kMaxColBlocks = (2 * kUbmMaxDim + 1 + 15) / 16;   // 16-wide blocks of the row (x | x·x | 1): 7
constexpr size_t kPassBytes = (size_t)96 << 20;                 // what a pass's partials and γ scratch may take of the workspace
static_assert(kSlab % kSumTile == 0 && kSumTile % 4 == 0 && kTile == 4 * kF, "ubm tiling");

typedef double double4_t __attribute__((ext_vector_type(4)));

struct Model {
  const float *gc, *mi, *half;   // gconsts [G], means_invvars [G][D], −½·inv_vars [G][D]
  int G, D;
};

__global__ __launch_bounds__(256) void ubm_half_kernel(const float *inv_vars, int n, float *half) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) half[i] = ubm_half_inv_var(inv_vars[i]);
}

// The tile of nc <= kTile frames at t0 against every Gaussian, a round of 64 at a time: fn(round, ll) gets, in every
// wavefront, ll[f] = the log-likelihood of Gaussian 64·round + lane on the wavefront's frame f (gmm_acc_loglike_block: the
// contract's chain).  Lanes past G and frames past nc compute on zeros: the caller leaves them out.  The whole workgroup
// calls it.
template <typename Fn>
__device__ __forceinline__ void ubm_score_tile(const Model &m, const float *feats, int64_t t0, int nc, float (&x_s)[kTile][kXStride],
                                               float (&w_s)[2 * kUbmMaxDim][kWStride], int tid, Fn fn) {
  const int D = m.D, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                                   // the previous tile's readers are done
  for (int i = tid; i < kTile * kUbmMaxDim; i += 256) {
    const int f = i / kUbmMaxDim, k = i - f * kUbmMaxDim;
    x_s[f][k] = f < nc && k < D ? feats[(size_t)(t0 + f) * D + k] : 0.0f;
  }
  const int rounds = (m.G + 63) >> 6;
  for (int rnd = 0; rnd < rounds; rnd++) {
    __syncthreads();                                 // the rows are staged; the previous round's readers are done
    for (int i = tid; i < 64 * D; i += 256) {
      const int gl = i / D, k = i - gl * D, g = 64 * rnd + gl;
      const bool in = g < m.G;
      w_s[k][gl] = in ? m.mi[(size_t)g * D + k] : 0.0f;
      w_s[D + k][gl] = in ? m.half[(size_t)g * D + k] : 0.0f;
    }
    __syncthreads();
    const int g = 64 * rnd + lane;
    float ll[kF];
    gmm_acc_loglike_block<kF>(g < m.G ? m.gc[g] : 0.0f, D, &w_s[0][lane], kWStride, &w_s[D][lane], kWStride, x_s[wave * kF],
                              kXStride, ll);
    fn(rnd, ll);
  }
}

// grid: the tiles of the batch.  A frame's list: lane j holds the j-th largest key met so far (0: none yet), all 64 lanes
// sorted; the first n are the answer.  A round's keys are tested against the n-th best with one ballot; the few that pass
// are inserted one at a time: its position is the number of larger entries, the entries from there on move up a lane.
__global__ __launch_bounds__(256) void ubm_gselect_kernel(Model m, const float *feats, int64_t T, int n, int32_t *gselect,
                                                          float *loglike) {
  __shared__ float x_s[kTile][kXStride];
  __shared__ float w_s[2 * kUbmMaxDim][kWStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * kTile;
  const int nc = (int)min((int64_t)kTile, T - t0);
  uint64_t list[kF];
#pragma unroll
  for (int f = 0; f < kF; f++) list[f] = 0;
  ubm_score_tile(m, feats, t0, nc, x_s, w_s, tid, [&](int rnd, const float (&ll)[kF]) {
    const int g = 64 * rnd + lane;
    const bool have = g < m.G;
#pragma unroll
    for (int f = 0; f < kF; f++) {
      if (wave * kF + f >= nc) continue;             // the same for the whole wavefront
      const uint64_t key = have ? ubm_key(ll[f], g) : 0;
      uint64_t cur = list[f];
      uint64_t thr = __shfl(cur, n - 1);
      uint64_t mask = __ballot(key > thr);
      while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t k = __shfl(key, l);
        if (k > thr) {
          const int pos = __popcll(__ballot(cur > k));
          const uint64_t up = __shfl_up(cur, 1);
          cur = lane < pos ? cur : (lane == pos ? k : up);
          thr = __shfl(cur, n - 1);
        }
      }
      list[f] = cur;
    }
  });
#pragma unroll
  for (int f = 0; f < kF; f++) {
    const int t = wave * kF + f;
    if (t >= nc) continue;
    const uint64_t key = list[f];
    if (lane < n) gselect[(size_t)(t0 + t) * n + lane] = ubm_key_index(key);
    if (loglike) {
      const float mx = ubm_key_loglike(__shfl(key, 0));
      float sum = lane < n ? expf(ubm_key_loglike(key) - mx) : 0.0f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      if (lane == 0) loglike[t0 + t] = gmm_acc_frame_loglike(mx, sum);
    }
  }
}

// What the posterior kernels leave for a pass over frames [f0, f1): γ at post[(t − post_base)·stride + j], and per frame
// fll[t − f0] = its log-likelihood, fw[t − f0] = its weight, 0 if it takes no part.
struct PostParams {
  Model m;
  const float *feats; int64_t f0, f1;
  int n; const int32_t *gselect; const float *fweight;
  float *post; int64_t post_base;
  float *fll, *fw;
};

// grid: 4 frames a workgroup, a wavefront each; lane j = entry j of the frame's list.
__global__ __launch_bounds__(256) void ubm_post_sparse_kernel(PostParams p) {
  __shared__ float x_s[4][kXStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = p.m.D, n = p.n;
  const int64_t t = p.f0 + (int64_t)blockIdx.x * 4 + wave;
  const bool live = t < p.f1;
  if (lane < kUbmMaxDim) x_s[wave][lane] = live && lane < D ? p.feats[(size_t)t * D + lane] : 0.0f;
  __syncthreads();
  if (!live) return;
  const int g = lane < n ? p.gselect[(size_t)t * n + lane] : -1;
  const bool valid = g >= 0 && g < p.m.G;
  const float w = p.fweight ? p.fweight[t] : 1.0f;
  const float ll = valid ? gmm_acc_loglike(p.m.gc[g], D, p.m.mi + (size_t)g * D, 1, p.m.half + (size_t)g * D, 1, x_s[wave]) : -INFINITY;
  const bool part = __ballot(valid) != 0 && w != 0.0f;
  float mx = ll;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  const float e = valid ? expf(ll - mx) : 0.0f;
  float sum = e;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane < n) p.post[(size_t)(t - p.post_base) * n + lane] = part && valid ? gmm_acc_posterior(e, 1.0f / sum, w) : 0.0f;
  if (lane == 0) {
    p.fll[t - p.f0] = part ? gmm_acc_frame_loglike(mx, sum) : 0.0f;
    p.fw[t - p.f0] = part ? w : 0.0f;
  }
}

// grid: the tiles of the pass; every Gaussian takes part.  Three sweeps over the frame's row of the γ scratch, each lane over
// the entries it wrote itself: the log-likelihoods (with the running maximum), the shifted exponentials (with their sum), γ.
__global__ __launch_bounds__(256) void ubm_post_dense_kernel(PostParams p) {
  __shared__ float x_s[kTile][kXStride];
  __shared__ float w_s[2 * kUbmMaxDim][kWStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = p.m.G;
  const int64_t t0 = p.f0 + (int64_t)blockIdx.x * kTile;
  const int nc = (int)min((int64_t)kTile, p.f1 - t0);
  float mx[kF];
#pragma unroll
  for (int f = 0; f < kF; f++) mx[f] = -INFINITY;
  float *row0 = p.post + (size_t)(t0 + wave * kF - p.post_base) * G;   // the wavefront's first frame
  ubm_score_tile(p.m, p.feats, t0, nc, x_s, w_s, tid, [&](int rnd, const float (&ll)[kF]) {
    const int g = 64 * rnd + lane;
    if (g >= G) return;
#pragma unroll
    for (int f = 0; f < kF; f++) {
      if (wave * kF + f >= nc) continue;
      row0[(size_t)f * G + g] = ll[f];
      mx[f] = fmaxf(mx[f], ll[f]);
    }
  });
  const int rounds = (G + 63) >> 6;
  for (int f = 0; f < kF; f++) {
    const int tl = wave * kF + f;
    if (tl >= nc) break;                             // the same for the whole wavefront
    const int64_t t = t0 + tl;
    float *row = row0 + (size_t)f * G;
    float m = mx[f];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.0f;
    for (int rnd = 0; rnd < rounds; rnd++) {
      const int g = 64 * rnd + lane;
      if (g < G) { const float e = expf(row[g] - m); row[g] = e; sum += e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float w = p.fweight ? p.fweight[t] : 1.0f, inv = 1.0f / sum;
    const bool part = w != 0.0f;
    for (int rnd = 0; rnd < rounds; rnd++) {
      const int g = 64 * rnd + lane;
      if (g < G) row[g] = part ? gmm_acc_posterior(row[g], inv, w) : 0.0f;
    }
    if (lane == 0) {
      p.fll[t - p.f0] = part ? gmm_acc_frame_loglike(m, sum) : 0.0f;
      p.fw[t - p.f0] = part ? w : 0.0f;
    }
  }
}

struct SumParams {
  const float *feats; int64_t f0, f1;
  int D, G, n;                     // n: entries of a frame's list; 0: the γ scratch is dense, [frame][G]
  const int32_t *gselect; const float *post; int64_t post_base;
  int ncb;                         // 16-wide blocks of the row (x | x·x | 1)
  double *partial;                 // per slab of the pass [G][16·ncb]
};

// grid: (slabs of the pass, blocks of kGaussBlock Gaussians); 256 threads, a wavefront owns 16 Gaussians and all column blocks.
// A step of the instruction takes 4 frames: lane l gives A[i = l & 15][k = l >> 4] = γ of frame k for the wavefront's Gaussian
// i (float to double: exact) and B[k = l >> 4][j = l & 15] = column j of the block of frame k's row (x | x·x | 1), the square
// formed in double.  Frames past the slab and columns past the row are zero operands; a feature that is not finite enters
// as 0, so that it stays with the Gaussians whose γ it has already made NaN.  A step whose 64 γ are all zero adds exact
// zeros and is left out.  Result layout of the f64 instruction: register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15].
__global__ __launch_bounds__(256) void ubm_sum_kernel(SumParams p) {
  __shared__ float P[kSumTile][kGaussBlock + 1];
  __shared__ float X[kSumTile][kXStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int D = p.D, G = p.G, n = p.n;
  const int gb0 = blockIdx.y * kGaussBlock;
  const int64_t s0 = p.f0 + (int64_t)blockIdx.x * kSlab, s1 = min(p.f1, s0 + kSlab);
  const bool wave_has = gb0 + wave * 16 < G;
  double4_t acc[kMaxColBlocks];
#pragma unroll
  for (int cb = 0; cb < kMaxColBlocks; cb++) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};

  for (int64_t t0 = s0; t0 < s1; t0 += kSumTile) {
    const int nf = (int)min((int64_t)kSumTile, s1 - t0);
    __syncthreads();                                 // the previous tile's readers are done
    for (int i = tid; i < kSumTile * kUbmMaxDim; i += 256) {
      const int f = i / kUbmMaxDim, k = i - f * kUbmMaxDim;
      const float v = f < nf && k < D ? p.feats[(size_t)(t0 + f) * D + k] : 0.0f;
      X[f][k] = isfinite(v) ? v : 0.0f;
    }
    if (n > 0) {
      for (int i = tid; i < kSumTile * kGaussBlock; i += 256) P[i >> 6][i & 63] = 0.0f;
      __syncthreads();
      for (int i = tid; i < nf * n; i += 256) {      // the tile's list entries, flat: consecutive in memory
        const size_t at = (size_t)t0 * n + i;
        const int g = p.gselect[at] - gb0;
        if (g >= 0 && g < kGaussBlock && g + gb0 < G) P[i / n][g] = p.post[at - (size_t)p.post_base * n];
      }
    } else {
      for (int i = tid; i < kSumTile * kGaussBlock; i += 256) {
        const int f = i >> 6, g = gb0 + (i & 63);
        P[f][i & 63] = f < nf && g < G ? p.post[(size_t)(t0 + f - p.post_base) * G + g] : 0.0f;
      }
    }
    __syncthreads();
    if (wave_has) {
      for (int r = 0; r < nf; r += 4) {
        const double a = (double)P[r + lk][wave * 16 + lc];
        if (__ballot(a != 0.0) == 0) continue;
        const float *xr = X[r + lk];
#pragma unroll
        for (int cb = 0; cb < kMaxColBlocks; cb++) {
          if (cb < p.ncb) {
            const int col = cb * 16 + lc;
            const double xv = (double)xr[col < D ? col : (col < 2 * D ? col - D : 0)];
            const double b = col < D ? xv : (col < 2 * D ? xv * xv : (col == 2 * D ? 1.0 : 0.0));
            acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[cb], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!wave_has) return;
  const int ncols = 16 * p.ncb;
  double *out = p.partial + (size_t)blockIdx.x * G * ncols;
#pragma unroll
  for (int cb = 0; cb < kMaxColBlocks; cb++) {
    if (cb < p.ncb) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int g = gb0 + wave * 16 + lk + 4 * r;
        if (g < G) out[(size_t)g * ncols + cb * 16 + lc] = acc[cb][r];
      }
    }
  }
}

// One thread per (Gaussian, column of its row): the caller's value, then the pass's slab partials in slab order.  A partial
// that is zero is not added: the sum's bits are the same, and a Gaussian that no frame selected keeps the caller's bits
// whatever they are.
__global__ __launch_bounds__(256) void ubm_reduce_kernel(const double *partial, int n_slabs, int G, int D, int ncols, double *occ,
                                                         double *mean, double *var) {
  const int row = 2 * D + 1;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= G * row) return;
  const int g = e / row, col = e - g * row;
  double *dst = col < D ? mean + (size_t)g * D + col : (col < 2 * D ? var + (size_t)g * D + (col - D) : occ + g);
  const double *src = partial + (size_t)g * ncols + col;
  const size_t stride = (size_t)G * ncols;
  double a = *dst;
  for (int s = 0; s < n_slabs; s++) {
    const double v = src[s * stride];
    if (v != 0.0) a += v;
  }
  *dst = a;
}

// One workgroup: thread s sums slab s of the pass from zero in frame order (gmm_acc_total), then thread 0 adds the slabs'
// totals in slab order onto the caller's two.
__global__ __launch_bounds__(256) void ubm_totals_kernel(const float *fll, const float *fw, int64_t frames, double *tot) {
  __shared__ double s[256][2];
  const int n_slabs = (int)((frames + kSlab - 1) / kSlab);
  double a = 0.0, b = 0.0;
  if (threadIdx.x == 0) { a = tot[0]; b = tot[1]; }
  for (int u0 = 0; u0 < n_slabs; u0 += 256) {
    __syncthreads();
    const int u = u0 + threadIdx.x;
    if (u < n_slabs) {
      double x = 0.0, y = 0.0;
      const int64_t e = min(frames, (int64_t)(u + 1) * kSlab);
      for (int64_t t = (int64_t)u * kSlab; t < e; t++)
        if (fw[t] != 0.0f) gmm_acc_total(fw[t], fll[t], x, y);
      s[threadIdx.x][0] = x; s[threadIdx.x][1] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < min(256, n_slabs - u0); i++)
        if (s[i][0] != 0.0 || s[i][1] != 0.0) { a += s[i][0]; b += s[i][1]; }
  }
  if (threadIdx.x == 0) { tot[0] = a; tot[1] = b; }
}

int refuse_shape(mfa_ctx *c, const char *who, int rc, int32_t dim, int32_t G, int64_t total_frames) {
  switch (rc) {
    case -2: return c->fail("%s: feature dim %d > %d (columns of a staged row)", who, dim, kUbmMaxDim);
    case -3: return c->fail("%s: %d Gaussians (1 to %d: 32 rounds of lane = Gaussian)", who, G, kUbmMaxGauss);
    case -5: return c->fail("%s: %lld frames in one call (fewer than 2^31)", who, (long long)total_frames);
    default: return c->fail("%s: feature dim %d, %lld frames", who, dim, (long long)total_frames);
  }
}

// Slabs per pass: what kPassBytes holds; MFA_UBM_PASS_SLABS=<slabs> overrides (tests: 1 makes every slab a pass).  Read at
// every call, as MFA_LIST_GRID is.
size_t pass_slabs(size_t bytes_per_slab, size_t n_slabs) {
  const char *e = getenv("MFA_UBM_PASS_SLABS");
  const long forced = e ? atol(e) : 0;
  const size_t fit = forced > 0 ? (size_t)forced : std::max<size_t>(1, kPassBytes / bytes_per_slab);
  return std::min(fit, n_slabs);
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_ubm_acc_slab_frames(void) { return kSlab; }
MFA_API int32_t mfa_ubm_gselect_tile_frames(void) { return kTile; }

MFA_API int mfa_ubm_gselect_batch(mfa_ctx *c, const float *d_feats, int64_t total_frames, int32_t dim, int32_t G,
                                  const float *d_gconsts, const float *d_means_invvars, const float *d_inv_vars, int32_t num_gselect,
                                  int32_t *d_gselect, float *d_loglike) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "Gaussian selection";
  const int rc = ubm_check_shape(dim, G, total_frames);
  if (rc) return refuse_shape(c, who, rc, dim, G, total_frames);
  if (num_gselect <= 0 || std::min(num_gselect, G) > kUbmMaxSelect)
    return c->fail("%s: %d Gaussians per frame (1 to %d: a frame's list is one wavefront register)", who, num_gselect, kUbmMaxSelect);
  if (total_frames == 0) return 0;
  if (!d_feats || !d_gconsts || !d_means_invvars || !d_inv_vars) return c->fail("%s: NULL input array", who);
  if (!d_gselect) return c->fail("%s: NULL output array", who);
  const int n = std::min(num_gselect, G);
  Workspace ws;
  const size_t o_half = ws.take((size_t)G * dim * 4);
  if (ws.reserve(c, "the Gaussian selection workspace")) return -1;
  float *half = ws.at<float>(o_half);
  KernelTimer kt(c, MFA_K_UBM_SELECT);
  hipLaunchKernelGGL(ubm_half_kernel, dim3((unsigned)((G * dim + 255) / 256)), dim3(256), 0, c->stream, d_inv_vars, G * dim, half);
  const Model m{d_gconsts, d_means_invvars, half, G, dim};
  hipLaunchKernelGGL(ubm_gselect_kernel, dim3((unsigned)((total_frames + kTile - 1) / kTile)), dim3(256), 0, c->stream, m, d_feats,
                     total_frames, n, d_gselect, d_loglike);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "ubm_gselect_kernel frames=%lld G=%d n=%d", (long long)total_frames, G, n);
  return 0;
}

MFA_API int mfa_ubm_acc_batch(mfa_ctx *c, const float *d_feats, int64_t total_frames, int32_t dim, int32_t G, const float *d_gconsts,
                              const float *d_means_invvars, const float *d_inv_vars, int32_t n, const int32_t *d_gselect,
                              const float *d_frame_weight, double *d_occ, double *d_mean, double *d_var, double *d_tot, float *d_post) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "UBM statistics";
  const int rc = ubm_check_shape(dim, G, total_frames);
  if (rc) return refuse_shape(c, who, rc, dim, G, total_frames);
  if (d_gselect && (n <= 0 || n > kUbmMaxSelect))
    return c->fail("%s: lists of %d Gaussians per frame (1 to %d: a frame's list is one wavefront)", who, n, kUbmMaxSelect);
  if (d_post && !d_gselect) return c->fail("%s: posteriors are written in the order of a selection: d_post needs d_gselect", who);
  if (total_frames == 0) return 0;
  if (!d_feats || !d_gconsts || !d_means_invvars || !d_inv_vars) return c->fail("%s: NULL input array", who);
  if (!d_occ || !d_mean || !d_var || !d_tot) return c->fail("%s: NULL accumulator", who);

  const bool sparse = d_gselect != nullptr;
  const int stride = sparse ? n : G, ncb = (2 * dim + 1 + 15) / 16, ncols = 16 * ncb;
  const size_t n_slabs = ((size_t)total_frames + kSlab - 1) / kSlab;
  const size_t partial_bytes = (size_t)G * ncols * 8, scratch_bytes = d_post ? 0 : (size_t)kSlab * stride * 4;
  const size_t per_pass = pass_slabs(partial_bytes + scratch_bytes, n_slabs);
  Workspace ws;
  const size_t o_half = ws.take((size_t)G * dim * 4), o_part = ws.take(per_pass * partial_bytes),
               o_post = ws.take(per_pass * scratch_bytes), o_fll = ws.take(per_pass * kSlab * 4), o_fw = ws.take(per_pass * kSlab * 4);
  if (ws.reserve(c, "the UBM statistics workspace")) return -1;
  float *half = ws.at<float>(o_half), *fll = ws.at<float>(o_fll), *fw = ws.at<float>(o_fw);
  double *partial = ws.at<double>(o_part);
  hipLaunchKernelGGL(ubm_half_kernel, dim3((unsigned)((G * dim + 255) / 256)), dim3(256), 0, c->stream, d_inv_vars, G * dim, half);
  const Model m{d_gconsts, d_means_invvars, half, G, dim};

  for (size_t slab0 = 0; slab0 < n_slabs; slab0 += per_pass) {
    const size_t slabs = std::min(per_pass, n_slabs - slab0);
    const int64_t f0 = (int64_t)(slab0 * kSlab), f1 = std::min(total_frames, f0 + (int64_t)(slabs * kSlab)), frames = f1 - f0;
    float *post = d_post ? d_post : ws.at<float>(o_post);
    const int64_t post_base = d_post ? 0 : f0;
    {
      KernelTimer kt(c, MFA_K_UBM_POST);
      const PostParams pp{m, d_feats, f0, f1, n, d_gselect, d_frame_weight, post, post_base, fll, fw};
      if (sparse) hipLaunchKernelGGL(ubm_post_sparse_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, c->stream, pp);
      else hipLaunchKernelGGL(ubm_post_dense_kernel, dim3((unsigned)((frames + kTile - 1) / kTile)), dim3(256), 0, c->stream, pp);
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "ubm_post kernel frames=[%lld, %lld) G=%d n=%d", (long long)f0, (long long)f1, G, sparse ? n : 0);
    }
    {
      KernelTimer kt(c, MFA_K_UBM_SUMS);
      const SumParams sp{d_feats, f0, f1, dim, G, sparse ? n : 0, d_gselect, post, post_base, ncb, partial};
      hipLaunchKernelGGL(ubm_sum_kernel, dim3((unsigned)slabs, (unsigned)((G + kGaussBlock - 1) / kGaussBlock)), dim3(256), 0, c->stream, sp);
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "ubm_sum_kernel slabs=%zu", slabs);
    }
    {
      KernelTimer kt(c, MFA_K_UBM_REDUCE);
      hipLaunchKernelGGL(ubm_reduce_kernel, dim3((unsigned)((G * (2 * dim + 1) + 255) / 256)), dim3(256), 0, c->stream, partial,
                         (int)slabs, G, dim, ncols, d_occ, d_mean, d_var);
      hipLaunchKernelGGL(ubm_totals_kernel, dim3(1), dim3(256), 0, c->stream, fll, fw, frames, d_tot);
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "ubm_reduce_kernel slabs=%zu", slabs);
    }
  }
  return 0;
}

}  // extern "C"
