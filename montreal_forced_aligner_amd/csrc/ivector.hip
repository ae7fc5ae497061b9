// The i-vector extractor stage on gfx950: what the reference's IvectorTrainer runs per job (MFA/ivector/trainer.py:390-632,
// ivector/multiprocessing.py:143-231 and :283-331) and ExtractIvectorsFunction per utterance (MFA/corpus/features.py:956-1015):
// gauss-to-post's pruning, the utterance statistics and the extractor's E-step.  Restated from the algorithm (Kaldi's source
// is not among this project's references): parity unpinned, DESIGN §2.  Arithmetic contract: include/mfa_hip.h "I-vector
// extractor"; the shared arithmetic: ivector_math.hpp; the host twins: ivector_host.cpp.  The model comes with every call as
// device arrays: no context state.
//
//   prune    ivec_prune_kernel, a thread per frame: ivector_prune_frame, the twin's own function
//   stats    ivec_utt_kernel, grid (utterance × block of 64 Gaussians): ubm_sum_kernel's pattern with the slab replaced by the
//            utterance.  Per tile of 64 frames the (index, p) lists are scattered into a zeroed dense LDS tile
//            [frame][Gaussian], the A operand of the f64 matrix instruction; B is the frame's row (x | 1) in double, so γ
//            comes with the ones column.  Written straight to gamma[u] and X[u].  ivec_cap_kernel: max_count.
//            ivec_scatter_kernel, grid (slab of 2048 frames × block of 64 Gaussians × group of 64 packed columns): the same A
//            tile, B the products x_j·x_k formed in double (exact); the slab's partial to the workspace.
//            ivec_scatter_reduce_kernel: the caller's S, then the slabs' partials in slab order.
//   E-step   per chunk of utterances: f64_gemm_kernel (f64_gemm.hpp) twice (Q = I + γ·U, lin = prior + X·W), ivec_solve_kernel (a workgroup
//            per utterance, the packed triangle in LDS: Cholesky, L⁻¹ in place, μ, Var, Sc), f64_gemm_kernel twice more
//            (Rq += γᵀ·Sc, Y += Xᵀ·μ, the accumulator continued from the caller's value) and ivec_small_acc_kernel (Γ, isum,
//            iscat, n: a thread per element, the chunk's utterances in order).
// Every sum has a fixed order and no floating-point atomics: two calls on the same input give the same bits.
#include <algorithm>

#include "acc_segments.hpp"
#include "ctx.hpp"
#include "f64_gemm.hpp"
#include "ivector_math.hpp"

namespace {

constexpr int kTileF = 64;                 // frames per dense posterior tile: 16 steps of the instruction's K = 4
constexpr int kGaussBlock = 64;            // Gaussians of a statistics workgroup: 16 per wavefront
constexpr int kXStride = kIvecMaxDim + 1;
constexpr int kUttColBlocks = (kIvecMaxDim + 1 + 15) / 16;   // 16-wide blocks of the row (x | 1): 4
constexpr int kSlab = 2048;                // frames per partial of the scatter sums
constexpr int kScatBlocks = 4;             // 16-wide column blocks of a scatter workgroup: 64 packed columns
constexpr size_t kScatPassBytes = (size_t)96 << 20;
constexpr size_t kEstepPassBytes = (size_t)192 << 20;
static_assert(kSlab % kTileF == 0 && kTileF % 4 == 0, "ivector tiling");

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void ivec_prune_kernel(const float *in, int64_t T, int n, float min_post, float scale, float *out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < T) ivector_prune_frame(in + t * n, out + t * n, n, min_post, scale);
}

// Frames [t0, t0 + nf) of the batch, nf <= kTileF: the feature rows (a value that is not finite as 0) and the dense
// posterior tile of the workgroup's Gaussians [gb0, gb0 + 64).  The whole workgroup calls it.
__device__ __forceinline__ void ivec_stage_tile(const float *feats, const int32_t *gselect, const float *post, int64_t t0, int nf, int D,
                                                int G, int n, int gb0, float (&Pt)[kTileF][kGaussBlock + 1], float (&X)[kTileF][kXStride],
                                                int tid) {
  __syncthreads();                                   // the previous tile's readers are done
  for (int i = tid; i < kTileF * kIvecMaxDim; i += 256) {
    const int f = i / kIvecMaxDim, k = i - f * kIvecMaxDim;
    const float v = f < nf && k < D ? feats[(size_t)(t0 + f) * D + k] : 0.0f;
    X[f][k] = isfinite(v) ? v : 0.0f;
  }
  for (int i = tid; i < kTileF * kGaussBlock; i += 256) Pt[i >> 6][i & 63] = 0.0f;
  __syncthreads();
  for (int i = tid; i < nf * n; i += 256) {          // the tile's list entries, flat: consecutive in memory
    const size_t at = (size_t)t0 * n + i;
    const int g = gselect[at] - gb0;
    if (g >= 0 && g < kGaussBlock && g + gb0 < G) Pt[i / n][g] = post[at];
  }
  __syncthreads();
}

// grid (utterances, blocks of 64 Gaussians); a wavefront owns 16 Gaussians.  Lane l of a step gives A[i = l & 15][k = l >> 4]
// = p of frame k for Gaussian i and B[k][j = l & 15] = column j of frame k's row (x | 1).  Register r of lane l is
// D[row = (l >> 4) + 4 r][col = l & 15].
__global__ __launch_bounds__(256) void ivec_utt_kernel(const float *feats, const int64_t *frame_off, int64_t T, int D, int G, int n,
                                                       const int32_t *gselect, const float *post, double *gamma, double *Xout) {
  __shared__ float Pt[kTileF][kGaussBlock + 1];
  __shared__ float X[kTileF][kXStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int u = blockIdx.x, gb0 = blockIdx.y * kGaussBlock;
  const int64_t s0 = max((int64_t)0, frame_off[u]), s1 = min(T, frame_off[u + 1]);   // offsets past the batch read nothing
  const bool wave_has = gb0 + wave * 16 < G;
  const int ncb = (D + 1 + 15) / 16;
  double4_t acc[kUttColBlocks];
#pragma unroll
  for (int cb = 0; cb < kUttColBlocks; cb++) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int64_t t0 = s0; t0 < s1; t0 += kTileF) {
    const int nf = (int)min((int64_t)kTileF, s1 - t0);
    ivec_stage_tile(feats, gselect, post, t0, nf, D, G, n, gb0, Pt, X, tid);
    if (!wave_has) continue;
    for (int r = 0; r < nf; r += 4) {
      const double a = (double)Pt[r + lk][wave * 16 + lc];
      if (__ballot(a != 0.0) == 0) continue;
      const float *xr = X[r + lk];
#pragma unroll
      for (int cb = 0; cb < kUttColBlocks; cb++) {
        if (cb < ncb) {
          const int col = cb * 16 + lc;
          const double b = col < D ? (double)xr[col] : (col == D ? 1.0 : 0.0);
          acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[cb], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_has) return;
#pragma unroll
  for (int cb = 0; cb < kUttColBlocks; cb++) {
    if (cb < ncb) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int g = gb0 + wave * 16 + lk + 4 * r, col = cb * 16 + lc;
        if (g >= G) continue;
        if (col < D) Xout[((size_t)u * G + g) * D + col] = acc[cb][r];
        else if (col == D) gamma[(size_t)u * G + g] = acc[cb][r];
      }
    }
  }
}

// One workgroup per utterance: Σγ (each thread its Gaussians g = tid, tid + 256, … ascending, then a tree over the threads),
// and γ and X scaled by max_count / Σγ when Σγ exceeds it.
__global__ __launch_bounds__(256) void ivec_cap_kernel(double *gamma, double *X, int G, int D, double max_count) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double *gu = gamma + (size_t)blockIdx.x * G, *xu = X + (size_t)blockIdx.x * G * D;
  double a = 0.0;
  for (int g = tid; g < G; g += 256) a += gu[g];
  s[tid] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  const double tot = s[0];
  if (!(tot > max_count)) return;
  const double f = max_count / tot;
  for (int g = tid; g < G; g += 256) gu[g] *= f;
  for (int i = tid; i < G * D; i += 256) xu[i] *= f;
}

struct ScatParams {
  const float *feats; int64_t f0, f1;
  int D, G, n, PD, PDpad;
  const int32_t *gselect; const float *post;
  double *partial;                 // per slab of the pass [G][PDpad]
};

// grid (slabs of the pass, blocks of 64 Gaussians, groups of 64 packed columns).  Column p of the packed triangle is the pair
// (j, k), k <= j, p = j (j + 1) / 2 + k: B[frame][p] = x_j · x_k, float × float in double, exact.
__global__ __launch_bounds__(256) void ivec_scatter_kernel(ScatParams p) {
  __shared__ float Pt[kTileF][kGaussBlock + 1];
  __shared__ float X[kTileF][kXStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int gb0 = blockIdx.y * kGaussBlock, c0 = blockIdx.z * (16 * kScatBlocks);
  const int64_t s0 = p.f0 + (int64_t)blockIdx.x * kSlab, s1 = min(p.f1, s0 + kSlab);
  const bool wave_has = gb0 + wave * 16 < p.G;
  int cj[kScatBlocks], ck[kScatBlocks];
#pragma unroll
  for (int cb = 0; cb < kScatBlocks; cb++) {
    const int col = c0 + cb * 16 + lc;
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= col && j < kIvecMaxDim) j++;
    cj[cb] = col < p.PD ? j : -1;
    ck[cb] = col < p.PD ? col - j * (j + 1) / 2 : 0;
  }
  double4_t acc[kScatBlocks];
#pragma unroll
  for (int cb = 0; cb < kScatBlocks; cb++) acc[cb] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int64_t t0 = s0; t0 < s1; t0 += kTileF) {
    const int nf = (int)min((int64_t)kTileF, s1 - t0);
    ivec_stage_tile(p.feats, p.gselect, p.post, t0, nf, p.D, p.G, p.n, gb0, Pt, X, tid);
    if (!wave_has) continue;
    for (int r = 0; r < nf; r += 4) {
      const double a = (double)Pt[r + lk][wave * 16 + lc];
      if (__ballot(a != 0.0) == 0) continue;
      const float *xr = X[r + lk];
#pragma unroll
      for (int cb = 0; cb < kScatBlocks; cb++) {
        const double b = cj[cb] >= 0 ? (double)xr[cj[cb]] * (double)xr[ck[cb]] : 0.0;
        acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[cb], 0, 0, 0);
      }
    }
  }
  if (!wave_has) return;
  double *out = p.partial + (size_t)blockIdx.x * p.G * p.PDpad;
#pragma unroll
  for (int cb = 0; cb < kScatBlocks; cb++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int g = gb0 + wave * 16 + lk + 4 * r, col = c0 + cb * 16 + lc;
      if (g < p.G && col < p.PDpad) out[(size_t)g * p.PDpad + col] = acc[cb][r];
    }
  }
}

// One thread per (Gaussian, packed column): the caller's value, then the pass's slab partials in slab order.  A partial
// that is zero is not added: the bits are the same, and a Gaussian that no frame lists keeps the caller's bits.
__global__ __launch_bounds__(256) void ivec_scatter_reduce_kernel(const double *partial, int n_slabs, int G, int PD, int PDpad, double *S) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)G * PD) return;
  const int g = (int)(e / PD), col = (int)(e - (int64_t)g * PD);
  const double *src = partial + (size_t)g * PDpad + col;
  const size_t stride = (size_t)G * PDpad;
  double a = S[e];
  for (int s = 0; s < n_slabs; s++) {
    const double v = src[s * stride];
    if (v != 0.0) a += v;
  }
  S[e] = a;
}

struct SolveParams {
  int R, G;
  const double *gamma;   // the chunk's [C][G]
  double *Q;             // the chunk's [C][P]: Q in, Sc (or zeros) out
  double *lin;           // the chunk's [C][R]: lin in, μ (or zeros) out
  int32_t *live;         // the chunk's [C]
  double *mean, *var, *aux;   // the chunk's rows of the outputs; var and aux may be NULL
  int want_sc;
};

// One workgroup per utterance, the packed lower triangle in LDS.  Every element's sum runs over k ascending in one thread,
// the operations those of the host twin: Cholesky left-looking by columns (s = q − Σ l_ik·l_jk, the square root, the
// divisions), L⁻¹ in place by columns from the last, y = L⁻¹·lin, μ = L⁻ᵀ·y, Var = L⁻ᵀ·L⁻¹, Sc = Var + μ·μᵀ.  A Q that is not
// positive definite, or anything that is not finite, ends as NaN in this utterance's outputs; no index depends on a value.
// The inner loops are unrolled so that a batch of LDS reads is in flight before the dependent chain of additions needs them
// (one workgroup per CU leaves nothing else to hide their latency); the order of the additions is the loop's.
template <int kMaxR>
__global__ __launch_bounds__(256) void ivec_solve_kernel(SolveParams p) {
  __shared__ double L[kMaxR * (kMaxR + 1) / 2];
  __shared__ double v[kMaxR], y[kMaxR], mu[kMaxR], col[kMaxR];
  const int tid = threadIdx.x, R = p.R, P = R * (R + 1) / 2, c = blockIdx.x;
  double *Q = p.Q + (size_t)c * P;
  for (int e = tid; e < P; e += 256) L[e] = Q[e];
  if (tid < R) v[tid] = p.lin[(size_t)c * R + tid];
  int nz = 0;
  for (int g = tid; g < p.G; g += 256) nz |= p.gamma[(size_t)c * p.G + g] != 0.0;
  const int any = __syncthreads_or(nz);
  for (int j = 0; j < R; j++) {
    const int i = j + tid;
    double s = 0.0;
    if (i < R) {
      s = L[ivector_packed(i, j)];
      const double *li = L + ivector_packed(i, 0), *lj = L + ivector_packed(j, 0);
#pragma unroll 8
      for (int k = 0; k < j; k++) s -= li[k] * lj[k];
      if (i == j) L[ivector_packed(j, j)] = sqrt(s);
    }
    __syncthreads();
    if (i > j && i < R) L[ivector_packed(i, j)] = s / L[ivector_packed(j, j)];
    __syncthreads();
  }
  double logdet = 0.0;
  if (tid == 0 && p.aux) {
    for (int j = 0; j < R; j++) logdet += log(L[ivector_packed(j, j)]);
    logdet *= 2.0;
  }
  __syncthreads();
  for (int j = R - 1; j >= 0; j--) {
    const int i = tid;
    if (i > j && i < R) col[i] = L[ivector_packed(i, j)];
    const double d = L[ivector_packed(j, j)];
    __syncthreads();
    if (i > j && i < R) {
      double s = 0.0;
      const double *li = L + ivector_packed(i, 0);
#pragma unroll 8
      for (int k = j + 1; k <= i; k++) s += li[k] * col[k];
      L[ivector_packed(i, j)] = -(s / d);
    }
    if (i == j) L[ivector_packed(j, j)] = 1.0 / d;
    __syncthreads();
  }
  if (tid < R) {
    double s = 0.0;
    for (int k = 0; k <= tid; k++) s += L[ivector_packed(tid, k)] * v[k];
    y[tid] = s;
  }
  __syncthreads();
  int fin = 1;
  if (tid < R) {
    double s = 0.0;
    for (int k = tid; k < R; k++) s += L[ivector_packed(k, tid)] * y[k];
    mu[tid] = s;
    fin = isfinite(s) ? 1 : 0;
    p.mean[(size_t)c * R + tid] = s;
  }
  const int live = __syncthreads_and(fin) && any;
  if (tid == 0) {
    p.live[c] = live;
    if (p.aux) {
      double quad = 0.0;
      for (int r = 0; r < R; r++) quad += v[r] * mu[r];
      p.aux[2 * (size_t)c] = quad;
      p.aux[2 * (size_t)c + 1] = logdet;
    }
  }
  if (tid < R && p.want_sc) p.lin[(size_t)c * R + tid] = live ? mu[tid] : 0.0;
  if (!p.var && !p.want_sc) return;
  for (int e = tid; e < P; e += 256) {
    int r = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= e) r++;
    while (r * (r + 1) / 2 > e) r--;
    const int cc = e - r * (r + 1) / 2;
    double s = 0.0;
#pragma unroll 8
    for (int k = r; k < R; k++) s += L[ivector_packed(k, r)] * L[ivector_packed(k, cc)];
    if (p.var) p.var[(size_t)c * P + e] = s;
    if (p.want_sc) Q[e] = live ? s + mu[r] * mu[cc] : 0.0;
  }
}

// A thread per element of (Γ | isum | iscat | n): the chunk's live utterances added in order onto the caller's value.
__global__ __launch_bounds__(256) void ivec_small_acc_kernel(const double *gamma, const double *mu, const double *Sc, const int32_t *live,
                                                             int C, int G, int R, int P, double *Gamma, double *isum, double *iscat,
                                                             double *n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= G + R + P + 1) return;
  const double *src; size_t stride; double *dst;
  if (e < G) { src = gamma + e; stride = G; dst = Gamma + e; }
  else if (e < G + R) { src = mu + (e - G); stride = R; dst = isum + (e - G); }
  else if (e < G + R + P) { src = Sc + (e - G - R); stride = P; dst = iscat + (e - G - R); }
  else { src = nullptr; stride = 0; dst = n; }
  double a = *dst;
  for (int c = 0; c < C; c++)
    if (live[c]) a += src ? src[c * stride] : 1.0;
  *dst = a;
}

int refuse(mfa_ctx *c, const char *who, int rc, int dim, int G, int n, int R, long long frames) {
  switch (rc) {
    case -2: return c->fail("%s: feature dim %d (1 to %d: columns of a staged row)", who, dim, kIvecMaxDim);
    case -3: return c->fail("%s: %d Gaussians (1 to %d)", who, G, kIvecMaxGauss);
    case -4: return c->fail("%s: lists of %d entries per frame (1 to %d)", who, n, kIvecMaxSelect);
    case -5: return c->fail("%s: %lld frames or utterances in one call (fewer than 2^31)", who, frames);
    case -6: return c->fail("%s: i-vector dimension %d (1 to %d: the packed triangle of Q lives in one workgroup's LDS)", who, R, kIvecMaxR);
    default: return c->fail("%s: a negative count", who);
  }
}

size_t env_count(const char *name) {
  const char *e = getenv(name);
  const long v = e ? atol(e) : 0;
  return v > 0 ? (size_t)v : 0;
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_ivector_scatter_slab_frames(void) { return kSlab; }

MFA_API int mfa_ivector_prune_post_batch(mfa_ctx *c, const float *d_post, int64_t total_frames, int32_t n, float min_post, float scale,
                                         float *d_out) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "posterior pruning";
  const int rc = ivector_check_shape(1, 1, n, 1, total_frames, 0);
  if (rc) return refuse(c, who, rc, 1, 1, n, 1, (long long)total_frames);
  if (total_frames == 0) return 0;
  if (!d_post || !d_out) return c->fail("%s: NULL array", who);
  KernelTimer kt(c, MFA_K_IVEC_PRUNE);
  hipLaunchKernelGGL(ivec_prune_kernel, dim3((unsigned)((total_frames + 255) / 256)), dim3(256), 0, c->stream, d_post, total_frames, n,
                     min_post, scale, d_out);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "ivec_prune_kernel frames=%lld n=%d", (long long)total_frames, n);
  return 0;
}

MFA_API int mfa_ivector_utt_stats_batch(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                                        int32_t dim, int32_t G, int32_t n, const int32_t *d_gselect, const float *d_post, double max_count,
                                        double *d_gamma, double *d_X, double *d_S) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "i-vector utterance statistics";
  if (n_utt < 0) return c->fail("%s: %d utterances", who, n_utt);
  const int rc = ivector_check_shape(dim, G, n, 1, total_frames, n_utt);
  if (rc) return refuse(c, who, rc, dim, G, n, 1, (long long)total_frames);
  if (n_utt == 0) return 0;
  if (!d_frame_off || !d_gamma || !d_X) return c->fail("%s: NULL array", who);
  if (total_frames > 0 && (!d_feats || !d_gselect || !d_post)) return c->fail("%s: NULL input array", who);
  {
    KernelTimer kt(c, MFA_K_IVEC_UTT);
    hipLaunchKernelGGL(ivec_utt_kernel, dim3((unsigned)n_utt, (unsigned)((G + kGaussBlock - 1) / kGaussBlock)), dim3(256), 0, c->stream,
                       d_feats, d_frame_off, total_frames, dim, G, n, d_gselect, d_post, d_gamma, d_X);
    if (max_count > 0.0)
      hipLaunchKernelGGL(ivec_cap_kernel, dim3((unsigned)n_utt), dim3(256), 0, c->stream, d_gamma, d_X, G, dim, max_count);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "ivec_utt_kernel utts=%d G=%d n=%d", n_utt, G, n);
  }
  if (!d_S || total_frames == 0) return 0;
  const int PD = dim * (dim + 1) / 2, ngroups = (PD + 16 * kScatBlocks - 1) / (16 * kScatBlocks), PDpad = ngroups * 16 * kScatBlocks;
  const size_t n_slabs = ((size_t)total_frames + kSlab - 1) / kSlab, partial_bytes = (size_t)G * PDpad * 8;
  const size_t forced = env_count("MFA_IVECTOR_PASS_SLABS");
  const size_t per_pass = std::min(n_slabs, forced ? forced : std::max<size_t>(1, kScatPassBytes / partial_bytes));
  Workspace ws;
  const size_t o_part = ws.take(per_pass * partial_bytes);
  if (ws.reserve(c, "the i-vector scatter workspace")) return -1;
  double *partial = ws.at<double>(o_part);
  KernelTimer kt(c, MFA_K_IVEC_SCATTER);
  for (size_t slab0 = 0; slab0 < n_slabs; slab0 += per_pass) {
    const size_t slabs = std::min(per_pass, n_slabs - slab0);
    const int64_t f0 = (int64_t)(slab0 * kSlab), f1 = std::min(total_frames, f0 + (int64_t)(slabs * kSlab));
    const ScatParams sp{d_feats, f0, f1, dim, G, n, PD, PDpad, d_gselect, d_post, partial};
    hipLaunchKernelGGL(ivec_scatter_kernel, dim3((unsigned)slabs, (unsigned)((G + kGaussBlock - 1) / kGaussBlock), (unsigned)ngroups), dim3(256),
                       0, c->stream, sp);
    hipLaunchKernelGGL(ivec_scatter_reduce_kernel, dim3((unsigned)(((size_t)G * PD + 255) / 256)), dim3(256), 0, c->stream, partial, (int)slabs,
                       G, PD, PDpad, d_S);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "ivec_scatter_kernel slabs=%zu", slabs);
  }
  return 0;
}

MFA_API int mfa_ivector_estep_batch(mfa_ctx *c, const double *d_gamma, const double *d_X, int32_t n_utt, int32_t dim, int32_t G, int32_t R,
                                    const double *d_W, const double *d_U, double prior_offset, double *d_ivec_mean, double *d_ivec_var,
                                    double *d_aux, double *d_Gamma, double *d_Y, double *d_Rq, double *d_isum, double *d_iscat, double *d_n) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "i-vector E-step";
  if (n_utt < 0) return c->fail("%s: %d utterances", who, n_utt);
  const int rc = ivector_check_shape(dim, G, 1, R, 0, n_utt);
  if (rc) return refuse(c, who, rc, dim, G, 1, R, (long long)n_utt);
  const int nacc = (d_Gamma != nullptr) + (d_Y != nullptr) + (d_Rq != nullptr) + (d_isum != nullptr) + (d_iscat != nullptr) + (d_n != nullptr);
  if (nacc != 0 && nacc != 6) return c->fail("%s: the accumulators are all NULL (extraction) or all set", who);
  if (n_utt == 0) return 0;
  if (!d_gamma || !d_X || !d_W || !d_U) return c->fail("%s: NULL input array", who);
  if (!d_ivec_mean) return c->fail("%s: NULL output array", who);
  const bool acc = nacc == 6;
  const int P = R * (R + 1) / 2, GD = G * dim;
  // utterances per chunk: a multiple of 4, the K of the matrix instruction, so that a step of the accumulating products
  // holds the same four utterances whatever the chunk size
  const size_t per_utt = (size_t)P * 8 + (size_t)R * 8 + 4;
  const size_t forced = env_count("MFA_IVECTOR_PASS_UTTS");
  size_t chunk = forced ? forced : std::max<size_t>(4, kEstepPassBytes / per_utt);
  chunk = std::min((chunk + 3) / 4 * 4, ((size_t)n_utt + 3) / 4 * 4);
  Workspace ws;
  const size_t o_q = ws.take(chunk * P * 8), o_lin = ws.take(chunk * R * 8), o_live = ws.take(chunk * 4);
  if (ws.reserve(c, "the i-vector E-step workspace")) return -1;
  double *Q = ws.at<double>(o_q), *lin = ws.at<double>(o_lin);
  int32_t *live = ws.at<int32_t>(o_live);
  for (size_t u0 = 0; u0 < (size_t)n_utt; u0 += chunk) {
    const int C = (int)std::min(chunk, (size_t)n_utt - u0);
    const double *gam = d_gamma + u0 * G, *Xc = d_X + u0 * GD;
    {
      KernelTimer kt(c, MFA_K_IVEC_PRODUCTS);
      launch_gemm<1>(c, GemmParams{gam, G, 1, d_U, P, 1, Q, C, P, G, nullptr, 0.0, nullptr});
      launch_gemm<2>(c, GemmParams{Xc, GD, 1, d_W, R, 1, lin, C, R, GD, nullptr, prior_offset, nullptr});
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "f64_gemm_kernel Q, lin: utts=[%zu, %zu) R=%d", u0, u0 + C, R);
    }
    {
      KernelTimer kt(c, MFA_K_IVEC_SOLVE);
      const SolveParams sp{R, G, gam, Q, lin, live, d_ivec_mean + u0 * R, d_ivec_var ? d_ivec_var + u0 * P : nullptr,
                           d_aux ? d_aux + 2 * u0 : nullptr, acc ? 1 : 0};
      if (R <= 64) hipLaunchKernelGGL(ivec_solve_kernel<64>, dim3((unsigned)C), dim3(256), 0, c->stream, sp);
      else hipLaunchKernelGGL(ivec_solve_kernel<kIvecMaxR>, dim3((unsigned)C), dim3(256), 0, c->stream, sp);
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "ivec_solve_kernel utts=%d R=%d", C, R);
    }
    if (!acc) continue;
    KernelTimer kt(c, MFA_K_IVEC_ACC);
    launch_gemm<0>(c, GemmParams{gam, 1, G, Q, P, 1, d_Rq, G, P, C, live, 0.0, nullptr});
    launch_gemm<0>(c, GemmParams{Xc, 1, GD, lin, R, 1, d_Y, GD, R, C, live, 0.0, nullptr});
    hipLaunchKernelGGL(ivec_small_acc_kernel, dim3((unsigned)((G + R + P + 1 + 255) / 256)), dim3(256), 0, c->stream, gam, lin, Q, live, C, G, R,
                       P, d_Gamma, d_isum, d_iscat, d_n);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "ivec accumulate utts=%d", C);
  }
  return 0;
}

}  // extern "C"
