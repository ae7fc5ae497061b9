// LDA statistics on gfx950: the accumulation of the reference's LDA stage (LdaAccStatsFunction → kalpy LdaStatsAccumulator,
// Kaldi acc-lda = LdaEstimate::Accumulate) in the spliced feature space, which is never materialised.
// Arithmetic contract: include/mfa_hip.h "LDA statistics"; the shared arithmetic: lda_acc_math.hpp; the host twin:
// lda_acc_host.cpp.
//
// The ordering by class, the units and the reductions are the segment skeleton of acc_segments.hpp:
//   lookup   lda_lookup_kernel: per frame its utterance, class and weight (after the random prune), the sort key (class;
//            n_classes = takes no part), the classes' frame counts and the transition-id counts;
//            lda_offsets_kernel: every utterance's CMVN offsets as float32
//   second   lda_second_kernel, one workgroup per slab of kSlab consecutive frames of the batch: Σ (w·x)·xᵀ on the f64
//            matrix pipe, the lower-triangle 16×16 tiles spread over four wavefronts; the slab's partial to the workspace
//   order    rocPRIM radix_sort_pairs (stable) of (class, frame index), then the scan of segment starts and units
//   class    lda_class_kernel, one workgroup per unit = (class, chunk of kChunk consecutive entries of its segment):
//            Σ w and Σ w·x from zero in frame order
//   reduce   the caller's value, then the slabs' (the class's chunks') partials in order; the second moment's upper
//            triangle is a copy of the lower
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "acc_segments.hpp"
#include "ctx.hpp"
#include "lda_acc_math.hpp"

namespace {

constexpr int kSlab = 4096;      // frames of the batch per second-moment partial (mfa_lda_acc_slab_frames)
constexpr int kTile = 64;        // frames staged in LDS at a time (plus 2·ctx halo rows): 16 steps of the instruction's K = 4
constexpr int kChunk = 512;      // entries of a class's segment per unit (mfa_lda_acc_chunk_frames)
constexpr int kMaxS = kLdaMaxSpliced;
constexpr int kMaxBlocks = kMaxS / 16;                          // 16-wide blocks of the padded spliced vector
constexpr int kMaxTiles = kMaxBlocks * (kMaxBlocks + 1) / 2;    // lower-triangle tiles: 36
constexpr int kWaves = 4;
constexpr int kTilesPerWave = (kMaxTiles + kWaves - 1) / kWaves;
// rows r .. r + 2·ctx of the staged tile are frame r's spliced vector, read up to the padded width from the last row
constexpr int kXFloats = kTile * kMaxS + 2 * kMaxS;
static_assert(kSlab % kTile == 0 && kTile % 4 == 0 && kMaxS % 16 == 0, "lda_second_kernel tiling");

typedef double double4_t __attribute__((ext_vector_type(4)));

struct LookupParams {
  const int32_t *ali; const int64_t *frame_off; int32_t n_utt; int64_t n;
  const int32_t *tid2class; const float *tid_weight; int32_t n_tids, n_classes;
  float theta; const uint32_t *utt_key; uint32_t seed;
  uint32_t *key, *val; float *weight; int32_t *utt; int32_t *class_count; unsigned long long *tid_count;
};

__global__ __launch_bounds__(256) void lda_lookup_kernel(LookupParams p) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = t < p.n;
  int32_t c = 0, u = 0;
  float w = 0.0f;
  const int tid = in ? p.ali[t] : 0;
  bool take = in && lda_frame_class(tid, p.tid2class, p.tid_weight, p.n_tids, p.n_classes, &c, &w);
  if (in) u = acc_owner(p.frame_off, p.n_utt, t);   // for t inside the batch that utterance is not empty and holds t
  if (take && p.theta > 0.0f) {
    w = lda_prune_weight(w, p.theta, p.seed, p.utt_key[u], (uint32_t)(t - p.frame_off[u]));
    take = w != 0.0f;
  }
  if (in) {
    p.key[t] = take ? (uint32_t)c : (uint32_t)p.n_classes;
    p.val[t] = (uint32_t)t;
    p.weight[t] = take ? w : 0.0f;
    p.utt[t] = u;
  }
  // one atomic per run of equal transition-ids inside the wavefront (acc_segments.hpp has the reasoning)
  acc_wave_runs(take, tid, [&](int len) {
    atomicAdd(&p.class_count[c], len);
    if (p.tid_count) atomicAdd(&p.tid_count[tid], (unsigned long long)len);
  });
}

// off[u][d] = what CMVN subtracts from column d of utterance u's rows (0 without CMVN)
__global__ void lda_offsets_kernel(const int32_t *utt2spk, const double *cmvn, int n_utt, int dim, float *off) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_utt * dim) return;
  const int u = i / dim, d = i - u * dim;
  off[i] = cmvn ? lda_cmvn_offset(cmvn + (size_t)utt2spk[u] * 2 * (dim + 1), dim, d) : 0.0f;
}

struct SecondParams {
  const float *mfcc; const int64_t *frame_off; int32_t n_utt; int64_t n;
  int dim, ctx, S, nb;             // nb: 16-wide blocks of S
  const float *off; const float *weight;
  double *partial;                 // per slab [tiles][16][16], tile (I, J <= I) at I·(I + 1)/2 + J
};

// grid: the slabs; 256 threads.  The slab is walked in pieces of at most kTile frames of ONE utterance: the piece's base
// rows and its 2·ctx halo rows (clamped to the utterance) are staged CMVN-applied with row stride dim, so the spliced vector
// of the piece's frame r is the contiguous run X[r·dim .. r·dim + S).  A step of the instruction takes 4 frames: lane l
// gives, for the tile's row block I and column block J, A[i = l & 15][k = l >> 4] = w_k·x_k[16 I + i] (formed in double: exact)
// and B[k = l >> 4][j = l & 15] = x_k[16 J + j]; columns past S and frames past the piece (weight 0) are zero operands.
// Result layout of the f64 instruction: register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15].
__global__ __launch_bounds__(256) void lda_second_kernel(SecondParams p) {
  __shared__ float X[kXFloats];
  __shared__ float W[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dim = p.dim, ctx = p.ctx, S = p.S, nb = p.nb, ntiles = nb * (nb + 1) / 2;
  const int64_t g0 = (int64_t)blockIdx.x * kSlab, g1 = min(p.n, g0 + kSlab);
  if (g0 >= g1) return;
  const int lc = lane & 15, lk = lane >> 4;

  int oa[kTilesPerWave], ob[kTilesPerWave];          // the lane's element of the tile's row / column block, or -1 (zero)
  double4_t acc[kTilesPerWave];
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    const int tile = wave + kWaves * q;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= tile) I++;
    const int J = tile - I * (I + 1) / 2;
    const int a = 16 * I + lc, b = 16 * J + lc;
    oa[q] = tile < ntiles && a < S ? a : -1;
    ob[q] = tile < ntiles && b < S ? b : -1;
    acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  }

  int u = acc_owner(p.frame_off, p.n_utt, g0);
  int64_t g = g0;
  while (g < g1) {
    while (u + 1 < p.n_utt && p.frame_off[u + 1] <= g) u++;
    const int64_t f0 = p.frame_off[u], f1 = min(p.frame_off[u + 1], p.n);
    if (f0 > g || f1 <= g) break;                    // offsets that do not describe the batch: nothing more is read
    const int n = (int)min((int64_t)kTile, min(g1, f1) - g);
    const int rows = n + 2 * ctx;
    const float *off = p.off + (size_t)u * dim;
    __syncthreads();                                 // the previous piece's readers are done
    for (int i = tid; i < rows * dim; i += 256) {
      const int r = i / dim, d = i - r * dim;
      int64_t t = g - ctx + r;
      t = t < f0 ? f0 : (t >= f1 ? f1 - 1 : t);
      X[i] = lda_cmvn_apply(p.mfcc[t * dim + d], off[d]);
    }
    if (tid < kTile) W[tid] = tid < n ? p.weight[g + tid] : 0.0f;
    __syncthreads();
    for (int r = 0; r < n; r += 4) {
      const float wk = W[r + lk];
      const double wd = (double)wk;
      const float *xr = X + (r + lk) * dim;
#pragma unroll
      for (int q = 0; q < kTilesPerWave; q++) {
        if (wave + kWaves * q < ntiles) {            // the same for the whole wavefront
          const bool ua = wk != 0.0f && oa[q] >= 0, ub = wk != 0.0f && ob[q] >= 0;
          const float xa = xr[ua ? oa[q] : 0], xb = xr[ub ? ob[q] : 0];
          const double a = ua ? wd * (double)xa : 0.0, b = ub ? (double)xb : 0.0;
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
        }
      }
    }
    g += n;
  }

  double *out = p.partial + (size_t)blockIdx.x * ntiles * 256;
#pragma unroll
  for (int q = 0; q < kTilesPerWave; q++) {
    const int tile = wave + kWaves * q;
    if (tile < ntiles) {
#pragma unroll
      for (int r = 0; r < 4; r++) out[(size_t)tile * 256 + (lk + 4 * r) * 16 + lc] = acc[q][r];
    }
  }
}

// One thread per element (i, j <= i) of the lower triangle: the caller's value, then the slabs' partials in slab order
// (acc_ordered_sum); the sum goes to both (i, j) and (j, i).
__global__ __launch_bounds__(256) void lda_second_reduce_kernel(const double *partial, int n_slabs, int S, int nb, double *second) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S * S) return;
  const int i = e / S, j = e - i * S;
  if (j > i) return;
  const int I = i >> 4, J = j >> 4, ntiles = nb * (nb + 1) / 2;
  const size_t stride = (size_t)ntiles * 256;
  const double *base = partial + (size_t)(I * (I + 1) / 2 + J) * 256 + (i & 15) * 16 + (j & 15);
  const double a = acc_ordered_sum(base, stride, n_slabs, second[(size_t)i * S + j]);
  second[(size_t)i * S + j] = a;
  second[(size_t)j * S + i] = a;
}

// acc_scan_kernel<2> over the classes: frames, units
struct LdaScan {
  const int32_t *cnt;
  int32_t *seg_off; int32_t *unit_base;
  __device__ void add(int q, int64_t (&v)[2]) const { v[0] += cnt[q]; v[1] += (cnt[q] + kChunk - 1) / kChunk; }
  __device__ void put(int q, const int64_t (&v)[2]) const { seg_off[q] = (int32_t)v[0]; unit_base[q] = (int32_t)v[1]; }
};

struct ClassParams {
  const float *mfcc; const int64_t *frame_off; int64_t n;
  int dim, ctx, S, C;
  const float *off; const float *weight; const int32_t *utt; const uint32_t *idx;   // idx: frame indices ordered by class
  const int32_t *seg_off; const int32_t *unit_base;
  double *partial;                 // per unit [S + 1]: Σ w, Σ w·x
};

// grid: an upper bound of the units (the true count is unit_base[C], known on the device only); 128 threads, thread i owns
// element i of the spliced vector.  The chunk's entries are described in LDS first (frame, weight, utterance bounds), then
// every thread walks them in order: its element's row, clamped, straight from the base features.
__global__ __launch_bounds__(128) void lda_class_kernel(ClassParams p) {
  __shared__ int64_t t_s[kChunk], f0_s[kChunk], f1_s[kChunk];
  __shared__ int32_t u_s[kChunk];
  __shared__ float w_s[kChunk];
  const int unit = blockIdx.x, C = p.C;
  if (unit >= p.unit_base[C]) return;
  const int cls = acc_owner(p.unit_base, C, unit), chunk = unit - p.unit_base[cls];
  const int s0 = p.seg_off[cls] + chunk * kChunk, s1 = min(p.seg_off[cls + 1], s0 + kChunk), n = s1 - s0;
  const int tid = threadIdx.x;
  for (int e = tid; e < n; e += 128) {
    const int64_t t = (int64_t)p.idx[s0 + e];
    const int u = p.utt[t];
    t_s[e] = t; u_s[e] = u; w_s[e] = p.weight[t];
    f0_s[e] = p.frame_off[u]; f1_s[e] = min(p.frame_off[u + 1], p.n);
  }
  __syncthreads();
  const int i = tid, dim = p.dim;
  if (i < p.S) {
    const int o = i / dim, col = i - o * dim;
    double z = 0.0, f = 0.0;
#pragma unroll 4
    for (int e = 0; e < n; e++) {
      const int64_t f0 = f0_s[e], f1 = f1_s[e];
      int64_t r = t_s[e] + o - p.ctx;
      r = r < f0 ? f0 : (r >= f1 ? f1 - 1 : r);
      const float x = lda_cmvn_apply(p.mfcc[r * dim + col], p.off[(size_t)u_s[e] * dim + col]);
      const double wd = (double)w_s[e];
      z += wd;
      lda_first_add(wd, x, f);
    }
    double *out = p.partial + (size_t)unit * (p.S + 1);
    out[1 + i] = f;
    if (i == 0) out[0] = z;
  }
}

// grid: the classes; 256 threads over the class's [S + 1] sums: the caller's value, then its units' partials in chunk order
// (acc_ordered_sum).
__global__ __launch_bounds__(256) void lda_class_reduce_kernel(const double *partial, const int32_t *unit_base, int S, double *zero,
                                                               double *first) {
  const int cls = blockIdx.x, u0 = unit_base[cls], nu = unit_base[cls + 1] - u0;
  const int e = threadIdx.x;
  if (nu == 0 || e > S) return;
  double *dst = e == 0 ? zero + cls : first + (size_t)cls * S + (e - 1);
  const double *base = partial + (size_t)u0 * (S + 1) + e;
  *dst = acc_ordered_sum(base, (size_t)(S + 1), nu, *dst);
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_lda_acc_slab_frames(void) { return kSlab; }
MFA_API int32_t mfa_lda_acc_chunk_frames(void) { return kChunk; }
MFA_API int32_t mfa_lda_acc_max_dim(void) { return kMaxS; }

MFA_API int mfa_lda_acc_batch(mfa_ctx *c, const float *d_mfcc, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                              int32_t dim, const int32_t *d_utt2spk, const double *d_cmvn, int32_t splice_ctx,
                              const int32_t *d_ali, const int32_t *d_tid2class, const float *d_tid_weight, int32_t n_tids,
                              int32_t n_classes, float rand_prune, const uint32_t *d_utt_key, uint32_t seed, double *d_zero,
                              double *d_first, double *d_second, int64_t *d_tid_count) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (dim <= 0 || splice_ctx < 0) return c->fail("LDA statistics: base dim %d, splice context %d: no spliced vector", dim, splice_ctx);
  const int64_t S64 = (2 * (int64_t)splice_ctx + 1) * dim;
  if (S64 > kMaxS) return c->fail("LDA statistics: spliced dim %lld > %d (the lower-triangle tiles of four wavefronts)", (long long)S64, kMaxS);
  if (n_classes <= 0) return c->fail("LDA statistics: %d classes", n_classes);
  if (total_frames >= ((int64_t)1 << 31) - kSlab) return c->fail("LDA statistics: %lld frames in one call (at most 2^31 - %d)", (long long)total_frames, kSlab + 1);
  if (total_frames <= 0 || n_utt <= 0) return 0;
  if (n_tids <= 0) return c->fail("LDA statistics: empty transition-id table");
  if (!d_mfcc || !d_frame_off || !d_ali || !d_tid2class || !d_tid_weight) return c->fail("LDA statistics: NULL input array");
  if (!d_zero || !d_first || !d_second) return c->fail("LDA statistics: NULL accumulator");
  if (d_cmvn && !d_utt2spk) return c->fail("LDA statistics: CMVN given without utt2spk");
  if (rand_prune > 0.0f && !d_utt_key) return c->fail("LDA statistics: random pruning without utterance keys");
  const int S = (int)S64, nb = (S + 15) / 16, ntiles = nb * (nb + 1) / 2, C = n_classes;

  const size_t T = (size_t)total_frames;
  const size_t n_slabs = (T + kSlab - 1) / kSlab;
  const size_t units_max = T / kChunk + (size_t)C;                              // Σ ceil(n_c / chunk) <= floor(T / chunk) + C
  const unsigned end_bit = acc_end_bit((uint64_t)C);
  size_t sort_bytes = 0;
  MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0u, end_bit, c->stream));
  Workspace ws;
  const size_t o_key = ws.take(T * 4), o_key2 = ws.take(T * 4), o_val = ws.take(T * 4), o_val2 = ws.take(T * 4), o_wgt = ws.take(T * 4),
               o_utt = ws.take(T * 4), o_off = ws.take((size_t)n_utt * dim * 4), o_cnt = ws.take(((size_t)C + 1) * 4),
               o_seg = ws.take(((size_t)C + 1) * 4), o_ub = ws.take(((size_t)C + 1) * 4),
               o_cpart = ws.take(units_max * ((size_t)S + 1) * 8), o_spart = ws.take(n_slabs * (size_t)ntiles * 256 * 8),
               o_sort = ws.take(sort_bytes);
  if (ws.reserve(c, "the LDA statistics workspace")) return -1;
  uint32_t *key = ws.at<uint32_t>(o_key), *key2 = ws.at<uint32_t>(o_key2), *val = ws.at<uint32_t>(o_val), *val2 = ws.at<uint32_t>(o_val2);
  float *wgt = ws.at<float>(o_wgt), *off = ws.at<float>(o_off);
  int32_t *utt = ws.at<int32_t>(o_utt), *cnt = ws.at<int32_t>(o_cnt), *seg = ws.at<int32_t>(o_seg), *ub = ws.at<int32_t>(o_ub);
  double *cpart = ws.at<double>(o_cpart), *spart = ws.at<double>(o_spart);

  {
    KernelTimer kt(c, MFA_K_LDA_LOOKUP);
    MFA_HIP_CHECK(c, hipMemsetAsync(cnt, 0, ((size_t)C + 1) * 4, c->stream));
    LookupParams lp{d_ali, d_frame_off, n_utt, total_frames, d_tid2class, d_tid_weight, n_tids, C, rand_prune, d_utt_key, seed,
                    key, val, wgt, utt, cnt, (unsigned long long *)d_tid_count};
    hipLaunchKernelGGL(lda_lookup_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, c->stream, lp);
    hipLaunchKernelGGL(lda_offsets_kernel, dim3((unsigned)(((size_t)n_utt * dim + 255) / 256)), dim3(256), 0, c->stream, d_utt2spk,
                       d_cmvn, n_utt, dim, off);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_LDA_SECOND);
    SecondParams sp{d_mfcc, d_frame_off, n_utt, total_frames, dim, splice_ctx, S, nb, off, wgt, spart};
    hipLaunchKernelGGL(lda_second_kernel, dim3((unsigned)n_slabs), dim3(256), 0, c->stream, sp);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_LDA_CLASS);
    MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(ws.at<char>(o_sort), sort_bytes, key, key2, val, val2, T, 0u, end_bit, c->stream));
    hipLaunchKernelGGL((acc_scan_kernel<2, LdaScan>), dim3(1), dim3(256), 0, c->stream, LdaScan{cnt, seg, ub}, C);
    ClassParams cp{d_mfcc, d_frame_off, total_frames, dim, splice_ctx, S, C, off, wgt, utt, val2, seg, ub, cpart};
    hipLaunchKernelGGL(lda_class_kernel, dim3((unsigned)units_max), dim3(128), 0, c->stream, cp);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_LDA_REDUCE);
    hipLaunchKernelGGL(lda_second_reduce_kernel, dim3((unsigned)((S * S + 255) / 256)), dim3(256), 0, c->stream, spart, (int)n_slabs,
                       S, nb, d_second);
    hipLaunchKernelGGL(lda_class_reduce_kernel, dim3((unsigned)C), dim3(256), 0, c->stream, cpart, ub, S, d_zero, d_first);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  return 0;
}

}  // extern "C"
