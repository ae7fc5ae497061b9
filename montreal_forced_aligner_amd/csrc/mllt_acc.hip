// MLLT statistics on gfx950: the accumulation of the reference's LDA+MLLT stage (MFA/acoustic_modeling/lda.py:122-180 →
// kalpy MlltStatsAccumulator, Kaldi gmm-acc-mllt = MlltAccs::AccumulateFromPosteriors) in the factored form
// G_j = Σ_g inv_var_g[j] · F_g: the device forms the per-Gaussian full second moments F_g = Σ_t γ_tg d_tg d_tgᵀ, the
// contraction over the Gaussians is a float64 GEMM on the host (mllt.py).
// Arithmetic contract: include/mfa_hip.h "MLLT statistics"; the shared arithmetic: mllt_acc_math.hpp over gmm_acc_math.hpp;
// the host twin: mllt_acc_host.cpp.
//
// The steps are the segment skeleton of acc_segments.hpp, the posterior phase is acc_posterior.hpp's:
//   lookup   fmllr_tid_lookup_kernel (tid_lookup.hpp), as the GMM statistics run it
//   order    rocPRIM radix_sort_pairs (stable) of (pdf, frame index); the scan gives the pdfs' segment starts, their units
//            (chunks of kChunk entries) and sub-units (chunks of kSub entries: the GMM statistics' chunks)
//   sums     mllt_acc_kernel, one workgroup per (unit, group of kGroup Gaussians of the pdf): the posteriors of all the pdf's
//            Gaussians by the pieces gmm_acc_kernel forms them with, then the group's lower-triangle 16×16 tiles of
//            Σ (γ·d)·dᵀ on the f64 matrix pipe; group 0 also sums occ and the totals per sub-unit
//   reduce   per pdf, the units' partials in chunk order onto the caller's full (both triangles written), the sub-units'
//            onto occ, the totals in (pdf, sub-unit) order
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "acc_posterior.hpp"
#include "acc_segments.hpp"
#include "ctx.hpp"
#include "mllt_acc_math.hpp"
#include "tid_lookup.hpp"

namespace {

constexpr int kSub = 512;        // entries per occ / totals partial: mfa_gmm_acc_chunk_frames(), so that both have that call's bits
constexpr int kSubsPerChunk = 8;
constexpr int kChunk = kSub * kSubsPerChunk;   // entries of a pdf's segment per unit (mfa_mllt_acc_chunk_frames)
constexpr int kTile = kAccTile, kMaxGauss = kAccMaxGauss, kMaxDim = kAccMaxDim, kXStride = kAccXStride;
constexpr int kBlocks = kMaxDim / 16;                    // 16-wide blocks of the padded feature vector
constexpr int kTiles = kBlocks * (kBlocks + 1) / 2;      // lower-triangle tiles of one Gaussian: 6
constexpr int kWaves = 4;
constexpr int kGaussPerWave = 4;                         // 4 · 6 tiles · 4 doubles = 192 accumulator registers per lane
constexpr int kGroup = kWaves * kGaussPerWave;           // Gaussians of a pdf per workgroup
static_assert(kSub % kTile == 0 && kTile % 4 == 0 && kMaxDim % 16 == 0 && kMaxGauss % kGroup == 0, "mllt_acc_kernel tiling");

typedef double double4_t __attribute__((ext_vector_type(4)));

// acc_scan_kernel<5> over the pdfs
struct MlltAccScan {
  const int32_t *cnt; const int32_t *ngauss;
  int32_t *seg_off, *unit_base, *sub_base;    // [P + 1] each: first sorted entry, first unit, first sub-unit of every pdf
  int64_t *prow, *srow;                       // [P + 1]: first partial row (units × Gaussians), first occ row (sub-units × Gaussians)
  __device__ void add(int q, int64_t (&v)[5]) const {
    const int64_t c = cnt[q], un = (c + kChunk - 1) / kChunk, sn = (c + kSub - 1) / kSub, ng = ngauss[q];
    v[0] += c; v[1] += un; v[2] += sn; v[3] += un * ng; v[4] += sn * ng;
  }
  __device__ void put(int q, const int64_t (&v)[5]) const {
    seg_off[q] = (int32_t)v[0]; unit_base[q] = (int32_t)v[1]; sub_base[q] = (int32_t)v[2];
    prow[q] = v[3]; srow[q] = v[4];
  }
};

struct AccParams {
  int D, kpad, num_pdfs;
  const float *w; const float *gc; const int32_t *row0;     // packed model (gmm_pack.hpp layout)
  const int32_t *ngauss; const int32_t *goff;               // [num_pdfs] Gaussians per pdf, first model Gaussian
  const float *means;                                       // [G][D], model Gaussian order
  const float *feats; const uint32_t *idx; const float *weight;   // idx: frame indices ordered by pdf
  const int32_t *seg_off; const int32_t *unit_base; const int32_t *sub_base; const int64_t *prow; const int64_t *srow;
  double *partial;     // per (unit, Gaussian) the lower triangle, element (i, j <= i) at i·(i + 1)/2 + j
  double *occ_part;    // per (sub-unit, Gaussian)
  double *sub_tot;     // per sub-unit {Σ w·loglike, Σ w}
};

// grid (an upper bound of the units — the true count is unit_base[num_pdfs], known on the device only —, groups of kGroup
// Gaussians); 256 threads.
// Posterior phase: acc_posterior_phase (acc_posterior.hpp), the function gmm_acc_kernel runs, so that γ, occ and the totals
// carry that kernel's bits; rows of post_s past the chunk's end are written as zeros for the moment phase.  The small pieces
// around it (owner search, gconsts, prefetch, LDS store, the occ / totals loops) are written out here although
// acc_posterior.hpp and acc_segments.hpp have them: with any of them called, the compiler schedules this kernel's 192
// accumulator registers another way and the sums stage takes 35.5 ms, not 35.0 (tools/mllt_rate.py's shape).
// Every group forms the posteriors of the whole pdf (the softmax needs them all): at most 128 · 2·dim float32 FMAs per frame beside the group's 16 · 6 matrix
// instructions per 4 frames.
// Moment phase: wavefront v owns Gaussians group·16 + v + 4 q (q < 4) and all their tiles.  A step of the instruction takes
// 4 frames, the operand layout is lda_second_kernel's: lane l gives, for the tile's row block I and column block J,
// A[i = l & 15][k = l >> 4] = γ_k·d_k[16 I + i] (formed in double: exact) and B[k = l >> 4][j = l & 15] = d_k[16 J + j];
// columns past D are zero operands (x and μ are both staged as 0 there) and so are frames past the chunk's end (γ = 0, x = 0).
// Result layout: register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15].
__global__ __launch_bounds__(256) void mllt_acc_kernel(AccParams p) {
  __shared__ float x_s[kTile][kXStride];
  __shared__ float w_s[2 * kMaxDim][64];
  __shared__ float post_s[kTile][kMaxGauss];
  __shared__ float fw_s[kTile], fll_s[kTile];
  const int unit = blockIdx.x, group = blockIdx.y, P = p.num_pdfs;
  if (unit >= p.unit_base[P]) return;
  int lo = 0, hi = P;                 // acc_owner, written out (see above): unit_base[lo] <= unit < unit_base[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.unit_base[mid] <= unit) lo = mid; else hi = mid;
  }
  const int pdf = lo, chunk = unit - p.unit_base[pdf];
  const int ng = p.ngauss[pdf], r0 = p.row0[pdf], D = p.D, nb = (D + 15) >> 4;
  if (group * kGroup >= ng) return;
  const int s0 = p.seg_off[pdf] + chunk * kChunk, s1 = min(p.seg_off[pdf + 1], s0 + kChunk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int rounds = (ng + 63) >> 6;
  const bool sums_occ = group == 0;
  float gcv[2];
#pragma unroll
  for (int rnd = 0; rnd < 2; rnd++) gcv[rnd] = lane + 64 * rnd < ng ? p.gc[r0 + lane + 64 * rnd] : 0.0f;

  float mu[kGaussPerWave][kBlocks];
  double4_t acc[kGaussPerWave][kTiles];
  const float *means = p.means + (size_t)p.goff[pdf] * D;
#pragma unroll
  for (int q = 0; q < kGaussPerWave; q++) {
    const int g = group * kGroup + wave + kWaves * q;
#pragma unroll
    for (int b = 0; b < kBlocks; b++) mu[q][b] = g < ng && 16 * b + lc < D ? means[(size_t)g * D + 16 * b + lc] : 0.0f;
#pragma unroll
    for (int t = 0; t < kTiles; t++) acc[q][t] = double4_t{0.0, 0.0, 0.0, 0.0};
  }
  double occ = 0.0, tot_like = 0.0, tot_count = 0.0;
  const int64_t srow0 = p.srow[pdf] + (int64_t)chunk * kSubsPerChunk * ng;
  const int sub0 = p.sub_base[pdf] + chunk * kSubsPerChunk;
  auto flush = [&](int sub) {         // the sub-unit's occ and totals: summed from zero, like a unit of gmm_acc_kernel
    if (tid < ng) p.occ_part[srow0 + (int64_t)sub * ng + tid] = occ;
    if (tid == 255) { p.sub_tot[2 * (size_t)(sub0 + sub)] = tot_like; p.sub_tot[2 * (size_t)(sub0 + sub) + 1] = tot_count; }
    occ = 0.0; tot_like = 0.0; tot_count = 0.0;
  };

  // acc_fetch and acc_stage_store, written out (see above): the next tile's rows are fetched into registers while this tile
  // is worked on, and only stored to LDS at the top of the next round.
  constexpr int kStage = kAccStage;
  float nx[kStage], nw = 0.0f;
  auto fetch = [&](int t0) {
    const int nc = min(kTile, s1 - t0);
#pragma unroll
    for (int i = 0; i < kStage; i++) {
      const int e = tid + 256 * i, t = e / kMaxDim, k = e % kMaxDim;
      nx[i] = t < nc && k < D ? p.feats[(size_t)p.idx[t0 + t] * D + k] : 0.0f;
    }
    if (tid < kTile) nw = tid < nc ? p.weight[p.idx[t0 + tid]] : 0.0f;
  };
  fetch(s0);
  for (int t0 = s0; t0 < s1; t0 += kTile) {
    const int nc = min(kTile, s1 - t0);
    if (sums_occ && t0 > s0 && (t0 - s0) % kSub == 0) flush((t0 - s0) / kSub - 1);
    __syncthreads();                  // the previous tile's moment phase has read x_s, post_s, fw_s, fll_s
#pragma unroll
    for (int i = 0; i < kStage; i++) {
      const int e = tid + 256 * i;
      x_s[e / kMaxDim][e % kMaxDim] = nx[i];
    }
    if (tid < kTile) fw_s[tid] = nw;
    if (t0 + kTile < s1) fetch(t0 + kTile);
    acc_posterior_phase<true>(p.w, p.kpad, r0, ng, D, gcv, t0, s0, nc, x_s, w_s, post_s, fw_s, fll_s, tid, lane, wave, rounds);
    __syncthreads();
    for (int r = 0; r < nc; r += 4) {
      const float *xr = x_s[r + lk];
      float xv[kBlocks];
#pragma unroll
      for (int b = 0; b < kBlocks; b++) xv[b] = xr[16 * b + lc];
#pragma unroll
      for (int q = 0; q < kGaussPerWave; q++) {
        const int g = group * kGroup + wave + kWaves * q;
        if (g < ng) {                   // the same for the whole wavefront
          const double gamma = (double)post_s[r + lk][g];
          double a[kBlocks], b[kBlocks];
#pragma unroll
          for (int k = 0; k < kBlocks; k++) {
            const float d = mllt_acc_diff(xv[k], mu[q][k]);
            a[k] = mllt_acc_left(gamma, d);
            b[k] = (double)d;
          }
#pragma unroll
          for (int I = 0; I < kBlocks; I++) {
            if (I < nb) {               // the same for the whole launch
#pragma unroll
              for (int J = 0; J <= I; J++)
                acc[q][I * (I + 1) / 2 + J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], b[J], acc[q][I * (I + 1) / 2 + J], 0, 0, 0);
            }
          }
        }
      }
    }
    if (sums_occ) {
      if (tid < kMaxGauss)
        for (int t = 0; t < nc; t++) occ += (double)post_s[t][tid];
      if (tid == 255)
        for (int t = 0; t < nc; t++) gmm_acc_total(fw_s[t], fll_s[t], tot_like, tot_count);
    }
  }
  if (sums_occ) flush((s1 - s0 - 1) / kSub);

  const int LT = D * (D + 1) / 2;
  double *out = p.partial + (size_t)(p.prow[pdf] + (int64_t)chunk * ng) * LT;
#pragma unroll
  for (int q = 0; q < kGaussPerWave; q++) {
    const int g = group * kGroup + wave + kWaves * q;
    if (g < ng) {
#pragma unroll
      for (int I = 0; I < kBlocks; I++)
#pragma unroll
        for (int J = 0; J <= I; J++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int i = 16 * I + lk + 4 * r, j = 16 * J + lc;
            if (i < D && j <= i) out[(size_t)g * LT + i * (i + 1) / 2 + j] = acc[q][I * (I + 1) / 2 + J][r];
          }
    }
  }
}

struct ReduceParams {
  int D;
  const int32_t *ngauss; const int32_t *goff; const int32_t *unit_base; const int32_t *sub_base; const int64_t *prow;
  const int64_t *srow;
  const double *partial; const double *occ_part;
  double *occ; double *full;
};

// grid (pdf, tile of 256 elements of its [n_gauss][D·(D + 1)/2] lower triangles): the caller's value (read from the lower
// triangle), then the pdf's partials in chunk order (acc_ordered_sum); the sum goes to (i, j) and (j, i).
__global__ __launch_bounds__(256) void mllt_acc_reduce_kernel(ReduceParams p) {
  const int pdf = blockIdx.x, nu = p.unit_base[pdf + 1] - p.unit_base[pdf];
  if (nu == 0) return;
  const int D = p.D, LT = D * (D + 1) / 2, ng = p.ngauss[pdf], n = ng * LT;
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= n) return;
  const int g = e / LT, rem = e - g * LT;
  int i = (int)((sqrtf(8.0f * (float)rem + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > rem) i--;
  while ((i + 1) * (i + 2) / 2 <= rem) i++;
  const int j = rem - i * (i + 1) / 2;
  double *sq = p.full + (size_t)(p.goff[pdf] + g) * D * D;
  const double *base = p.partial + (size_t)p.prow[pdf] * LT + e;
  const double a = acc_ordered_sum(base, (size_t)n, nu, sq[(size_t)i * D + j]);
  sq[(size_t)i * D + j] = a;
  sq[(size_t)j * D + i] = a;
}

// grid: the pdfs; 128 threads, one per Gaussian: the caller's occ, then the pdf's sub-units in order
__global__ __launch_bounds__(128) void mllt_acc_occ_kernel(ReduceParams p) {
  const int pdf = blockIdx.x, ns = p.sub_base[pdf + 1] - p.sub_base[pdf], ng = p.ngauss[pdf], g = threadIdx.x;
  if (ns == 0 || g >= ng) return;
  const double *base = p.occ_part + p.srow[pdf] + g;
  double a = p.occ[p.goff[pdf] + g];
  for (int s = 0; s < ns; s++) a += base[(size_t)s * ng];
  p.occ[p.goff[pdf] + g] = a;
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_mllt_acc_chunk_frames(void) { return kChunk; }
MFA_API int32_t mfa_mllt_acc_max_dim(void) { return kMaxDim; }

MFA_API int mfa_mllt_acc_batch(mfa_ctx *c, const float *d_feats, int64_t total_frames, const int32_t *d_ali,
                               const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids, const float *d_means,
                               double *d_occ, double *d_full, double *d_tot) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  AccModel am;
  if (const int rc = acc_model_tabs(c, "MLLT statistics", kMaxDim, "three 16-wide blocks of the matrix tiles", kMaxGauss, kChunk,
                                    total_frames, n_tids, am))
    return rc < 0 ? rc : 0;
  if (!d_feats || !d_ali || !d_tid2pdf || !d_tid_weight || !d_means) return c->fail("MLLT statistics: NULL input array");
  if (!d_occ || !d_full || !d_tot) return c->fail("MLLT statistics: NULL accumulator");
  const int D = c->dim, P = c->num_pdfs, max_ng = am.max_ng;
  const int32_t *d_ngauss = am.d_ngauss, *d_goff = am.d_goff;

  const size_t T = (size_t)total_frames, LT = (size_t)D * (D + 1) / 2;
  const size_t units_max = T / kChunk + (size_t)P;                              // Σ ceil(n_p / C) <= floor(T / C) + P
  const size_t subs_max = T / kSub + (size_t)P;
  const size_t rows_max = (T / kChunk + 1) * (size_t)max_ng + (size_t)am.G;        // Σ ceil(n_p / C)·g_p <= (T / C)·max g + Σ g_p
  const size_t srows_max = (T / kSub + 1) * (size_t)max_ng + (size_t)am.G;
  const unsigned end_bit = acc_end_bit((uint64_t)P);
  size_t sort_bytes = 0;
  MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0u, end_bit, c->stream));
  Workspace ws;
  const size_t o_key = ws.take(T * 4), o_key2 = ws.take(T * 4), o_val = ws.take(T * 4), o_val2 = ws.take(T * 4), o_wgt = ws.take(T * 4),
               o_cnt = ws.take(((size_t)P + 1) * 4), o_seg = ws.take(((size_t)P + 1) * 4), o_ub = ws.take(((size_t)P + 1) * 4),
               o_sb = ws.take(((size_t)P + 1) * 4), o_prow = ws.take(((size_t)P + 1) * 8), o_srow = ws.take(((size_t)P + 1) * 8),
               o_stot = ws.take(subs_max * 16), o_opart = ws.take(srows_max * 8), o_part = ws.take(rows_max * LT * 8),
               o_sort = ws.take(sort_bytes);
  if (ws.reserve(c, "the MLLT statistics workspace")) return -1;
  uint32_t *key = ws.at<uint32_t>(o_key), *key2 = ws.at<uint32_t>(o_key2), *val = ws.at<uint32_t>(o_val), *val2 = ws.at<uint32_t>(o_val2);
  float *wgt = ws.at<float>(o_wgt);
  int32_t *cnt = ws.at<int32_t>(o_cnt), *seg = ws.at<int32_t>(o_seg), *ub = ws.at<int32_t>(o_ub), *sb = ws.at<int32_t>(o_sb);
  int64_t *prow = ws.at<int64_t>(o_prow), *srow = ws.at<int64_t>(o_srow);
  double *stot = ws.at<double>(o_stot), *opart = ws.at<double>(o_opart), *part = ws.at<double>(o_part);

  {
    KernelTimer kt(c, MFA_K_MLLT_LOOKUP);
    MFA_HIP_CHECK(c, hipMemsetAsync(cnt, 0, ((size_t)P + 1) * 4, c->stream));
    TidLookupSort s;
    s.key = key; s.val = val; s.num_pdfs = P; s.pdf_count = cnt; s.tid_count = nullptr;
    hipLaunchKernelGGL(fmllr_tid_lookup_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, c->stream, d_ali, total_frames,
                       d_tid2pdf, d_tid_weight, n_tids, (int32_t *)nullptr, wgt, s);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_MLLT_SORT);
    MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(ws.at<char>(o_sort), sort_bytes, key, key2, val, val2, T, 0u, end_bit, c->stream));
    hipLaunchKernelGGL((acc_scan_kernel<5, MlltAccScan>), dim3(1), dim3(256), 0, c->stream, MlltAccScan{cnt, d_ngauss, seg, ub, sb, prow, srow}, P);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_MLLT_SUMS);
    AccParams ap{D, c->kpad, P, c->d_w.ptr<float>(), c->d_gc.ptr<float>(), c->d_row0.ptr<int32_t>(), d_ngauss, d_goff, d_means,
                 d_feats, val2, wgt, seg, ub, sb, prow, srow, part, opart, stot};
    hipLaunchKernelGGL(mllt_acc_kernel, dim3((unsigned)units_max, (unsigned)((max_ng + kGroup - 1) / kGroup)), dim3(256), 0,
                       c->stream, ap);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_MLLT_REDUCE);
    ReduceParams rp{D, d_ngauss, d_goff, ub, sb, prow, srow, part, opart, d_occ, d_full};
    hipLaunchKernelGGL(mllt_acc_reduce_kernel, dim3((unsigned)P, (unsigned)(((size_t)max_ng * LT + 255) / 256)), dim3(256), 0,
                       c->stream, rp);
    hipLaunchKernelGGL(mllt_acc_occ_kernel, dim3((unsigned)P), dim3(128), 0, c->stream, rp);
    hipLaunchKernelGGL(acc_totals_kernel, dim3(1), dim3(256), 0, c->stream, stot, sb, P, d_tot);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  return 0;
}

}  // extern "C"
