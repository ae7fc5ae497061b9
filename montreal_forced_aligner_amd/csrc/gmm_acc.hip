// GMM sufficient statistics on gfx950: the E-step of `mfa adapt` and of every training stage of the reference
// (AccStatsFunction → kalpy GmmStatsAccumulator, Kaldi gmm-acc-stats-ali / AccumAmDiagGmm::AccumulateForGmm).
// Arithmetic contract: include/mfa_hip.h "GMM statistics"; the shared arithmetic: gmm_acc_math.hpp; the host twin:
// gmm_acc_host.cpp.
//
// The five steps are the segment skeleton of acc_segments.hpp, the posterior phase is acc_posterior.hpp's:
//   lookup   fmllr_tid_lookup_kernel (tid_lookup.hpp): per frame the sort key (pdf; num_pdfs = takes no part), the pdfs'
//            frame counts and the transition-id counts
//   order    rocPRIM radix_sort_pairs (stable) of (pdf, frame index)
//   scan     segment starts, first unit and first partial row of every pdf
//   sums     gmm_acc_kernel, one workgroup per unit = (pdf, chunk of kChunk consecutive entries of its segment)
//   reduce   per pdf, the units' partials in chunk order into the caller's accumulators; the two totals in unit order
// mfa_gmm_acc_twofeats_batch (Kaldi gmm-acc-stats-twofeats: the alignment model of the SAT stage) is the same five steps with
// gmm_acc_kernel<true>: posteriors from one feature matrix, the sums' x from a second one of the same frames.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "acc_posterior.hpp"
#include "acc_segments.hpp"
#include "ctx.hpp"
#include "tid_lookup.hpp"

namespace {

constexpr int kChunk = 512;      // C: entries of a pdf's segment per unit (mfa_gmm_acc_chunk_frames)
constexpr int kTile = kAccTile, kMaxGauss = kAccMaxGauss, kXStride = kAccXStride;
constexpr int kMaxDim = kAccMaxDim;   // a thread owns columns l, l + 16, l + 32 (l < 16) of 8 Gaussians
constexpr int kColsPerThread = kMaxDim / 16, kGaussPerThread = kMaxGauss / 16;
static_assert(kChunk % kTile == 0 && kMaxDim % 16 == 0, "gmm_acc_kernel tiling");

struct AccParams {
  int D, kpad, num_pdfs;
  const float *w; const float *gc; const int32_t *row0;     // packed model (gmm_pack.hpp layout)
  const int32_t *ngauss;                                    // [num_pdfs] Gaussians per pdf
  const float *feats; const uint32_t *idx; const float *weight;   // idx: frame indices ordered by pdf
  const int32_t *seg_off; const int32_t *unit_base; const int64_t *prow;   // [num_pdfs + 1] each
  double *partial;     // per unit [n_gauss][2·D + 1]: occupancy, first-order sums, second-order sums
  double *unit_tot;    // per unit {Σ w·loglike, Σ w}
};
// The two-feature form's arguments, in a type of its own: the one-feature kernel's argument block, and with it the
// compiler's register allocation, stay what they were.
struct AccParams2 : AccParams {
  const float *feats_sum;     // the rows the sums are formed from
};
template <bool kTwoFeats> struct AccParamsOf { using type = AccParams; };
template <> struct AccParamsOf<true> { using type = AccParams2; };

// acc_scan_kernel<3> over the pdfs: frames, units, partial rows = units × Gaussians
struct GmmAccScan {
  const int32_t *cnt; const int32_t *ngauss;
  int32_t *seg_off; int32_t *unit_base; int64_t *prow;
  __device__ void add(int q, int64_t (&v)[3]) const {
    const int64_t c = cnt[q], un = (c + kChunk - 1) / kChunk;
    v[0] += c; v[1] += un; v[2] += un * ngauss[q];
  }
  __device__ void put(int q, const int64_t (&v)[3]) const { seg_off[q] = (int32_t)v[0]; unit_base[q] = (int32_t)v[1]; prow[q] = v[2]; }
};

// grid: an upper bound of the units (the true count is unit_base[num_pdfs], known on the device only); 256 threads.
// Posterior phase: acc_posterior.hpp.  Sum phase: thread (gg = tid / 16, l = tid % 16) keeps mean / var of Gaussians gg + 16 j
// (j < 8) in columns l + 16 c (c < 3) in registers over the whole chunk: 48 double FMAs per frame at 128 Gaussians,
// 6 · ceil(n / 16) in general.
// kTwoFeats (mfa_gmm_acc_twofeats_batch): the posterior phase reads the rows of p.feats as ever, the sum phase the same
// frames' rows of p.feats_sum, gathered with them and staged in a tile of their own (x2_s: 6 272 B more LDS, 53 760 B in all;
// three workgroups of a CU's 160 KB either way).  Without it the kernel is the one-feature kernel, instruction for instruction.
template <bool kTwoFeats>
__global__ __launch_bounds__(256) void gmm_acc_kernel(typename AccParamsOf<kTwoFeats>::type p) {
  __shared__ float x_s[kTile][kXStride];
  __shared__ float x2_s[kTwoFeats ? kTile : 1][kTwoFeats ? kXStride : 1];
  __shared__ float w_s[2 * kMaxDim][64];
  __shared__ float post_s[kTile][kMaxGauss];
  __shared__ float fw_s[kTile], fll_s[kTile];
  const int unit = blockIdx.x, P = p.num_pdfs;
  if (unit >= p.unit_base[P]) return;
  const int pdf = acc_owner(p.unit_base, P, unit), chunk = unit - p.unit_base[pdf];
  const int ng = p.ngauss[pdf], r0 = p.row0[pdf], D = p.D;
  const int s0 = p.seg_off[pdf] + chunk * kChunk, s1 = min(p.seg_off[pdf + 1], s0 + kChunk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, gg = tid >> 4, l = tid & 15;
  const int rounds = (ng + 63) >> 6;
  float gcv[2];
  acc_gconsts(p.gc, r0, ng, lane, gcv);
  double m[kGaussPerThread][kColsPerThread], v[kGaussPerThread][kColsPerThread];
#pragma unroll
  for (int j = 0; j < kGaussPerThread; j++)
#pragma unroll
    for (int c = 0; c < kColsPerThread; c++) { m[j][c] = 0.0; v[j][c] = 0.0; }
  double occ = 0.0, tot_like = 0.0, tot_count = 0.0;

  const float *feats_sum = nullptr;
  float (*x2)[kXStride] = nullptr;
  if constexpr (kTwoFeats) { feats_sum = p.feats_sum; x2 = x2_s; }
  AccStaged<kTwoFeats> next;          // the next tile's rows: in flight while this tile is worked on
  acc_fetch(next, p.feats, feats_sum, p.idx, p.weight, D, s0, s1, tid);
  for (int t0 = s0; t0 < s1; t0 += kTile) {
    const int nc = min(kTile, s1 - t0);
    __syncthreads();                  // the previous tile's sum phase has read x_s, post_s, fw_s, fll_s
    acc_stage_store(next, x_s, x2, fw_s, tid);
    if (t0 + kTile < s1) acc_fetch(next, p.feats, feats_sum, p.idx, p.weight, D, t0 + kTile, s1, tid);
    acc_posterior_phase<false>(p.w, p.kpad, r0, ng, D, gcv, t0, s0, nc, x_s, w_s, post_s, fw_s, fll_s, tid, lane, wave, rounds);
    __syncthreads();
    for (int t = 0; t < nc; t++) {
      float xf[kColsPerThread];
#pragma unroll
      for (int c = 0; c < kColsPerThread; c++) xf[c] = kTwoFeats ? x2_s[t][l + 16 * c] : x_s[t][l + 16 * c];
#pragma unroll
      for (int j = 0; j < kGaussPerThread; j++) {
        if (16 * j < ng) {              // the same for the whole workgroup
          const double gamma = (double)post_s[t][gg + 16 * j];
#pragma unroll
          for (int c = 0; c < kColsPerThread; c++) gmm_acc_add(gamma, xf[c], m[j][c], v[j][c]);
        }
      }
    }
    acc_occ_totals(post_s, fw_s, fll_s, nc, tid, occ, tot_like, tot_count);
  }

  const int W = 2 * D + 1;
  double *out = p.partial + (size_t)(p.prow[pdf] + (int64_t)chunk * ng) * W;
#pragma unroll
  for (int j = 0; j < kGaussPerThread; j++) {
    const int g = gg + 16 * j;
    if (g < ng) {
#pragma unroll
      for (int c = 0; c < kColsPerThread; c++) {
        const int k = l + 16 * c;
        if (k < D) { out[(size_t)g * W + 1 + k] = m[j][c]; out[(size_t)g * W + 1 + D + k] = v[j][c]; }
      }
    }
  }
  if (tid < ng) out[(size_t)tid * W] = occ;
  if (tid == 255) { p.unit_tot[2 * (size_t)unit] = tot_like; p.unit_tot[2 * (size_t)unit + 1] = tot_count; }
}

struct ReduceParams {
  int D;
  const int32_t *ngauss; const int32_t *goff; const int32_t *unit_base; const int64_t *prow;
  const double *partial;
  double *occ; double *mean; double *var;
};

// grid (pdf, tile of 256 elements of its [n_gauss][2·D + 1] sums): the caller's value, then the pdf's partials in chunk
// order (acc_ordered_sum).
__global__ __launch_bounds__(256) void gmm_acc_reduce_kernel(ReduceParams p) {
  const int pdf = blockIdx.x, nu = p.unit_base[pdf + 1] - p.unit_base[pdf];
  if (nu == 0) return;
  const int D = p.D, W = 2 * D + 1, ng = p.ngauss[pdf], n = ng * W;
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= n) return;
  const size_t g0 = (size_t)p.goff[pdf];
  const double *base = p.partial + (size_t)p.prow[pdf] * W + e;
  const int g = e / W, c = e % W;
  double *dst = c == 0 ? p.occ + g0 + g : c <= D ? p.mean + (g0 + g) * D + (c - 1) : p.var + (g0 + g) * D + (c - 1 - D);
  *dst = acc_ordered_sum(base, (size_t)n, nu, *dst);
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_gmm_acc_chunk_frames(void) { return kChunk; }
MFA_API int32_t mfa_gmm_acc_max_dim(void) { return kMaxDim; }

}  // extern "C"

// d_feats_sum NULL: the one-feature form.
static int gmm_acc_run(mfa_ctx *c, const float *d_feats, const float *d_feats_sum, int64_t total_frames, const int32_t *d_ali,
                       const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids, double *d_occ, double *d_mean,
                       double *d_var, double *d_tot, int64_t *d_tid_count) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  AccModel am;
  if (const int rc = acc_model_tabs(c, "GMM statistics", kMaxDim, "a thread of the sum kernel owns 3 of 48 columns", kMaxGauss, kChunk,
                                    total_frames, n_tids, am))
    return rc < 0 ? rc : 0;
  const int D = c->dim, P = c->num_pdfs, max_ng = am.max_ng;
  const int32_t *d_ngauss = am.d_ngauss, *d_goff = am.d_goff;

  const size_t T = (size_t)total_frames, W = 2 * (size_t)D + 1;
  const size_t units_max = T / kChunk + (size_t)P;                              // Σ ceil(n_p / C) <= floor(T / C) + P
  const size_t rows_max = (T / kChunk + 1) * (size_t)max_ng + (size_t)am.G;     // Σ ceil(n_p / C)·g_p <= (T / C)·max g + Σ g_p
  const unsigned end_bit = acc_end_bit((uint64_t)P);
  size_t sort_bytes = 0;
  MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0u, end_bit, c->stream));
  Workspace ws;
  const size_t o_key = ws.take(T * 4), o_key2 = ws.take(T * 4), o_val = ws.take(T * 4), o_val2 = ws.take(T * 4), o_wgt = ws.take(T * 4),
               o_cnt = ws.take(((size_t)P + 1) * 4), o_seg = ws.take(((size_t)P + 1) * 4), o_ub = ws.take(((size_t)P + 1) * 4),
               o_prow = ws.take(((size_t)P + 1) * 8), o_utot = ws.take(units_max * 16), o_part = ws.take(rows_max * W * 8),
               o_sort = ws.take(sort_bytes);
  if (ws.reserve(c, "the GMM statistics workspace")) return -1;
  uint32_t *key = ws.at<uint32_t>(o_key), *key2 = ws.at<uint32_t>(o_key2), *val = ws.at<uint32_t>(o_val), *val2 = ws.at<uint32_t>(o_val2);
  float *wgt = ws.at<float>(o_wgt);
  int32_t *cnt = ws.at<int32_t>(o_cnt), *seg = ws.at<int32_t>(o_seg), *ub = ws.at<int32_t>(o_ub);
  int64_t *prow = ws.at<int64_t>(o_prow);
  double *utot = ws.at<double>(o_utot), *part = ws.at<double>(o_part);

  {
    KernelTimer kt(c, MFA_K_ACC_LOOKUP);
    MFA_HIP_CHECK(c, hipMemsetAsync(cnt, 0, ((size_t)P + 1) * 4, c->stream));
    TidLookupSort s;
    s.key = key; s.val = val; s.num_pdfs = P; s.pdf_count = cnt; s.tid_count = (unsigned long long *)d_tid_count;
    hipLaunchKernelGGL(fmllr_tid_lookup_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, c->stream, d_ali, total_frames,
                       d_tid2pdf, d_tid_weight, n_tids, (int32_t *)nullptr, wgt, s);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_ACC_SORT);
    MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(ws.at<char>(o_sort), sort_bytes, key, key2, val, val2, T, 0u, end_bit, c->stream));
    hipLaunchKernelGGL((acc_scan_kernel<3, GmmAccScan>), dim3(1), dim3(256), 0, c->stream, GmmAccScan{cnt, d_ngauss, seg, ub, prow}, P);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_ACC_SUMS);
    AccParams ap{D, c->kpad, P, c->d_w.ptr<float>(), c->d_gc.ptr<float>(), c->d_row0.ptr<int32_t>(), d_ngauss,
                 d_feats, val2, wgt, seg, ub, prow, part, utot};
    if (d_feats_sum) {
      AccParams2 ap2;
      static_cast<AccParams &>(ap2) = ap;
      ap2.feats_sum = d_feats_sum;
      hipLaunchKernelGGL(gmm_acc_kernel<true>, dim3((unsigned)units_max), dim3(256), 0, c->stream, ap2);
    } else {
      hipLaunchKernelGGL(gmm_acc_kernel<false>, dim3((unsigned)units_max), dim3(256), 0, c->stream, ap);
    }
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_ACC_REDUCE);
    ReduceParams rp{D, d_ngauss, d_goff, ub, prow, part, d_occ, d_mean, d_var};
    hipLaunchKernelGGL(gmm_acc_reduce_kernel, dim3((unsigned)P, (unsigned)((max_ng * (2 * D + 1) + 255) / 256)), dim3(256), 0, c->stream, rp);
    hipLaunchKernelGGL(acc_totals_kernel, dim3(1), dim3(256), 0, c->stream, utot, ub, P, d_tot);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  return 0;
}

extern "C" {

MFA_API int mfa_gmm_acc_batch(mfa_ctx *c, const float *d_feats, int64_t total_frames, const int32_t *d_ali,
                              const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids, double *d_occ, double *d_mean,
                              double *d_var, double *d_tot, int64_t *d_tid_count) {
  return gmm_acc_run(c, d_feats, nullptr, total_frames, d_ali, d_tid2pdf, d_tid_weight, n_tids, d_occ, d_mean, d_var, d_tot, d_tid_count);
}

MFA_API int mfa_gmm_acc_twofeats_batch(mfa_ctx *c, const float *d_feats_post, const float *d_feats_sum, int64_t total_frames,
                                       const int32_t *d_ali, const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids,
                                       double *d_occ, double *d_mean, double *d_var, double *d_tot, int64_t *d_tid_count) {
  if (!d_feats_sum && total_frames > 0) return c->fail("GMM statistics, two features: no matrix to form the sums from (d_feats_sum is NULL)");
  return gmm_acc_run(c, d_feats_post, d_feats_sum, total_frames, d_ali, d_tid2pdf, d_tid_weight, n_tids, d_occ, d_mean, d_var, d_tot, d_tid_count);
}

}  // extern "C"
