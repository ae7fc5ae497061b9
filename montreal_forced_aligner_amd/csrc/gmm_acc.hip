// GMM sufficient statistics on gfx950: the E-step of `mfa adapt` and of every training stage of the reference
// (AccStatsFunction → kalpy GmmStatsAccumulator, Kaldi gmm-acc-stats-ali / AccumAmDiagGmm::AccumulateForGmm).
// Arithmetic contract: include/mfa_hip.h "GMM statistics"; the shared arithmetic: gmm_acc_math.hpp; the host twin:
// gmm_acc_host.cpp.
//
//   lookup   fmllr_tid_lookup_kernel (tid_lookup.hpp): per frame the sort key (pdf; num_pdfs = takes no part), the pdfs'
//            frame counts and the transition-id counts (integer atomics: exact)
//   order    rocPRIM radix_sort_pairs (stable) of (pdf, frame index): every pdf's segment lists its frames in ascending
//            frame index, so every sum below is a function of the input alone
//   scan     one workgroup: segment starts, first unit and first partial row of every pdf
//   sums     gmm_acc_kernel, one workgroup per unit = (pdf, chunk of kChunk consecutive entries of its segment)
//   reduce   per pdf, the units' partials in chunk order into the caller's accumulators; the two totals in unit order
// No floating-point atomics anywhere.
// mfa_gmm_acc_twofeats_batch (Kaldi gmm-acc-stats-twofeats: the alignment model of the SAT stage) is the same five steps with
// gmm_acc_kernel<true>: posteriors from one feature matrix, the sums' x from a second one of the same frames.
#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "ctx.hpp"
#include "gmm_acc_math.hpp"
#include "tid_lookup.hpp"

namespace {

constexpr int kChunk = 512;      // C: entries of a pdf's segment per unit (mfa_gmm_acc_chunk_frames)
constexpr int kTile = 32;        // frames staged in LDS at a time; 8 per wavefront in the posterior phase
constexpr int kMaxGauss = 128;   // two rounds of lane = Gaussian
constexpr int kMaxDim = 48;      // a thread owns columns l, l + 16, l + 32 (l < 16) of 8 Gaussians
constexpr int kXStride = kMaxDim + 1;
constexpr int kColsPerThread = kMaxDim / 16, kGaussPerThread = kMaxGauss / 16;
static_assert(kChunk % kTile == 0 && kTile == 4 * 8 && kMaxDim % 16 == 0 && kMaxGauss == 2 * 64, "gmm_acc_kernel tiling");

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

// One workgroup: exclusive scans over the pdfs of (frames, units, partial rows = units × Gaussians).
__global__ __launch_bounds__(256) void gmm_acc_scan_kernel(const int32_t *cnt, const int32_t *ngauss, int P, int32_t *seg_off,
                                                           int32_t *unit_base, int64_t *prow) {
  __shared__ int32_t sf[256], su[256];
  __shared__ int64_t sr[256];
  const int per = (P + 255) / 256, a = min(P, (int)threadIdx.x * per), b = min(P, a + per);
  int32_t f = 0, u = 0;
  int64_t r = 0;
  for (int p = a; p < b; p++) { const int un = (cnt[p] + kChunk - 1) / kChunk; f += cnt[p]; u += un; r += (int64_t)un * ngauss[p]; }
  sf[threadIdx.x] = f; su[threadIdx.x] = u; sr[threadIdx.x] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t af = 0, au = 0;
    int64_t ar = 0;
    for (int i = 0; i < 256; i++) {
      const int32_t tf = sf[i], tu = su[i];
      const int64_t tr = sr[i];
      sf[i] = af; su[i] = au; sr[i] = ar;
      af += tf; au += tu; ar += tr;
    }
    seg_off[P] = af; unit_base[P] = au; prow[P] = ar;
  }
  __syncthreads();
  f = sf[threadIdx.x]; u = su[threadIdx.x]; r = sr[threadIdx.x];
  for (int p = a; p < b; p++) {
    seg_off[p] = f; unit_base[p] = u; prow[p] = r;
    const int un = (cnt[p] + kChunk - 1) / kChunk;
    f += cnt[p]; u += un; r += (int64_t)un * ngauss[p];
  }
}

// grid: an upper bound of the units (the true count is unit_base[num_pdfs], known on the device only); 256 threads.
// Posterior phase: wavefront = 8 frames of the tile, lane = Gaussian (two rounds of 64), weights of the round in LDS as
// [k][Gaussian].  Sum phase: thread (gg = tid / 16, l = tid % 16) keeps mean / var of Gaussians gg + 16 j (j < 8) in columns
// l + 16 c (c < 3) in registers over the whole chunk: 48 double FMAs per frame at 128 Gaussians, 6 · ceil(n / 16) in general.
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
  int lo = 0, hi = P;                 // unit_base[lo] <= unit < unit_base[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.unit_base[mid] <= unit) lo = mid; else hi = mid;
  }
  const int pdf = lo, chunk = unit - p.unit_base[pdf];
  const int ng = p.ngauss[pdf], r0 = p.row0[pdf], D = p.D;
  const int s0 = p.seg_off[pdf] + chunk * kChunk, s1 = min(p.seg_off[pdf + 1], s0 + kChunk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, gg = tid >> 4, l = tid & 15;
  const int rounds = (ng + 63) >> 6;
  float gcv[2];
#pragma unroll
  for (int rnd = 0; rnd < 2; rnd++) gcv[rnd] = lane + 64 * rnd < ng ? p.gc[r0 + lane + 64 * rnd] : 0.0f;
  double m[kGaussPerThread][kColsPerThread], v[kGaussPerThread][kColsPerThread];
#pragma unroll
  for (int j = 0; j < kGaussPerThread; j++)
#pragma unroll
    for (int c = 0; c < kColsPerThread; c++) { m[j][c] = 0.0; v[j][c] = 0.0; }
  double occ = 0.0, tot_like = 0.0, tot_count = 0.0;

  // The gather of a tile is two dependent global loads (sorted index, then the row): the next tile's rows are fetched into
  // registers while this tile is worked on, and only stored to LDS at the top of the next round.
  constexpr int kStage = kTile * kMaxDim / 256;
  static_assert(kStage * 256 == kTile * kMaxDim, "every thread stages the same number of elements");
  float nx[kStage], nx2[kTwoFeats ? kStage : 1], nw = 0.0f;
  auto fetch = [&](int t0) {
    const int nc = min(kTile, s1 - t0);
#pragma unroll
    for (int i = 0; i < kStage; i++) {
      const int e = tid + 256 * i, t = e / kMaxDim, k = e % kMaxDim;
      if constexpr (kTwoFeats) {
        const bool in = t < nc && k < D;
        const size_t at = in ? (size_t)p.idx[t0 + t] * D + k : 0;
        nx[i] = in ? p.feats[at] : 0.0f;
        nx2[i] = in ? p.feats_sum[at] : 0.0f;
      } else {
        nx[i] = t < nc && k < D ? p.feats[(size_t)p.idx[t0 + t] * D + k] : 0.0f;       // columns up to 48 read as 0
      }
    }
    if (tid < kTile) nw = tid < nc ? p.weight[p.idx[t0 + tid]] : 0.0f;
  };
  fetch(s0);
  for (int t0 = s0; t0 < s1; t0 += kTile) {
    const int nc = min(kTile, s1 - t0);
    __syncthreads();                  // the previous tile's sum phase has read x_s, post_s, fw_s, fll_s
#pragma unroll
    for (int i = 0; i < kStage; i++) {
      const int e = tid + 256 * i;
      x_s[e / kMaxDim][e % kMaxDim] = nx[i];
      if constexpr (kTwoFeats) x2_s[e / kMaxDim][e % kMaxDim] = nx2[i];
    }
    if (tid < kTile) fw_s[tid] = nw;
    if (t0 + kTile < s1) fetch(t0 + kTile);
    float ll[8][2];
#pragma unroll
    for (int rnd = 0; rnd < 2; rnd++) {
      if (rnd < rounds) {
        if (rounds > 1 || t0 == s0) {   // one round: its weights stay for the whole chunk
          __syncthreads();              // the other round's readers are done
          for (int i = tid; i < 2 * D * 64; i += 256) {
            const int k = i >> 6, g = (i & 63) + 64 * rnd;
            w_s[k][i & 63] = g < ng ? p.w[mfa_packed_offset(r0 + g, k, p.kpad)] : 0.0f;
          }
        }
        __syncthreads();
        const bool have = lane + 64 * rnd < ng;
        float blk[8];                   // rows past the chunk's end are zeros: computed, never used
        gmm_acc_loglike_block<8>(gcv[rnd], D, &w_s[0][lane], 64, &w_s[D][lane], 64, x_s[wave * 8], kXStride, blk);
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
      }
    }
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
    if (tid < kMaxGauss)
      for (int t = 0; t < nc; t++) occ += (double)post_s[t][tid];
    if (tid == 255)
      for (int t = 0; t < nc; t++) gmm_acc_total(fw_s[t], fll_s[t], tot_like, tot_count);
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
// order.  The loads of 8 chunks are issued together (a pdf that holds a seventh of the corpus has thousands of chunks and one
// thread per element to walk them); the additions stay one after the other, in chunk order.
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
  double a = *dst;
  int ch = 0;
  for (; ch + 8 <= nu; ch += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = base[(size_t)(ch + i) * n];
#pragma unroll
    for (int i = 0; i < 8; i++) a += v[i];
  }
  for (; ch < nu; ch++) a += base[(size_t)ch * n];
  *dst = a;
}

// one workgroup: the units' totals in unit order onto the caller's two
__global__ __launch_bounds__(256) void gmm_acc_totals_kernel(const double *unit_tot, const int32_t *unit_base, int P, double *tot) {
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

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

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
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  const int D = c->dim, P = c->num_pdfs;
  if (D > kMaxDim) return c->fail("GMM statistics: feature dim %d > %d (a thread of the sum kernel owns 3 of 48 columns)", D, kMaxDim);
  int max_ng = 0;
  int64_t G = 0;
  for (int p = 0; p < P; p++) {
    if (c->h_ngauss[p] > kMaxGauss) return c->fail("GMM statistics: pdf %d has more than %d Gaussians", p, kMaxGauss);
    max_ng = std::max(max_ng, (int)c->h_ngauss[p]);
    G += c->h_ngauss[p];
  }
  if (total_frames <= 0) return 0;
  if (total_frames >= ((int64_t)1 << 31) - kChunk) return c->fail("GMM statistics: %lld frames in one call (at most 2^31 - %d)", (long long)total_frames, kChunk + 1);
  if (n_tids <= 0) return c->fail("GMM statistics: empty transition-id table");
  if (!c->d_acc_tabs) {
    std::vector<int32_t> tabs((size_t)2 * P + 1);
    int32_t off = 0;
    for (int p = 0; p < P; p++) { tabs[p] = c->h_ngauss[p]; tabs[P + p] = off; off += c->h_ngauss[p]; }
    tabs[2 * P] = off;
    if (dev_upload_commit<MfaHipDev>(c, "the pdfs' Gaussian counts", {{&c->d_acc_tabs, tabs.data(), tabs.size() * 4}})) return -1;
  }
  const int32_t *d_ngauss = c->d_acc_tabs.ptr<int32_t>(), *d_goff = d_ngauss + P;

  const size_t T = (size_t)total_frames, W = 2 * (size_t)D + 1;
  const size_t units_max = T / kChunk + (size_t)P;                              // Σ ceil(n_p / C) <= floor(T / C) + P
  const size_t rows_max = (T / kChunk + 1) * (size_t)max_ng + (size_t)G;        // Σ ceil(n_p / C)·g_p <= (T / C)·max g + Σ g_p
  const unsigned end_bit = [&] { unsigned b = 1; while (((uint64_t)1 << b) <= (uint64_t)P) b++; return b; }();
  size_t sort_bytes = 0;
  MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0u, end_bit, c->stream));
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
  const size_t o_key = take(T * 4), o_key2 = take(T * 4), o_val = take(T * 4), o_val2 = take(T * 4), o_wgt = take(T * 4),
               o_cnt = take(((size_t)P + 1) * 4), o_seg = take(((size_t)P + 1) * 4), o_ub = take(((size_t)P + 1) * 4),
               o_prow = take(((size_t)P + 1) * 8), o_utot = take(units_max * 16), o_part = take(rows_max * W * 8),
               o_sort = take(sort_bytes);
  if (c->d_ws.reserve(c, o, "the GMM statistics workspace")) return -1;
  char *ws = c->d_ws.ptr<char>();
  uint32_t *key = (uint32_t *)(ws + o_key), *key2 = (uint32_t *)(ws + o_key2), *val = (uint32_t *)(ws + o_val), *val2 = (uint32_t *)(ws + o_val2);
  float *wgt = (float *)(ws + o_wgt);
  int32_t *cnt = (int32_t *)(ws + o_cnt), *seg = (int32_t *)(ws + o_seg), *ub = (int32_t *)(ws + o_ub);
  int64_t *prow = (int64_t *)(ws + o_prow);
  double *utot = (double *)(ws + o_utot), *part = (double *)(ws + o_part);

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
    MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(ws + o_sort, sort_bytes, key, key2, val, val2, T, 0u, end_bit, c->stream));
    hipLaunchKernelGGL(gmm_acc_scan_kernel, dim3(1), dim3(256), 0, c->stream, cnt, d_ngauss, P, seg, ub, prow);
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
    hipLaunchKernelGGL(gmm_acc_totals_kernel, dim3(1), dim3(256), 0, c->stream, utot, ub, P, d_tot);
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
