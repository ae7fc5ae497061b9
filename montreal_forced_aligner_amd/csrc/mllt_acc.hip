// MLLT statistics on gfx950: the accumulation of the reference's LDA+MLLT stage (MFA/acoustic_modeling/lda.py:122-180 →
// kalpy MlltStatsAccumulator, Kaldi gmm-acc-mllt = MlltAccs::AccumulateFromPosteriors) in the factored form
// G_j = Σ_g inv_var_g[j] · F_g: the device forms the per-Gaussian full second moments F_g = Σ_t γ_tg d_tg d_tgᵀ, the
// contraction over the Gaussians is a float64 GEMM on the host (mllt.py).
// Arithmetic contract: include/mfa_hip.h "MLLT statistics"; the shared arithmetic: mllt_acc_math.hpp over gmm_acc_math.hpp;
// the host twin: mllt_acc_host.cpp.
//
//   lookup   fmllr_tid_lookup_kernel (tid_lookup.hpp), as the GMM statistics run it
//   order    rocPRIM radix_sort_pairs (stable) of (pdf, frame index); one workgroup scans the pdfs' segment starts, their
//            units (chunks of kChunk entries) and sub-units (chunks of kSub entries: the GMM statistics' chunks)
//   sums     mllt_acc_kernel, one workgroup per (unit, group of kGroup Gaussians of the pdf): the posteriors of all the pdf's
//            Gaussians exactly as gmm_acc_kernel forms them, then the group's lower-triangle 16×16 tiles of Σ (γ·d)·dᵀ on
//            the f64 matrix pipe; group 0 also sums occ and the totals per sub-unit
//   reduce   per pdf, the units' partials in chunk order onto the caller's full (both triangles written), the sub-units'
//            onto occ, the totals in (pdf, sub-unit) order
// No floating-point atomics anywhere.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "ctx.hpp"
#include "mllt_acc_math.hpp"
#include "tid_lookup.hpp"

namespace {

constexpr int kSub = 512;        // entries per occ / totals partial: mfa_gmm_acc_chunk_frames(), so that both have that call's bits
constexpr int kSubsPerChunk = 8;
constexpr int kChunk = kSub * kSubsPerChunk;   // entries of a pdf's segment per unit (mfa_mllt_acc_chunk_frames)
constexpr int kTile = 32;        // frames staged in LDS at a time; 8 per wavefront in the posterior phase
constexpr int kMaxGauss = 128;   // two rounds of lane = Gaussian
constexpr int kMaxDim = 48;
constexpr int kXStride = kMaxDim + 1;
constexpr int kBlocks = kMaxDim / 16;                    // 16-wide blocks of the padded feature vector
constexpr int kTiles = kBlocks * (kBlocks + 1) / 2;      // lower-triangle tiles of one Gaussian: 6
constexpr int kWaves = 4;
constexpr int kGaussPerWave = 4;                         // 4 · 6 tiles · 4 doubles = 192 accumulator registers per lane
constexpr int kGroup = kWaves * kGaussPerWave;           // Gaussians of a pdf per workgroup
static_assert(kSub % kTile == 0 && kTile == 4 * 8 && kMaxDim % 16 == 0 && kMaxGauss == 2 * 64 && kMaxGauss % kGroup == 0,
              "mllt_acc_kernel tiling");

typedef double double4_t __attribute__((ext_vector_type(4)));

struct ScanParams {
  const int32_t *cnt; const int32_t *ngauss; int P;
  int32_t *seg_off, *unit_base, *sub_base;    // [P + 1] each: first sorted entry, first unit, first sub-unit of every pdf
  int64_t *prow, *srow;                       // [P + 1]: first partial row (units × Gaussians), first occ row (sub-units × Gaussians)
};

// One workgroup: exclusive scans over the pdfs.
__global__ __launch_bounds__(256) void mllt_acc_scan_kernel(ScanParams p) {
  __shared__ int64_t s[256][5];
  const int P = p.P, per = (P + 255) / 256, a = min(P, (int)threadIdx.x * per), b = min(P, a + per);
  int64_t v[5] = {0, 0, 0, 0, 0};
  auto add = [&](int q) {
    const int64_t c = p.cnt[q], un = (c + kChunk - 1) / kChunk, sn = (c + kSub - 1) / kSub, ng = p.ngauss[q];
    v[0] += c; v[1] += un; v[2] += sn; v[3] += un * ng; v[4] += sn * ng;
  };
  for (int q = a; q < b; q++) add(q);
  for (int k = 0; k < 5; k++) s[threadIdx.x][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 256; i++)
      for (int k = 0; k < 5; k++) { const int64_t t = s[i][k]; s[i][k] = acc[k]; acc[k] += t; }
    p.seg_off[P] = (int32_t)acc[0]; p.unit_base[P] = (int32_t)acc[1]; p.sub_base[P] = (int32_t)acc[2];
    p.prow[P] = acc[3]; p.srow[P] = acc[4];
  }
  __syncthreads();
  for (int k = 0; k < 5; k++) v[k] = s[threadIdx.x][k];
  for (int q = a; q < b; q++) {
    p.seg_off[q] = (int32_t)v[0]; p.unit_base[q] = (int32_t)v[1]; p.sub_base[q] = (int32_t)v[2];
    p.prow[q] = v[3]; p.srow[q] = v[4];
    add(q);
  }
}

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
// Posterior phase: gmm_acc_kernel's, operation for operation — wavefront = 8 frames of the tile, lane = Gaussian (two rounds
// of 64), the same butterfly sums — so that γ, occ and the totals carry that kernel's bits.  Every group forms the posteriors
// of the whole pdf (the softmax needs them all): at most 128 · 2·dim float32 FMAs per frame beside the group's 16 · 6 matrix
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
  int lo = 0, hi = P;                 // unit_base[lo] <= unit < unit_base[hi]
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

  // The gather of a tile is two dependent global loads (sorted index, then the row): the next tile's rows are fetched into
  // registers while this tile is worked on, and only stored to LDS at the top of the next round.
  constexpr int kStage = kTile * kMaxDim / 256;
  static_assert(kStage * 256 == kTile * kMaxDim, "every thread stages the same number of elements");
  float nx[kStage], nw = 0.0f;
  auto fetch = [&](int t0) {
    const int nc = min(kTile, s1 - t0);
#pragma unroll
    for (int i = 0; i < kStage; i++) {
      const int e = tid + 256 * i, t = e / kMaxDim, k = e % kMaxDim;
      nx[i] = t < nc && k < D ? p.feats[(size_t)p.idx[t0 + t] * D + k] : 0.0f;         // columns up to 48 and rows past the end read as 0
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
      } else {                          // a frame past the chunk's end is a zero operand of the last step
        post_s[t][lane] = 0.0f;
        post_s[t][lane + 64] = 0.0f;
      }
    }
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
// triangle), then the pdf's partials in chunk order; the sum goes to (i, j) and (j, i).  The loads of 8 chunks are issued
// together, the additions stay one after the other.
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
  double a = sq[(size_t)i * D + j];
  int ch = 0;
  for (; ch + 8 <= nu; ch += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = base[(size_t)(ch + k) * n];
#pragma unroll
    for (int k = 0; k < 8; k++) a += v[k];
  }
  for (; ch < nu; ch++) a += base[(size_t)ch * n];
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

// one workgroup: the sub-units' totals in order onto the caller's two
__global__ __launch_bounds__(256) void mllt_acc_totals_kernel(const double *sub_tot, const int32_t *sub_base, int P, double *tot) {
  __shared__ double s[256][2];
  const int n = sub_base[P];
  double a = 0.0, b = 0.0;
  if (threadIdx.x == 0) { a = tot[0]; b = tot[1]; }
  for (int u0 = 0; u0 < n; u0 += 256) {
    __syncthreads();
    const int u = u0 + threadIdx.x;
    if (u < n) { s[threadIdx.x][0] = sub_tot[2 * (size_t)u]; s[threadIdx.x][1] = sub_tot[2 * (size_t)u + 1]; }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < min(256, n - u0); i++) { a += s[i][0]; b += s[i][1]; }
  }
  if (threadIdx.x == 0 && n > 0) { tot[0] = a; tot[1] = b; }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

MFA_API int32_t mfa_mllt_acc_chunk_frames(void) { return kChunk; }
MFA_API int32_t mfa_mllt_acc_max_dim(void) { return kMaxDim; }

MFA_API int mfa_mllt_acc_batch(mfa_ctx *c, const float *d_feats, int64_t total_frames, const int32_t *d_ali,
                               const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids, const float *d_means,
                               double *d_occ, double *d_full, double *d_tot) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  const int D = c->dim, P = c->num_pdfs;
  if (D > kMaxDim) return c->fail("MLLT statistics: feature dim %d > %d (three 16-wide blocks of the matrix tiles)", D, kMaxDim);
  int max_ng = 0;
  int64_t G = 0;
  for (int p = 0; p < P; p++) {
    if (c->h_ngauss[p] > kMaxGauss) return c->fail("MLLT statistics: pdf %d has more than %d Gaussians", p, kMaxGauss);
    max_ng = std::max(max_ng, (int)c->h_ngauss[p]);
    G += c->h_ngauss[p];
  }
  if (total_frames <= 0) return 0;
  if (total_frames >= ((int64_t)1 << 31) - kChunk) return c->fail("MLLT statistics: %lld frames in one call (at most 2^31 - %d)", (long long)total_frames, kChunk + 1);
  if (n_tids <= 0) return c->fail("MLLT statistics: empty transition-id table");
  if (!d_feats || !d_ali || !d_tid2pdf || !d_tid_weight || !d_means) return c->fail("MLLT statistics: NULL input array");
  if (!d_occ || !d_full || !d_tot) return c->fail("MLLT statistics: NULL accumulator");
  if (!c->d_acc_tabs) {               // the table of the GMM statistics, built by whichever call comes first
    std::vector<int32_t> tabs((size_t)2 * P + 1);
    int32_t off = 0;
    for (int p = 0; p < P; p++) { tabs[p] = c->h_ngauss[p]; tabs[P + p] = off; off += c->h_ngauss[p]; }
    tabs[2 * P] = off;
    if (dev_upload_commit<MfaHipDev>(c, "the pdfs' Gaussian counts", {{&c->d_acc_tabs, tabs.data(), tabs.size() * 4}})) return -1;
  }
  const int32_t *d_ngauss = c->d_acc_tabs.ptr<int32_t>(), *d_goff = d_ngauss + P;

  const size_t T = (size_t)total_frames, LT = (size_t)D * (D + 1) / 2;
  const size_t units_max = T / kChunk + (size_t)P;                              // Σ ceil(n_p / C) <= floor(T / C) + P
  const size_t subs_max = T / kSub + (size_t)P;
  const size_t rows_max = (T / kChunk + 1) * (size_t)max_ng + (size_t)G;        // Σ ceil(n_p / C)·g_p <= (T / C)·max g + Σ g_p
  const size_t srows_max = (T / kSub + 1) * (size_t)max_ng + (size_t)G;
  const unsigned end_bit = [&] { unsigned b = 1; while (((uint64_t)1 << b) <= (uint64_t)P) b++; return b; }();
  size_t sort_bytes = 0;
  MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0u, end_bit, c->stream));
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o = align256(o + bytes); return at; };
  const size_t o_key = take(T * 4), o_key2 = take(T * 4), o_val = take(T * 4), o_val2 = take(T * 4), o_wgt = take(T * 4),
               o_cnt = take(((size_t)P + 1) * 4), o_seg = take(((size_t)P + 1) * 4), o_ub = take(((size_t)P + 1) * 4),
               o_sb = take(((size_t)P + 1) * 4), o_prow = take(((size_t)P + 1) * 8), o_srow = take(((size_t)P + 1) * 8),
               o_stot = take(subs_max * 16), o_opart = take(srows_max * 8), o_part = take(rows_max * LT * 8),
               o_sort = take(sort_bytes);
  if (c->d_ws.reserve(c, o, "the MLLT statistics workspace")) return -1;
  char *ws = c->d_ws.ptr<char>();
  uint32_t *key = (uint32_t *)(ws + o_key), *key2 = (uint32_t *)(ws + o_key2), *val = (uint32_t *)(ws + o_val), *val2 = (uint32_t *)(ws + o_val2);
  float *wgt = (float *)(ws + o_wgt);
  int32_t *cnt = (int32_t *)(ws + o_cnt), *seg = (int32_t *)(ws + o_seg), *ub = (int32_t *)(ws + o_ub), *sb = (int32_t *)(ws + o_sb);
  int64_t *prow = (int64_t *)(ws + o_prow), *srow = (int64_t *)(ws + o_srow);
  double *stot = (double *)(ws + o_stot), *opart = (double *)(ws + o_opart), *part = (double *)(ws + o_part);

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
    MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(ws + o_sort, sort_bytes, key, key2, val, val2, T, 0u, end_bit, c->stream));
    ScanParams sp{cnt, d_ngauss, P, seg, ub, sb, prow, srow};
    hipLaunchKernelGGL(mllt_acc_scan_kernel, dim3(1), dim3(256), 0, c->stream, sp);
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
    hipLaunchKernelGGL(mllt_acc_totals_kernel, dim3(1), dim3(256), 0, c->stream, stot, sb, P, d_tot);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  return 0;
}

}  // extern "C"
