// The silhouette stage on gfx950: the last step of the reference's cluster_matrix (MFA/diarization/multiprocessing.py), which
// scores every clustering with metrics.silhouette_score, on N points whose columns are ordered by cluster, with no N × N array
// stored.  Arithmetic contract: include/mfa_hip.h "Silhouette"; the shared rules: silhouette_math.hpp; the sweep and its
// silhouette consumer: plda.hip (pair_sweep.hpp); the host twin: silhouette_host.cpp.
//
//   prepare    the pair form's pair_prepare_kernel (hdbscan.hip) and pair_pack_kernel (plda.hip), as the HDBSCAN stage runs them
//   offsets    sil_offsets_kernel, a thread per cluster and per point: the checks of the column ranges (a flag, a plain store of
//              the same value) and every point's cluster by a search that stays inside the array on any input
//   sweep      the sweep's silhouette consumer, one column pass: a, b, bj and s of every row
// No atomics; every sum has a fixed order: two calls on the same input give the same bits, whatever MFA_PLDA_PASS_COLS says.
#include "pair_sweep.hpp"
#include "silhouette_math.hpp"

namespace {

// flags[1] |= offsets that are not 0 = off[0] < off[1] < … < off[C] = N.
__global__ __launch_bounds__(256) void sil_offsets_kernel(const int32_t *off, int32_t C, int64_t N, int32_t *own, int32_t *flags) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < C && !sil_offset_ok(off[t], off[t + 1], (int32_t)t, C, N)) flags[1] = 1;
  if (t < N) own[t] = sil_cluster_of(off, C, t);
}

int refuse(mfa_ctx *c, const char *who, int rc, int D, int C, long long n) {
  switch (rc) {
    case -2: return c->fail("%s: dimension %d (1 to %d)", who, D, kPldaMaxDim);
    case -5: return c->fail("%s: %lld points in one call (fewer than 2^31)", who, n);
    case -6: return c->fail("%s: %d clusters for %lld points (2 to the number of points)", who, C, n);
    default: return c->fail("%s: a negative count", who);
  }
}

}  // namespace

extern "C" MFA_API int mfa_silhouette_batch(mfa_ctx *c, const double *d_x, int64_t N, int32_t D, int32_t metric, const double *d_psi,
                                            const int32_t *d_off, int32_t C, double *d_sil, double *d_a, double *d_b, int32_t *d_bj,
                                            double *d_v) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "silhouette";
  if (!plda_metric_ok(metric)) return c->fail("%s: metric %d (0 plda, 1 euclidean, 2 dot)", who, metric);
  const int rc = sil_check_shape(D, N, C);
  if (rc) return refuse(c, who, rc, D, C, (long long)N);
  if (N == 0) return 0;
  if (!d_x || !d_off || !d_sil || (metric == kMetricPlda && !d_psi)) return c->fail("%s: NULL array", who);
  MfaPairSweep op;
  if (mfa_pair_lay_out(c, op, N, D, 0)) return -1;
  const size_t o_y = op.ws.take((size_t)N * D * 8), o_q = op.ws.take((size_t)N * 8), o_own = op.ws.take((size_t)N * 4), o_flags = op.ws.take(8);
  if (op.ws.reserve(c, "the silhouette workspace")) return -1;
  double *y = op.ws.at<double>(o_y), *q = op.ws.at<double>(o_q);
  int32_t *own = op.ws.at<int32_t>(o_own), *flags = op.ws.at<int32_t>(o_flags);
  if (mfa_pair_prepare(c, d_x, metric, d_psi, N, D, y, q, flags)) return -1;
  {
    KernelTimer kt(c, MFA_K_SIL_OFFSETS);
    hipLaunchKernelGGL(sil_offsets_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_off, C, N, own, flags);   // C <= N
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "sil_offsets_kernel N=%lld C=%d", (long long)N, C);
  }
  int32_t h_flags[2] = {0, 0};
  MFA_HIP_CHECK(c, hipMemcpyAsync(h_flags, flags, 8, hipMemcpyDeviceToHost, c->stream));
  MFA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  if (h_flags[0]) return c->fail("%s: a psi entry that is not positive and finite", who);
  if (h_flags[1]) return c->fail("%s: offsets that are not 0 = off[0] < ... < off[%d] = %lld", who, C, (long long)N);
  if (mfa_pair_pack(c, op, y, N, D)) return -1;
  return mfa_pair_silhouette_sweep(c, op, y, q, pair_weight(metric), metric, d_off, C, own, N, D, d_sil, d_a, d_b, d_bj, d_v);
}
