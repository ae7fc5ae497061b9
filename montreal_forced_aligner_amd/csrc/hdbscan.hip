// The HDBSCAN stage on gfx950: what the reference's cluster_matrix (MFA/diarization/multiprocessing.py) asks of the hdbscan
// package for ClusterType.hdbscan that costs O(N²·D): every point's core distance and the minimum spanning tree of the
// mutual-reachability graph, with no N × N array stored.  Restated from the papers (Campello, Moulavi, Sander 2013; McInnes,
// Healy 2017); the cluster tree on the N − 1 edges is host work (hdbscan.py).  Arithmetic contract: include/mfa_hip.h
// "HDBSCAN"; the shared rules: hdbscan_math.hpp; the sweep and its two pair consumers: plda.hip (pair_sweep.hpp); the host
// twins: hdbscan_host.cpp.
//
//   prepare    pair_prepare_kernel, a thread per point: the row y and the scalar q of the pair form
//   core       the sweep's core consumer: the k-nearest list on v, the k-th entry is the core score
//   rounds     Borůvka: the sweep's edge consumer gives every row its best edge out of its component; hdb_row_score_kernel
//              and hdb_row_pair_kernel reduce the rows' bests to one per component with 64-bit integer atomics on keys that
//              preserve edge_better (atomicMax on the score's key, then atomicMin on (lo << 32) | hi among the rows that hold
//              that score); hdb_choose_kernel, a thread per root: the root it joins and whether it emits the edge (of two
//              components that chose the same edge the smaller root emits and stays); the exclusive scan of the emit flags
//              (vad.hip's) gives the edges' places; hdb_emit_kernel writes them, the roots' links and the round's record;
//              hdb_jump_kernel follows the links, out of place, 16 at a launch
// Integer max and min commute and are associative, so what the atomics leave does not depend on the order the device ran
// the threads in; no floating-point atomic, no loop that waits on another wavefront, and every loop has a bound known at
// its start.  Under the strict total order of edge_better the tree is unique: the same bits every run, whatever the passes.
#include <algorithm>

#include "hdbscan_math.hpp"
#include "pair_sweep.hpp"

namespace {

constexpr int kJumpHops = 16;              // links a thread of the jump kernel follows in one launch

// flags[0] |= a psi that is not positive and finite (a plain store of the same value).
__global__ __launch_bounds__(256) void pair_prepare_kernel(const double *x, int32_t metric, const double *psi, int64_t N, int D, double *y,
                                                           double *q, int32_t *flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double s_quad = 0.0, s_logr = 0.0;
  for (int k = 0; k < D; k++) {
    const double ps = metric == kMetricPlda ? psi[k] : 1.0;
    if (!plda_psi_ok(ps)) flags[0] = 1;
    const PairTerm t = pair_term(metric, x[(size_t)i * D + k], ps);
    y[(size_t)i * D + k] = t.y;
    s_quad += t.quad;
    s_logr += t.logr;
  }
  q[i] = pair_q(metric, s_quad, s_logr);
}

__global__ __launch_bounds__(256) void hdb_init_kernel(int64_t N, int32_t *comp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) comp[i] = (int32_t)i;
}

// A thread per row with an edge: its component's best score.  key_m is zeroed before (0: no edge).
__global__ __launch_bounds__(256) void hdb_row_score_kernel(const double *row_m, const int32_t *row_j, const int32_t *comp, int64_t N,
                                                            unsigned long long *key_m) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N || row_j[i] < 0) return;
  atomicMax(&key_m[comp[i]], (unsigned long long)score_key(row_m[i]));
}

// ... and among the rows that hold that score, the smallest pair.  key_e is set to all ones before.
__global__ __launch_bounds__(256) void hdb_row_pair_kernel(const double *row_m, const int32_t *row_j, const int32_t *comp, int64_t N,
                                                           const unsigned long long *key_m, unsigned long long *key_e) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N || row_j[i] < 0) return;
  const int32_t r = comp[i];
  if ((unsigned long long)score_key(row_m[i]) != key_m[r]) return;
  atomicMin(&key_e[r], (unsigned long long)pair_key((int32_t)i, row_j[i]));
}

// A thread per point; only a root with an edge acts.  The edge's far end is the one outside the root's component; fr is its
// root.  When fr chose the same edge (two components whose best edges point at each other chose the same edge: each is an
// edge out of the other, so neither is better), the smaller root emits it and stays a root.  next: the root's link; flag:
// it emits.  Reads comp only.
__global__ __launch_bounds__(256) void hdb_choose_kernel(const int32_t *comp, int64_t N, const unsigned long long *key_m,
                                                         const unsigned long long *key_e, int32_t *next, int32_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int32_t nx = comp[i], fl = 0;
  if (nx == (int32_t)i && key_m[i] != 0) {
    const unsigned long long e = key_e[i];
    const int32_t lo = (int32_t)(e >> 32), hi = (int32_t)(e & 0xffffffffull);
    const int32_t fr = comp[lo] == (int32_t)i ? comp[hi] : comp[lo];
    const bool same = key_m[fr] != 0 && key_e[fr] == e;
    fl = same && fr < (int32_t)i ? 0 : 1;
    nx = same && (int32_t)i < fr ? (int32_t)i : fr;
  }
  next[i] = nx;
  flag[i] = fl;
}

// A thread per point: an emitting root writes its edge at base + G[i]; every point takes its link (a point that is no root
// keeps its root).  Thread 0 writes the round's record: edges so far, components left, something changed.
__global__ __launch_bounds__(256) void hdb_emit_kernel(const int32_t *next, const int32_t *flag, const int32_t *G, int64_t N, int32_t base,
                                                       const unsigned long long *key_m, const unsigned long long *key_e, int32_t *edge_lo,
                                                       int32_t *edge_hi, double *edge_score, int32_t *comp, int32_t *record) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (flag[i]) {
    const int64_t at = (int64_t)base + G[i];
    if (at < N - 1) {                                 // a forest on N points has at most N − 1 edges: never false
      const unsigned long long e = key_e[i];
      edge_lo[at] = (int32_t)(e >> 32);
      edge_hi[at] = (int32_t)(e & 0xffffffffull);
      edge_score[at] = key_score(key_m[i]);
    }
  }
  comp[i] = next[i];
  if (i == 0) {
    const int32_t added = G[N];
    record[0] = base + added;
    record[1] = (int32_t)(N - (int64_t)base - added);
    record[2] = added > 0 ? 1 : 0;
  }
}

// A thread per point: dst[i] is up to kJumpHops links on from src[i] (a root links to itself).  Out of place: src does not
// change during the launch, so the result is a function of src alone; a chain of L links becomes one of ceil(L / 16).
__global__ __launch_bounds__(256) void hdb_jump_kernel(const int32_t *src, int64_t N, int32_t *dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int32_t r = src[i];
  for (int h = 0; h < kJumpHops; h++) {
    const int32_t p = src[r];
    if (p == r) break;
    r = p;
  }
  dst[i] = r;
}

unsigned blocks(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

int refuse(mfa_ctx *c, const char *who, int rc, int D, int k, long long n) {
  switch (rc) {
    case -2: return c->fail("%s: dimension %d (1 to %d)", who, D, kPldaMaxDim);
    case -3: return c->fail("%s: %d neighbours (0 to %d: a row's list is one wavefront register)", who, k, kPldaMaxK);
    case -5: return c->fail("%s: %lld points in one call (fewer than 2^31)", who, n);
    default: return c->fail("%s: a negative count", who);
  }
}

}  // namespace

int mfa_pair_prepare(mfa_ctx *c, const double *d_x, int32_t metric, const double *d_psi, int64_t N, int D, double *d_y, double *d_q,
                     int32_t *d_flags) {
  KernelTimer kt(c, MFA_K_PLDA_PREPARE);
  MFA_HIP_CHECK(c, hipMemsetAsync(d_flags, 0, 8, c->stream));
  hipLaunchKernelGGL(pair_prepare_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, d_x, metric, d_psi, N, D, d_y, d_q, d_flags);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "pair_prepare_kernel N=%lld D=%d metric=%d", (long long)N, D, metric);
  return 0;
}

extern "C" MFA_API int mfa_hdbscan_core_batch(mfa_ctx *c, const double *d_x, int64_t N, int32_t D, int32_t metric, const double *d_psi, int32_t k,
                                              double *d_y, double *d_q, double *d_core, double *d_v) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "HDBSCAN core scores";
  if (!plda_metric_ok(metric)) return c->fail("%s: metric %d (0 plda, 1 euclidean, 2 dot)", who, metric);
  const int rc = hdbscan_check_shape(D, k, N);
  if (rc) return refuse(c, who, rc, D, k, (long long)N);
  if (N == 0) return 0;
  if (!d_x || !d_y || !d_q || !d_core || (metric == kMetricPlda && !d_psi)) return c->fail("%s: NULL array", who);
  MfaPairSweep op;
  if (mfa_pair_lay_out(c, op, N, D, k)) return -1;
  const size_t o_flags = op.ws.take(8);
  if (op.ws.reserve(c, "the HDBSCAN workspace")) return -1;
  int32_t *flags = op.ws.at<int32_t>(o_flags);
  if (mfa_pair_prepare(c, d_x, metric, d_psi, N, D, d_y, d_q, flags)) return -1;
  int32_t h_flags[2] = {0, 0};
  MFA_HIP_CHECK(c, hipMemcpyAsync(h_flags, flags, 8, hipMemcpyDeviceToHost, c->stream));
  MFA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  if (h_flags[0]) return c->fail("%s: a psi entry that is not positive and finite", who);
  if (k > 0 || d_v) {
    if (mfa_pair_pack(c, op, d_y, N, D)) return -1;
  }
  return mfa_pair_core_sweep(c, op, d_y, d_q, pair_weight(metric), N, D, k, d_core, d_v);
}

extern "C" MFA_API int mfa_hdbscan_mst_batch(mfa_ctx *c, const double *d_y, const double *d_q, const double *d_core, int64_t N, int32_t D,
                                             int32_t metric, int32_t *d_edge_lo, int32_t *d_edge_hi, double *d_edge_score,
                                             int32_t *h_n_edges, int32_t *h_rounds) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "HDBSCAN spanning tree";
  if (!plda_metric_ok(metric)) return c->fail("%s: metric %d (0 plda, 1 euclidean, 2 dot)", who, metric);
  const int rc = hdbscan_check_shape(D, 0, N);
  if (rc) return refuse(c, who, rc, D, 0, (long long)N);
  if (!h_n_edges || !h_rounds) return c->fail("%s: NULL result", who);
  *h_n_edges = 0;
  *h_rounds = 0;
  if (N <= 1) return 0;
  if (!d_y || !d_q || !d_core || !d_edge_lo || !d_edge_hi || !d_edge_score) return c->fail("%s: NULL array", who);
  MfaPairSweep op;
  if (mfa_pair_lay_out(c, op, N, D, 0)) return -1;
  Workspace &ws = op.ws;
  const size_t P = mfa_int_scan_blocks(N);
  const size_t o_comp = ws.take((size_t)N * 4), o_comp2 = ws.take((size_t)N * 4), o_next = ws.take((size_t)N * 4), o_flag = ws.take((size_t)N * 4),
               o_G = ws.take(((size_t)N + 1) * 4), o_bsum = ws.take(P * 4), o_base = ws.take((P + 1) * 4), o_rm = ws.take((size_t)N * 8),
               o_rj = ws.take((size_t)N * 4), o_km = ws.take((size_t)N * 8), o_ke = ws.take((size_t)N * 8), o_rec = ws.take(16);
  if (ws.reserve(c, "the HDBSCAN workspace")) return -1;
  int32_t *comp = ws.at<int32_t>(o_comp), *comp2 = ws.at<int32_t>(o_comp2), *next = ws.at<int32_t>(o_next), *flag = ws.at<int32_t>(o_flag),
          *G = ws.at<int32_t>(o_G), *row_j = ws.at<int32_t>(o_rj), *record = ws.at<int32_t>(o_rec);
  double *row_m = ws.at<double>(o_rm);
  unsigned long long *key_m = ws.at<unsigned long long>(o_km), *key_e = ws.at<unsigned long long>(o_ke);
  if (mfa_pair_pack(c, op, d_y, N, D)) return -1;
  hipLaunchKernelGGL(hdb_init_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, N, comp);
  MFA_HIP_CHECK(c, hipGetLastError());
  int jumps = 0;                                       // launches that bring any chain of up to N + 1 links down to one
  for (int64_t reach = 1; reach < N + 1; reach *= kJumpHops) jumps++;
  const double w = pair_weight(metric);
  int32_t edges = 0, rounds = 0;
  while (N - edges > 1) {
    if (rounds == kHdbscanMaxRounds) return c->fail("%s: %lld components left after %d rounds", who, (long long)(N - edges), rounds);
    if (mfa_pair_edge_sweep(c, op, d_y, d_q, w, d_core, comp, N, D, row_m, row_j)) return -1;
    int32_t h_rec[3] = {0, 0, 0};
    {
      KernelTimer kt(c, MFA_K_CLUSTER_ROUNDS);
      MFA_HIP_CHECK(c, hipMemsetAsync(key_m, 0, (size_t)N * 8, c->stream));
      MFA_HIP_CHECK(c, hipMemsetAsync(key_e, 0xff, (size_t)N * 8, c->stream));
      hipLaunchKernelGGL(hdb_row_score_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, row_m, row_j, comp, N, key_m);
      hipLaunchKernelGGL(hdb_row_pair_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, row_m, row_j, comp, N, key_m, key_e);
      hipLaunchKernelGGL(hdb_choose_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, comp, N, key_m, key_e, next, flag);
      mfa_int_scan(c, flag, N, ws.at<int32_t>(o_bsum), ws.at<int32_t>(o_base), G);
      hipLaunchKernelGGL(hdb_emit_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, next, flag, G, N, edges, key_m, key_e, d_edge_lo,
                         d_edge_hi, d_edge_score, comp, record);
      for (int j = 0; j < jumps; j++) {
        hipLaunchKernelGGL(hdb_jump_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, comp, N, comp2);
        std::swap(comp, comp2);
      }
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "hdbscan round %d", rounds);
    }
    MFA_HIP_CHECK(c, hipMemcpyAsync(h_rec, record, 12, hipMemcpyDeviceToHost, c->stream));
    MFA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    rounds++;
    if (h_rec[0] < edges || h_rec[0] > N - 1) return c->fail("%s: a round's record of %d edges after %d", who, h_rec[0], edges);
    edges = h_rec[0];
    if (!h_rec[2]) break;                              // no edge between the components that are left
  }
  *h_n_edges = edges;
  *h_rounds = rounds;
  return 0;
}
