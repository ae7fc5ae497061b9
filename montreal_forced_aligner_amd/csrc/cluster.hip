// The clustering stage on gfx950: what the reference's cluster_matrix (MFA/diarization/multiprocessing.py) does with the
// vectors of a corpus for ClusterType.dbscan, on the neighbour bit matrix that the sweep of plda.hip writes (its fourth
// consumer).  scikit-learn's DBSCAN restated as integer work with a unique answer: DESIGN.md "Clustering".
// Arithmetic contract: include/mfa_hip.h "Clustering"; the shared rules: cluster_math.hpp; the host twin: cluster_host.cpp.
//
//   symmetrise  cluster_symmetrise_kernel, a wavefront per pair of 64 × 64 blocks (I, J), (J, I), I <= J: a lane holds a
//               row's word of either block; word r of a block's transpose is the ballot of bit r over the lanes.  Each
//               block is read and written by its one wavefront: in place.  The diagonal is set, padding bits are cleared
//   degree      cluster_degree_kernel, a wavefront per row: the popcount; cluster_core_kernel: the core mask as words and
//               the first roots (a core point's own index)
//   components  rounds of cluster_propagate_kernel (a wavefront per core row: the minimum root over its core neighbours)
//               and cluster_jump_kernel (a thread per core point follows root[root[..]]), until a round changes nothing
//   labels      the roots' flags, their exclusive scan (vad.hip's reduce-then-scan) = a cluster's number, and
//               cluster_label_kernel, a wavefront per row: a core point its cluster's number, any other point the smallest
//               number among its core neighbours
// No atomics.  The rounds work in place on root[], and a wavefront may read a root that another is just lowering.  That is
// harmless, because the answer does not depend on the schedule: every value stored into root[x] is below one that root[x] held
// earlier in the same round (so a root ends a round at or below where it began, and root[x] <= x always), and it is the index
// of a core point of the same component, so every schedule stays at or above the component's smallest index; and a state that
// no round changes has root[i] <= root[j] over every edge in both directions, hence one value per component, which the
// smallest member (its own root from the start) pins to its index.  That state is unique.  Only the number of rounds is the
// schedule's.
#include <algorithm>

#include "acc_segments.hpp"
#include "cluster_math.hpp"
#include "ctx.hpp"

namespace {

constexpr int kJumpHops = 16;              // links a thread of the jump kernel follows at the most
constexpr int64_t kGridY = 65535;

// grid (W, blocks of 4 J from j4_0).
__global__ __launch_bounds__(256) void cluster_symmetrise_kernel(uint64_t *bits, int64_t N, int64_t W, int64_t j4_0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t I = blockIdx.x, J = (j4_0 + blockIdx.y) * 4 + wave;
  if (J >= W || I > J) return;                       // the same for the whole wavefront
  const int64_t ri = I * 64 + lane, rj = J * 64 + lane;
  const bool diag = I == J;
  const uint64_t a = ri < N ? bits[(size_t)ri * W + J] : 0;                    // block (I, J): row ri's columns of J
  const uint64_t b = diag ? a : (rj < N ? bits[(size_t)rj * W + I] : 0);       // block (J, I): row rj's columns of I
  uint64_t ta = 0, tb = 0;                           // their transposes: lane r takes the ballot of bit r
#pragma unroll 8
  for (int r = 0; r < 64; r++) {
    const uint64_t ma = __ballot((a >> r) & 1), mb = __ballot((b >> r) & 1);
    ta = lane == r ? ma : ta;
    tb = lane == r ? mb : tb;
  }
  if (ri < N) bits[(size_t)ri * W + J] = (a | tb | (diag ? (uint64_t)1 << lane : 0)) & cluster_pad_mask(N, J);
  if (!diag && rj < N) bits[(size_t)rj * W + I] = (b | ta) & cluster_pad_mask(N, I);
}

// grid: 4 rows a workgroup, a wavefront each.
__global__ __launch_bounds__(256) void cluster_degree_kernel(const uint64_t *bits, int64_t N, int64_t W, int32_t min_samples, int32_t *count,
                                                             int32_t *core) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= N) return;
  const uint64_t *br = bits + (size_t)row * W;
  int32_t n = 0;
  for (int64_t w = lane; w < W; w += 64) n += __popcll(br[w]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if (lane == 0) { count[row] = n; core[row] = cluster_is_core(n, min_samples) ? 1 : 0; }
}

// grid: 4 words a workgroup, a wavefront each: lane l is point 64 w + l.
__global__ __launch_bounds__(256) void cluster_core_kernel(const int32_t *core, int64_t N, int64_t W, uint64_t *coremask, int32_t *root) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= W) return;
  const int64_t i = w * 64 + lane;
  const bool c = i < N && core[i] != 0;
  const uint64_t m = __ballot(c);
  if (lane == 0) coremask[w] = m;
  if (i < N) root[i] = c ? (int32_t)i : kClusterNoRoot;
}

// The smallest root among row's core neighbours (the point itself is one when it is a core point); the whole wavefront
// gets it.  The bits name columns below N only (symmetrise cleared the padding), so every root[] index is in range.
__device__ __forceinline__ int32_t min_core_root(const uint64_t *br, const uint64_t *coremask, int64_t W, const int32_t *root, int lane) {
  int32_t m = kClusterNoRoot;
  for (int64_t w = lane; w < W; w += 64) {
    uint64_t x = br[w] & coremask[w];
    while (x) {
      const int bit = __ffsll((long long)x) - 1;
      x &= x - 1;
      m = min(m, root[w * 64 + bit]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
  return m;
}

// grid: 4 rows a workgroup, a wavefront each.  changed: the "something changed" word, a plain store of 1.
__global__ __launch_bounds__(256) void cluster_propagate_kernel(const uint64_t *bits, const uint64_t *coremask, const int32_t *core, int64_t N,
                                                                int64_t W, int32_t *root, int32_t *changed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= N || core[row] == 0) return;            // the same for the whole wavefront
  const int32_t m = min_core_root(bits + (size_t)row * W, coremask, W, root, lane);
  if (lane != 0) return;
  const int32_t mine = root[row];
  if (m >= mine) return;
  root[row] = m;
  *changed = 1;
  // The point's old root hears of the lower root too, so that a tree learns from its border at once and not one link a
  // round.  Several wavefronts may store here, and the last one wins, not the smallest: every value stored is below one
  // that root[mine] held earlier in the round (so it ends the round below where it began, and still at or below mine), and it
  // is a core index of the same component.  Which of them stays changes the number of rounds, never the state they end in.
  if (m < root[mine]) root[mine] = m;
}

// A thread per point: a core point's root becomes its root's root, up to kJumpHops links on.  A root is a core point's
// index at or below the point's own, so the walk goes down and stays in range.
__global__ __launch_bounds__(256) void cluster_jump_kernel(const int32_t *core, int64_t N, int32_t *root, int32_t *changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N || core[i] == 0) return;
  const int32_t r0 = root[i];
  int32_t r = r0;
  for (int h = 0; h < kJumpHops; h++) {
    const int32_t p = root[r];
    if (p >= r) break;
    r = p;
  }
  if (r < r0) { root[i] = r; *changed = 1; }
}

__global__ __launch_bounds__(256) void cluster_rootflag_kernel(const int32_t *core, const int32_t *root, int64_t N, int32_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) flag[i] = core[i] != 0 && root[i] == (int32_t)i ? 1 : 0;
}

// grid: 4 rows a workgroup, a wavefront each.  G: the exclusive scan of the root flags = the number of a root's cluster.
// Cluster numbers ascend with the roots, so the smallest number among a point's core neighbours is that of the smallest root.
__global__ __launch_bounds__(256) void cluster_label_kernel(const uint64_t *bits, const uint64_t *coremask, const int32_t *core,
                                                            const int32_t *root, const int32_t *G, int64_t N, int64_t W, int32_t *labels) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= N) return;
  const int32_t r = core[row] != 0 ? root[row] : min_core_root(bits + (size_t)row * W, coremask, W, root, lane);
  if (lane == 0) labels[row] = r == kClusterNoRoot ? kClusterNoise : G[r];
}

unsigned blocks(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

extern "C" MFA_API int mfa_dbscan_from_bits(mfa_ctx *c, uint64_t *d_bits, int64_t N, int32_t min_samples, int32_t *d_labels, int32_t *d_core,
                                            int32_t *d_count, int32_t *h_n_clusters, int32_t *h_rounds) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "DBSCAN";
  const int rc = cluster_check(N, min_samples);
  if (rc == -2) return c->fail("%s: %lld points (0 to 2^31 - 1)", who, (long long)N);
  if (rc == -3) return c->fail("%s: min_samples %d (1 or more)", who, min_samples);
  if (!h_n_clusters || !h_rounds) return c->fail("%s: NULL result", who);
  *h_n_clusters = 0;
  *h_rounds = 0;
  if (N == 0) return 0;
  if (!d_bits || !d_labels || !d_core || !d_count) return c->fail("%s: NULL array", who);
  const int64_t W = cluster_words(N);
  Workspace ws;
  const size_t P = mfa_int_scan_blocks(N);
  const size_t o_mask = ws.take((size_t)W * 8), o_root = ws.take((size_t)N * 4), o_flag = ws.take((size_t)N * 4),
               o_G = ws.take(((size_t)N + 1) * 4), o_bsum = ws.take(P * 4), o_base = ws.take((P + 1) * 4), o_changed = ws.take(4);
  if (ws.reserve(c, "the clustering workspace")) return -1;
  uint64_t *mask = ws.at<uint64_t>(o_mask);
  int32_t *root = ws.at<int32_t>(o_root), *flag = ws.at<int32_t>(o_flag), *G = ws.at<int32_t>(o_G), *changed = ws.at<int32_t>(o_changed);
  {
    KernelTimer kt(c, MFA_K_CLUSTER_SYMM);
    const int64_t j4 = (W + 3) / 4;
    for (int64_t y0 = 0; y0 < j4; y0 += kGridY)
      hipLaunchKernelGGL(cluster_symmetrise_kernel, dim3((unsigned)W, (unsigned)std::min<int64_t>(kGridY, j4 - y0)), dim3(256), 0, c->stream,
                         d_bits, N, W, y0);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "cluster_symmetrise_kernel N=%lld", (long long)N);
  }
  {
    KernelTimer kt(c, MFA_K_CLUSTER_DEGREE);
    hipLaunchKernelGGL(cluster_degree_kernel, dim3(blocks(N, 4)), dim3(256), 0, c->stream, d_bits, N, W, min_samples, d_count, d_core);
    hipLaunchKernelGGL(cluster_core_kernel, dim3(blocks(W, 4)), dim3(256), 0, c->stream, d_core, N, W, mask, root);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "cluster_degree_kernel N=%lld min_samples=%d", (long long)N, min_samples);
  }
  int32_t rounds = 0;
  for (;;) {
    int32_t h_changed = 0;
    {
      KernelTimer kt(c, MFA_K_CLUSTER_ROUNDS);
      MFA_HIP_CHECK(c, hipMemsetAsync(changed, 0, 4, c->stream));
      hipLaunchKernelGGL(cluster_propagate_kernel, dim3(blocks(N, 4)), dim3(256), 0, c->stream, d_bits, mask, d_core, N, W, root, changed);
      hipLaunchKernelGGL(cluster_jump_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, d_core, N, root, changed);
      MFA_HIP_CHECK(c, hipGetLastError());
      MFA_DEBUG_POINT(c, "cluster round %d", rounds);
    }
    MFA_HIP_CHECK(c, hipMemcpyAsync(&h_changed, changed, 4, hipMemcpyDeviceToHost, c->stream));
    MFA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    rounds++;
    if (!h_changed) break;
    // a round that changes something lowers the sum of the roots, which starts below N^2 / 2: the search ends; this is the net under it
    if (rounds == INT32_MAX || (int64_t)rounds > N * (N + 1) / 2 + 1) return c->fail("%s: the components did not settle in %d rounds", who, rounds);
  }
  int32_t n_clusters = 0;
  {
    KernelTimer kt(c, MFA_K_CLUSTER_LABELS);
    hipLaunchKernelGGL(cluster_rootflag_kernel, dim3(blocks(N, 256)), dim3(256), 0, c->stream, d_core, root, N, flag);
    mfa_int_scan(c, flag, N, ws.at<int32_t>(o_bsum), ws.at<int32_t>(o_base), G);
    hipLaunchKernelGGL(cluster_label_kernel, dim3(blocks(N, 4)), dim3(256), 0, c->stream, d_bits, mask, d_core, root, G, N, W, d_labels);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "cluster_label_kernel N=%lld", (long long)N);
  }
  MFA_HIP_CHECK(c, hipMemcpyAsync(&n_clusters, G + N, 4, hipMemcpyDeviceToHost, c->stream));
  MFA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  *h_n_clusters = n_clusters;
  *h_rounds = rounds;
  return 0;
}
