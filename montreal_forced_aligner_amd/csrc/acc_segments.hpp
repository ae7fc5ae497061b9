// What the training-statistics translation units (gmm_acc.hip, mllt_acc.hip, lda_acc.hip, tree_acc.hip) share around their
// sum kernels: frames are ordered by key (pdf, class, event) with a stable sort, a key's segment is cut into units of a fixed
// number of entries, a workgroup (wavefront) sums a unit from zero in frame order, and the units' partials are added in unit
// order onto the caller's value.  Every sum is thus a function of the input alone; no floating-point atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ctx.hpp"

// Largest i in [0, n) with base[i] <= v (base ascending, base[0] <= v): with base the exclusive scan of the keys' unit counts,
// the key that owns unit v; with base an utterance's first frames, the utterance of frame v.
template <typename T>
__device__ __forceinline__ int acc_owner(const T *base, int n, T v) {
  int lo = 0, hi = n;                 // base[lo] <= v < base[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// One workgroup of 256 threads: exclusive scans over P keys of N quantities.  The functor gives a key's contributions,
// f.add(q, v): v[k] += quantity k of key q, and takes the scans, f.put(q, v) for q in [0, P]: v[k] = the sum of quantity k
// over the keys before q (q = P: the totals).
template <int N, typename F>
static __global__ __launch_bounds__(256) void acc_scan_kernel(F f, int P) {
  __shared__ int64_t s[256][N], total[N];
  const int per = (P + 255) / 256, a = min(P, (int)threadIdx.x * per), b = min(P, a + per);
  int64_t v[N];
  for (int k = 0; k < N; k++) v[k] = 0;
  for (int q = a; q < b; q++) f.add(q, v);
  for (int k = 0; k < N; k++) s[threadIdx.x][k] = v[k];
  __syncthreads();
  if (threadIdx.x < N) {              // thread k scans quantity k over the 256 threads' sums
    const int k = threadIdx.x;
    int64_t acc = 0;
    for (int i = 0; i < 256; i++) { const int64_t t = s[i][k]; s[i][k] = acc; acc += t; }
    total[k] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < N; k++) v[k] = total[k];
    f.put(P, v);
  }
  for (int k = 0; k < N; k++) v[k] = s[threadIdx.x][k];
  for (int q = a; q < b; q++) { f.put(q, v); f.add(q, v); }
}

// a, then base[0], base[stride], .. base[(n − 1)·stride] added one after the other in that order.  The loads of 8 partials
// are issued together (a pdf that holds a seventh of the corpus has thousands of chunks and one thread per element to walk
// them); the additions stay in order.
__device__ __forceinline__ double acc_ordered_sum(const double *base, size_t stride, int n, double a) {
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = base[(size_t)(i + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; k++) a += v[k];
  }
  for (; i < n; i++) a += base[(size_t)i * stride];
  return a;
}

// An alignment is runs of one transition-id (self-loops), and silence holds a good share of a corpus: one atomic per run of
// equal ids inside the wavefront, not one per frame, keeps the hot counters from serialising a lookup's launch.  The whole
// wavefront calls this with its lane's frame (take: the frame counts; id: its transition-id); the first lane of every run of
// frames that count and share an id calls counts(run length).
template <typename F>
__device__ __forceinline__ void acc_wave_runs(bool take, int id, F counts) {
  const int lane = threadIdx.x & 63;
  const int key = take ? id : -1;
  const int prev = __shfl_up(key, 1);
  const bool ends = lane == 0 || prev != key;                 // a run of any kind starts here
  const bool head = take && ends;
  const unsigned long long starts = __ballot(ends);
  if (head) {
    const unsigned long long above = lane == 63 ? 0ull : starts >> (lane + 1);
    counts(above ? __ffsll((long long)above) : 64 - lane);
  }
}

// Bits of a sort key that takes the values 0 .. n_keys (n_keys itself: a frame that takes no part).
inline unsigned acc_end_bit(uint64_t n_keys) { unsigned b = 1; while (((uint64_t)1 << b) <= n_keys) b++; return b; }

// The context's workspace carved into arrays that start 256 bytes apart at the least: take() every array, reserve(), then at().
struct Workspace {
  size_t bytes = 0;
  char *base = nullptr;
  size_t take(size_t n) { const size_t off = bytes; bytes = (bytes + n + 255) & ~(size_t)255; return off; }
  int reserve(mfa_ctx *c, const char *what) {
    if (c->d_ws.reserve(c, bytes, what)) return -1;
    base = c->d_ws.ptr<char>();
    return 0;
  }
  template <typename T> T *at(size_t off) const { return (T *)(base + off); }
};

// The loaded model as the posterior kernels (acc_posterior.hpp) see it: Gaussians of the largest pdf and in all; on the
// device [num_pdfs] Gaussians per pdf and [num_pdfs + 1] first model Gaussian.
struct AccModel {
  int max_ng = 0;
  int64_t G = 0;
  const int32_t *d_ngauss = nullptr, *d_goff = nullptr;
};

// The checks that the statistics over a loaded model begin with, in their order, and the context's table of the pdfs'
// Gaussian counts (d_acc_tabs), built by whichever call comes first.  who: the message prefix ("GMM statistics"); dim_why: why
// the feature dim is limited to max_dim; chunk: entries per unit.
// Returns 0: go on; 1: no frames, nothing to do; -1: failed (the message is set).
inline int acc_model_tabs(mfa_ctx *c, const char *who, int max_dim, const char *dim_why, int max_gauss, int chunk,
                          int64_t total_frames, int32_t n_tids, AccModel &m) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  const int D = c->dim, P = c->num_pdfs;
  if (D > max_dim) return c->fail("%s: feature dim %d > %d (%s)", who, D, max_dim, dim_why);
  for (int p = 0; p < P; p++) {
    if (c->h_ngauss[p] > max_gauss) return c->fail("%s: pdf %d has more than %d Gaussians", who, p, max_gauss);
    m.max_ng = std::max(m.max_ng, (int)c->h_ngauss[p]);
    m.G += c->h_ngauss[p];
  }
  if (total_frames <= 0) return 1;
  if (total_frames >= ((int64_t)1 << 31) - chunk) return c->fail("%s: %lld frames in one call (at most 2^31 - %d)", who, (long long)total_frames, chunk + 1);
  if (n_tids <= 0) return c->fail("%s: empty transition-id table", who);
  if (!c->d_acc_tabs) {
    std::vector<int32_t> tabs((size_t)2 * P + 1);
    int32_t off = 0;
    for (int p = 0; p < P; p++) { tabs[p] = c->h_ngauss[p]; tabs[P + p] = off; off += c->h_ngauss[p]; }
    tabs[2 * P] = off;
    if (dev_upload_commit<MfaHipDev>(c, "the pdfs' Gaussian counts", {{&c->d_acc_tabs, tabs.data(), tabs.size() * 4}})) return -1;
  }
  m.d_ngauss = c->d_acc_tabs.ptr<int32_t>();
  m.d_goff = m.d_ngauss + P;
  return 0;
}
