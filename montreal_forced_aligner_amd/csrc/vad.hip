// Speech activity for gfx950: Kaldi's energy VAD, sliding-window CMVN, voiced-frame selection with subsampling, and the
// runs of voiced frames — the contract of include/mfa_hip.h ("Speech activity"); the arithmetic is vad_math.hpp's, which the
// host twins (vad_host.cpp) run too.  Every kernel is parallel over the frames inside an utterance: a batch is four
// recordings of 360 000 frames as readily as 8 192 utterances of 1 000.
//
//   the scan     one exclusive scan of an int32 per frame over the WHOLE batch, G [total + 1], reduce-then-scan: block sums
//                (scan_sums_kernel), their exclusive scan by one workgroup (acc_scan_kernel of acc_segments.hpp), the scan
//                inside every block on top of its base (scan_apply_kernel).  Three launches in stream order, no workgroup
//                ever waits for another.  Integers: the per-utterance scan is G[f] − G[first frame of the utterance],
//                exact, and so the same whatever else the batch holds.  G also is the run offsets and the kept-row ranks.
//   VAD          chunk sums of column 0 in the documented order (one workgroup per (utterance, chunk)), one thread per
//                utterance adds them in order and fixes the threshold, a frame-parallel pass writes the e > thr flags,
//                the scan, and a frame-parallel pass takes both window counts from G.  The voiced count is integer
//                atomics, one per run of voiced frames of a wavefront (acc_wave_runs).
//   sliding CMVN a lane owns (tile of kCmnTile frames, column): lanes run over the columns of a row first, then the tiles, so
//                a wavefront's loads are runs of whole rows; (window + 2·tile) / tile cached loads per output.
//   selection    keep flags → G → per-utterance counts scanned by one workgroup → every kept row writes its source index
//                into the row map; the gather itself is a second entry point (the caller sizes its output in between).
//   runs         run-start flags → G → a run's first frame writes begin[G[f]], its last frame end[G[f + 1] − 1].
// The owner of a frame is found by bisection of d_frame_off (acc_owner).  Every store is a vector store of plain C++.
#include <cstdint>

#include "acc_segments.hpp"
#include "ctx.hpp"
#include "vad_math.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaveLanes = 64;
constexpr int kWaves = kThreads / kWaveLanes;
constexpr int kPerThread = kVadScanBlock / kThreads;   // consecutive values of a thread in the scan kernels
static_assert(kVadSumLanes == kThreads && kVadScanThreads == 256, "vad_math.hpp's lane counts are this file's workgroup");

inline unsigned blocks_for(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

// ---------------------------------------------------------------- the scan
__global__ __launch_bounds__(kThreads) void scan_sums_kernel(const int32_t *v, int64_t total, int32_t *bsum) {
  __shared__ int32_t wsum[kWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kVadScanBlock + (int64_t)threadIdx.x * kPerThread;
  int32_t s = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; k++) s += i0 + k < total ? v[i0 + k] : 0;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t t = 0;
    for (int w = 0; w < kWaves; w++) t += wsum[w];
    bsum[blockIdx.x] = t;
  }
}

struct BlockBases {            // acc_scan_kernel<1>: base[q] = Σ bsum[< q], q in [0, P]
  const int32_t *bsum; int32_t *base;
  __device__ void add(int q, int64_t *v) const { v[0] += bsum[q]; }
  __device__ void put(int q, const int64_t *v) const { base[q] = (int32_t)v[0]; }
};

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(const int32_t *v, int64_t total, const int32_t *base, int32_t *G) {
  __shared__ int32_t wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kVadScanBlock + (int64_t)threadIdx.x * kPerThread;
  int32_t x[kPerThread], s = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; k++) { x[k] = i0 + k < total ? v[i0 + k] : 0; s += x[k]; }
  int32_t incl = s;
  for (int o = 1; o < kWaveLanes; o <<= 1) {
    const int32_t up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == kWaveLanes - 1) wsum[wave] = incl;
  __syncthreads();
  int32_t at = base[blockIdx.x] + incl - s;
  for (int w = 0; w < wave; w++) at += wsum[w];
#pragma unroll
  for (int k = 0; k < kPerThread; k++) {
    if (i0 + k < total) G[i0 + k] = at;
    at += x[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) G[total] = base[gridDim.x];
}

// G [total + 1] from v [total], total > 0; bsum [P], base [P + 1] with P = blocks of kVadScanBlock frames.
void global_scan(mfa_ctx *c, const int32_t *v, int64_t total, int32_t *bsum, int32_t *base, int32_t *G) {
  const unsigned P = blocks_for(total, kVadScanBlock);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(P), dim3(kThreads), 0, c->stream, v, total, bsum);
  hipLaunchKernelGGL((acc_scan_kernel<1, BlockBases>), dim3(1), dim3(256), 0, c->stream, BlockBases{bsum, base}, (int)P);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(P), dim3(kThreads), 0, c->stream, v, total, base, G);
}

struct ScanSpace {             // the scan's arrays in the context's workspace, after whatever the caller took first
  size_t flags, G, bsum, base;
  void take(Workspace &ws, int64_t total) {
    const size_t P = (size_t)((total + kVadScanBlock - 1) / kVadScanBlock);
    flags = ws.take((size_t)total * 4); G = ws.take(((size_t)total + 1) * 4);
    bsum = ws.take(P * 4); base = ws.take((P + 1) * 4);
  }
};

// d_frame_off[0] = 0 is the caller's word (the offsets are on the device); what the host can see is checked.
int check_batch(mfa_ctx *c, const char *who, int32_t n_utt, int64_t total, const void *d_frame_off) {
  if (n_utt < 0 || total < 0) return c->fail("%s: negative sizes", who);
  if (total >= ((int64_t)1 << 31) - kVadScanBlock) return c->fail("%s: %lld frames in one call (at most 2^31 - %d)", who, (long long)total, kVadScanBlock + 1);
  if (n_utt > 0 && !d_frame_off) return c->fail("%s: no frame offsets", who);
  if (n_utt == 0 && total > 0) return c->fail("%s: frames without utterances", who);
  return 0;
}

__global__ __launch_bounds__(kThreads) void segment_scan_kernel(const int32_t *G, const int64_t *frame_off, int n_utt, int64_t total, int32_t *scan) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  const int u = acc_owner(frame_off, n_utt, g);
  scan[g] = G[g] - G[frame_off[u]];
}

__global__ __launch_bounds__(kThreads) void segment_totals_kernel(const int32_t *G, const int64_t *frame_off, int n_utt, int32_t *totals) {
  const int u = blockIdx.x * kThreads + threadIdx.x;
  if (u < n_utt) totals[u] = G[frame_off[u + 1]] - G[frame_off[u]];
}

// ---------------------------------------------------------------- energy VAD
// Partial sums live at slot frame_off[u] / chunk + u + chunk index: ceil(T / chunk) slots per utterance never overlap.
__device__ inline int64_t sum_slot(int64_t f0, int u) { return f0 / kVadSumChunk + u; }

__global__ __launch_bounds__(kThreads) void vad_chunk_sums_kernel(const float *feats, int stride, const int64_t *frame_off, double *partial) {
  __shared__ double lanes[kVadSumLanes];
  const int u = blockIdx.x;
  const int64_t f0 = frame_off[u], T = frame_off[u + 1] - f0, c0 = (int64_t)blockIdx.y * kVadSumChunk;
  if (c0 >= T) return;                               // (the whole workgroup)
  const int n = (int)(T - c0 < kVadSumChunk ? T - c0 : kVadSumChunk);
  const float *e0 = feats + (f0 + c0) * stride;
  lanes[threadIdx.x] = mfa_vad_lane_sum([&](int i) { return e0[(int64_t)i * stride]; }, n, (int)threadIdx.x);
  __syncthreads();
  for (int half = kVadSumLanes / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) mfa_vad_fold(lanes, threadIdx.x, half);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[sum_slot(f0, u) + blockIdx.y] = lanes[0];
}

__global__ __launch_bounds__(kThreads) void vad_threshold_kernel(const int64_t *frame_off, int n_utt, const double *partial, mfa_vad_opts o,
                                                                 float *thr, int32_t *voiced) {
  const int u = blockIdx.x * kThreads + threadIdx.x;
  if (u >= n_utt) return;
  const int64_t f0 = frame_off[u], T = frame_off[u + 1] - f0;
  const int chunks = (int)((T + kVadSumChunk - 1) / kVadSumChunk);
  const double sum = chunks > 0 ? acc_ordered_sum(partial + sum_slot(f0, u), 1, chunks, 0.0) : 0.0;
  thr[u] = mfa_vad_threshold(sum, T, o.energy_threshold, o.energy_mean_scale);
  if (voiced) voiced[u] = 0;
}

__global__ __launch_bounds__(kThreads) void vad_flags_kernel(const float *feats, int stride, const int64_t *frame_off, int n_utt, int64_t total,
                                                             const float *thr, int32_t *flags) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  const int u = acc_owner(frame_off, n_utt, g);
  flags[g] = feats[g * stride] > thr[u] ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void vad_decide_kernel(const int32_t *G, const int64_t *frame_off, int n_utt, int64_t total, mfa_vad_opts o,
                                                              float *vad, int32_t *voiced) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = g < total;                       // (every lane stays for the wavefront's ballot)
  int u = -1;
  bool v = false;
  if (live) {
    u = acc_owner(frame_off, n_utt, g);
    const int64_t f0 = frame_off[u], T = frame_off[u + 1] - f0;
    int64_t lo, hi;
    mfa_vad_context(g - f0, T, o.frames_context, &lo, &hi);
    v = mfa_vad_decide(G[f0 + hi] - G[f0 + lo], (int32_t)(hi - lo), o.proportion_threshold);
    vad[g] = v ? 1.0f : 0.0f;
  }
  if (voiced) acc_wave_runs(v, u, [&](int len) { atomicAdd(&voiced[u], len); });
}

// ---------------------------------------------------------------- sliding-window CMVN
__global__ __launch_bounds__(kThreads) void sliding_cmvn_kernel(const float *feats, const int64_t *frame_off, int dim, int stride,
                                                                mfa_sliding_cmvn_opts o, float *out) {
  const int u = blockIdx.x;
  const int64_t f0 = frame_off[u], T = frame_off[u + 1] - f0;
  const int64_t j = (int64_t)blockIdx.y * kThreads + threadIdx.x;
  const int64_t tile = j / stride;
  const int col = (int)(j - tile * stride);
  const int64_t t0 = tile * kCmnTile;
  if (t0 >= T) return;
  const int64_t t1 = t0 + kCmnTile < T ? t0 + kCmnTile : T;
  const float *src = feats + f0 * stride + col;
  float *dst = out + f0 * stride + col;
  if (col < dim) {
    mfa_cmn_tile(t0, t1, T, o, [&](int64_t t) { return src[t * stride]; }, [&](int64_t t, float v) { dst[t * stride] = v; });
  } else {
    for (int64_t t = t0; t < t1; t++) dst[t * stride] = src[t * stride];
  }
}

// ---------------------------------------------------------------- selection
__global__ __launch_bounds__(kThreads) void keep_flags_kernel(const float *vad, int64_t total, int32_t *flags) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g < total) flags[g] = vad && vad[g] == 0.0f ? 0 : 1;
}

struct SelectOffsets {         // acc_scan_kernel<1> over the utterances: out_off[q] = Σ rows of the utterances before q
  const int32_t *G; const int64_t *frame_off; int32_t n; int64_t *out_off;
  __device__ void add(int q, int64_t *v) const { v[0] += mfa_select_count(G[frame_off[q + 1]] - G[frame_off[q]], n); }
  __device__ void put(int q, const int64_t *v) const { out_off[q] = v[0]; }
};

__global__ __launch_bounds__(kThreads) void select_map_kernel(const int32_t *flags, const int32_t *G, const int64_t *frame_off, int n_utt,
                                                              int64_t total, int32_t n, const int64_t *out_off, int32_t *src) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total || !flags[g]) return;
  const int u = acc_owner(frame_off, n_utt, g);
  const int32_t row = mfa_select_row(G[g] - G[frame_off[u]], n);
  if (row >= 0) src[out_off[u] + row] = (int32_t)g;
}

__global__ __launch_bounds__(kThreads) void gather_rows_kernel(const float *feats, int stride, int dim, const int32_t *src, int64_t n_out,
                                                               float *out, int out_stride) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t r = i / dim;
  if (r >= n_out) return;
  const int col = (int)(i - r * dim);
  out[r * out_stride + col] = feats[(int64_t)src[r] * stride + col];
}

// ---------------------------------------------------------------- runs
__global__ __launch_bounds__(kThreads) void run_start_flags_kernel(const float *vad, const int64_t *frame_off, int n_utt, int64_t total, int32_t *flags) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  const int u = acc_owner(frame_off, n_utt, g);
  flags[g] = vad[g] != 0.0f && (g == frame_off[u] || vad[g - 1] == 0.0f) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void run_scatter_kernel(const float *vad, const int32_t *flags, const int32_t *G, const int64_t *frame_off,
                                                               int n_utt, int64_t total, int64_t capacity, int32_t *run_begin, int32_t *run_end) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total || vad[g] == 0.0f) return;
  const int u = acc_owner(frame_off, n_utt, g);
  const int64_t t = g - frame_off[u];
  if (flags[g] && G[g] < capacity) run_begin[G[g]] = (int32_t)t;
  if (g + 1 == frame_off[u + 1] || vad[g + 1] == 0.0f) {
    const int64_t r = (int64_t)G[g + 1] - 1;         // run starts up to and including this frame, less one
    if (r < capacity) run_end[r] = (int32_t)(t + 1);
  }
}

__global__ __launch_bounds__(kThreads) void run_offsets_kernel(const int32_t *G, const int64_t *frame_off, int n_utt, int64_t *run_off) {
  const int u = blockIdx.x * kThreads + threadIdx.x;
  if (u <= n_utt) run_off[u] = G[frame_off[u]];
}

}  // namespace

// The scan for the other stages (ctx.hpp): cluster.hip numbers its clusters with it.
size_t mfa_int_scan_blocks(int64_t total) { return (size_t)((total + kVadScanBlock - 1) / kVadScanBlock); }
void mfa_int_scan(mfa_ctx *c, const int32_t *d_v, int64_t total, int32_t *d_bsum, int32_t *d_base, int32_t *d_G) {
  global_scan(c, d_v, total, d_bsum, d_base, d_G);
}

extern "C" {

MFA_API int32_t mfa_vad_scan_block_frames(void) { return kVadScanBlock; }
MFA_API int32_t mfa_vad_scan_totals_threads(void) { return kVadScanThreads; }
MFA_API int32_t mfa_vad_sum_chunk_frames(void) { return kVadSumChunk; }
MFA_API int32_t mfa_sliding_cmvn_tile_frames(void) { return kCmnTile; }

MFA_API int mfa_vad_scan_batch(mfa_ctx *c, const int32_t *d_values, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                               int32_t *d_scan, int32_t *d_totals) {
  if (check_batch(c, "scan", n_utt, total_frames, d_frame_off)) return -1;
  if (n_utt == 0) return 0;
  if (total_frames > 0 && !d_values) return c->fail("scan: no values");
  KernelTimer kt(c, MFA_K_VAD);
  if (total_frames == 0) {
    if (d_totals) MFA_HIP_CHECK(c, hipMemsetAsync(d_totals, 0, (size_t)n_utt * 4, c->stream));
    return 0;
  }
  Workspace ws;
  ScanSpace sp;
  sp.take(ws, total_frames);
  if (ws.reserve(c, "the scan")) return -1;
  int32_t *G = ws.at<int32_t>(sp.G);
  global_scan(c, d_values, total_frames, ws.at<int32_t>(sp.bsum), ws.at<int32_t>(sp.base), G);
  if (d_scan)
    hipLaunchKernelGGL(segment_scan_kernel, dim3(blocks_for(total_frames, kThreads)), dim3(kThreads), 0, c->stream, G, d_frame_off, n_utt, total_frames, d_scan);
  if (d_totals)
    hipLaunchKernelGGL(segment_totals_kernel, dim3(blocks_for(n_utt, kThreads)), dim3(kThreads), 0, c->stream, G, d_frame_off, n_utt, d_totals);
  MFA_DEBUG_POINT(c, "vad scan n_utt %d frames %lld", n_utt, (long long)total_frames);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

MFA_API int mfa_vad_batch(mfa_ctx *c, const float *d_feats, int32_t stride, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                          int32_t max_frames, const mfa_vad_opts *opts, float *d_vad, float *d_thr, int32_t *d_voiced) {
  if (check_batch(c, "VAD", n_utt, total_frames, d_frame_off)) return -1;
  if (!opts) return c->fail("VAD: no options");
  if (stride < 1) return c->fail("VAD: rows of %d floats", stride);
  if (opts->frames_context < 0) return c->fail("VAD: frames_context %d < 0", opts->frames_context);
  if (n_utt == 0) return 0;
  if (!d_thr) return c->fail("VAD: no output for the thresholds");
  if (total_frames > 0 && (!d_feats || !d_vad)) return c->fail("VAD: no input or no output");
  if (max_frames < 0 || max_frames > total_frames) return c->fail("VAD: longest utterance of %d frames in a batch of %lld", max_frames, (long long)total_frames);
  const unsigned chunks = blocks_for(max_frames, kVadSumChunk);
  if (chunks > 65535u) return c->fail("VAD: an utterance of %d frames (at most %d)", max_frames, 65535 * kVadSumChunk);
  Workspace ws;
  ScanSpace sp;
  const size_t o_partial = ws.take(((size_t)(total_frames / kVadSumChunk) + n_utt + 1) * sizeof(double));
  if (total_frames > 0) sp.take(ws, total_frames);
  if (ws.reserve(c, "the VAD's sums and scan")) return -1;
  double *partial = ws.at<double>(o_partial);
  KernelTimer kt(c, MFA_K_VAD);
  if (total_frames > 0)
    hipLaunchKernelGGL(vad_chunk_sums_kernel, dim3(n_utt, chunks), dim3(kThreads), 0, c->stream, d_feats, stride, d_frame_off, partial);
  hipLaunchKernelGGL(vad_threshold_kernel, dim3(blocks_for(n_utt, kThreads)), dim3(kThreads), 0, c->stream, d_frame_off, n_utt, partial, *opts, d_thr, d_voiced);
  if (total_frames > 0) {
    const dim3 grid(blocks_for(total_frames, kThreads));
    int32_t *flags = ws.at<int32_t>(sp.flags), *G = ws.at<int32_t>(sp.G);
    hipLaunchKernelGGL(vad_flags_kernel, grid, dim3(kThreads), 0, c->stream, d_feats, stride, d_frame_off, n_utt, total_frames, d_thr, flags);
    global_scan(c, flags, total_frames, ws.at<int32_t>(sp.bsum), ws.at<int32_t>(sp.base), G);
    hipLaunchKernelGGL(vad_decide_kernel, grid, dim3(kThreads), 0, c->stream, G, d_frame_off, n_utt, total_frames, *opts, d_vad, d_voiced);
  }
  MFA_DEBUG_POINT(c, "vad n_utt %d frames %lld", n_utt, (long long)total_frames);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

MFA_API int mfa_sliding_cmvn_batch(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int32_t max_frames, int32_t dim,
                                   int32_t stride, const mfa_sliding_cmvn_opts *opts, float *d_out) {
  if (!opts) return c->fail("sliding CMVN: no options");
  if (n_utt < 0 || max_frames < 0) return c->fail("sliding CMVN: negative sizes");
  if (dim < 1 || stride < dim) return c->fail("sliding CMVN: %d columns do not lie inside a row of %d", dim, stride);
  if (opts->cmn_window < 1 || opts->min_window < 1) return c->fail("sliding CMVN: cmn_window %d, min_window %d (both at least 1)", opts->cmn_window, opts->min_window);
  if (n_utt == 0 || max_frames == 0) return 0;
  if (!d_feats || !d_frame_off || !d_out) return c->fail("sliding CMVN: no input or no output");
  if (d_out == d_feats) return c->fail("sliding CMVN: the output may not be the input (a frame's window reads its neighbours)");
  const int64_t lanes = ((int64_t)max_frames + kCmnTile - 1) / kCmnTile * stride;
  const int64_t gy = (lanes + kThreads - 1) / kThreads;
  if (gy > 65535) return c->fail("sliding CMVN: an utterance of %d frames by %d columns is beyond one launch", max_frames, stride);
  KernelTimer kt(c, MFA_K_VAD);
  hipLaunchKernelGGL(sliding_cmvn_kernel, dim3(n_utt, (unsigned)gy), dim3(kThreads), 0, c->stream, d_feats, d_frame_off, dim, stride, *opts, d_out);
  MFA_DEBUG_POINT(c, "sliding cmvn n_utt %d max_frames %d", n_utt, max_frames);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

MFA_API int mfa_select_frames_count(mfa_ctx *c, const float *d_vad, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames, int32_t n,
                                    int32_t *d_src, int64_t *d_out_off) {
  if (check_batch(c, "frame selection", n_utt, total_frames, d_frame_off)) return -1;
  if (n < 1) return c->fail("frame selection: subsample factor %d (at least 1; Kaldi's negative offsets are not built)", n);
  if (!d_out_off) return c->fail("frame selection: no output for the offsets");
  if (total_frames > 0 && !d_src) return c->fail("frame selection: no output for the row map");
  KernelTimer kt(c, MFA_K_VAD);
  if (total_frames == 0) {
    MFA_HIP_CHECK(c, hipMemsetAsync(d_out_off, 0, ((size_t)n_utt + 1) * 8, c->stream));
    return 0;
  }
  Workspace ws;
  ScanSpace sp;
  sp.take(ws, total_frames);
  if (ws.reserve(c, "the selection's scan")) return -1;
  int32_t *flags = ws.at<int32_t>(sp.flags), *G = ws.at<int32_t>(sp.G);
  const dim3 grid(blocks_for(total_frames, kThreads));
  hipLaunchKernelGGL(keep_flags_kernel, grid, dim3(kThreads), 0, c->stream, d_vad, total_frames, flags);
  global_scan(c, flags, total_frames, ws.at<int32_t>(sp.bsum), ws.at<int32_t>(sp.base), G);
  hipLaunchKernelGGL((acc_scan_kernel<1, SelectOffsets>), dim3(1), dim3(256), 0, c->stream, SelectOffsets{G, d_frame_off, n, d_out_off}, (int)n_utt);
  hipLaunchKernelGGL(select_map_kernel, grid, dim3(kThreads), 0, c->stream, flags, G, d_frame_off, n_utt, total_frames, n, d_out_off, d_src);
  MFA_DEBUG_POINT(c, "select frames n_utt %d frames %lld n %d", n_utt, (long long)total_frames, n);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

MFA_API int mfa_select_frames_batch(mfa_ctx *c, const float *d_feats, int32_t stride, int32_t dim, const int32_t *d_src, int64_t n_out,
                                    float *d_out, int32_t out_stride) {
  if (dim < 1 || stride < dim || out_stride < dim) return c->fail("frame selection: %d columns do not lie inside rows of %d and %d", dim, stride, out_stride);
  if (n_out < 0 || n_out >= ((int64_t)1 << 31)) return c->fail("frame selection: %lld output rows", (long long)n_out);
  if (n_out == 0) return 0;
  if (!d_feats || !d_src || !d_out) return c->fail("frame selection: no input, no row map or no output");
  const int64_t blocks = (n_out * dim + kThreads - 1) / kThreads;
  if (blocks >= ((int64_t)1 << 31)) return c->fail("frame selection: %lld rows of %d columns are beyond one launch", (long long)n_out, dim);
  KernelTimer kt(c, MFA_K_VAD);
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, c->stream, d_feats, stride, dim, d_src, n_out, d_out, out_stride);
  MFA_DEBUG_POINT(c, "gather rows %lld x %d", (long long)n_out, dim);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

MFA_API int mfa_vad_runs_batch(mfa_ctx *c, const float *d_vad, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames, int64_t capacity,
                               int32_t *d_run_begin, int32_t *d_run_end, int64_t *d_run_off) {
  if (check_batch(c, "voiced runs", n_utt, total_frames, d_frame_off)) return -1;
  if (capacity < 0) return c->fail("voiced runs: capacity %lld", (long long)capacity);
  if (!d_run_off) return c->fail("voiced runs: no output for the offsets");
  if (capacity > 0 && (!d_run_begin || !d_run_end)) return c->fail("voiced runs: no output for the runs");
  if (total_frames > 0 && !d_vad) return c->fail("voiced runs: no input");
  KernelTimer kt(c, MFA_K_VAD);
  if (total_frames == 0) {
    MFA_HIP_CHECK(c, hipMemsetAsync(d_run_off, 0, ((size_t)n_utt + 1) * 8, c->stream));
    return 0;
  }
  Workspace ws;
  ScanSpace sp;
  sp.take(ws, total_frames);
  if (ws.reserve(c, "the runs' scan")) return -1;
  int32_t *flags = ws.at<int32_t>(sp.flags), *G = ws.at<int32_t>(sp.G);
  const dim3 grid(blocks_for(total_frames, kThreads));
  hipLaunchKernelGGL(run_start_flags_kernel, grid, dim3(kThreads), 0, c->stream, d_vad, d_frame_off, n_utt, total_frames, flags);
  global_scan(c, flags, total_frames, ws.at<int32_t>(sp.bsum), ws.at<int32_t>(sp.base), G);
  hipLaunchKernelGGL(run_scatter_kernel, grid, dim3(kThreads), 0, c->stream, d_vad, flags, G, d_frame_off, n_utt, total_frames, capacity, d_run_begin, d_run_end);
  hipLaunchKernelGGL(run_offsets_kernel, dim3(blocks_for((int64_t)n_utt + 1, kThreads)), dim3(kThreads), 0, c->stream, G, d_frame_off, n_utt, d_run_off);
  MFA_DEBUG_POINT(c, "vad runs n_utt %d frames %lld", n_utt, (long long)total_frames);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

}  // extern "C"
