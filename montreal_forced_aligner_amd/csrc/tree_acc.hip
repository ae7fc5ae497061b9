// Tree statistics on gfx950: the accumulation of the reference's triphone stage (TreeStatsFunction → kalpy
// TreeStatsAccumulator, Kaldi acc-tree-stats): per (left phone, centre phone, right phone, pdf-class) a count, Σx and Σx².
// Contract: include/mfa_hip.h "Tree statistics"; what the host twin (tree_acc_host.cpp) shares: tree_acc_math.hpp.
//
//   keys    tree_keys_kernel, one wavefront per utterance, 64 frames a step.  Forward: the segments (runs of frames that end
//           at a final transition-id and the self-loops after it: reordered alignments) from wave-level scans over the
//           frames' flags, the open segment's phone and left neighbour carried across steps; the utterance's validity.
//           Backward, for an utterance that takes part: the right neighbour the same way, and the frame's sort key.
//   order   rocPRIM radix_sort_pairs (stable) of (key, frame index): an event lists its frames in ascending frame index.
//           Heads of runs flagged, rocPRIM inclusive_scan: the event of every sorted position; tree_events_kernel writes
//           frame_event, the events' first positions, their keys and n_events.
//   sums    tree_small_kernel, wavefronts striding over the events: an event of at most one chunk is summed and written; a
//           longer one gets a run of partial rows (an integer atomic hands out the rows: where they lie is not part of the
//           result).  tree_big_kernel, wavefronts striding over those (event, chunk) units; tree_big_reduce_kernel adds an
//           event's partials in chunk order.  The workspace is carved by acc_segments.hpp's Workspace.
// A unit is a wavefront: lane = column, the rows of 16 frames fetched whole through the sorted index (all 64 lanes load),
// staged in the wavefront's own LDS slice and added in frame order.  No floating-point atomics anywhere.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "acc_segments.hpp"
#include "ctx.hpp"
#include "tree_acc_math.hpp"

namespace {

constexpr int kChunk = kTreeChunk;
constexpr int kRows = 16;                                  // frames staged at a time by a wavefront
constexpr int kTileFloats = kRows * kTreeMaxDim;           // 768 floats = 3 KiB a wavefront
constexpr int kLoads = kTileFloats / 64;                   // loads a lane issues for a full tile
constexpr int kWaves = 4;                                  // independent wavefronts of a workgroup
static_assert(kTileFloats % 64 == 0 && kChunk % kRows == 0, "tree_chunk_sum tiling");

#define TREE_WAVE_SYNC()                                     \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)

__global__ __launch_bounds__(256) void tree_init_kernel(uint64_t *key, uint32_t *val, int64_t n, uint64_t none) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) { key[t] = none; val[t] = (uint32_t)t; }
}

struct KeyParams {
  const int32_t *ali; const int64_t *frame_off; int32_t n_utt; int64_t n;
  const int32_t *tid_phone, *tid_class, *tid_flags; int32_t n_tids;
  const uint8_t *phone_ci; int32_t n_phones; int bits;
  int32_t *left;                   // [n] scratch: the left neighbour of the frame's segment | kEndBit if the frame ends it
  uint64_t *key;                   // [n] sort keys, initialised to "takes no part"
  unsigned long long *skipped;
};

constexpr int32_t kEndBit = 1 << 30;   // above every phone id (kTreeMaxPhones)

// What a lane knows of its frame: whether the frame and its table entries are usable, its phone, pdf-class and flags.
struct TreeFrame { bool ok; int32_t phone, cls, flags; };
__device__ inline TreeFrame tree_frame(const KeyParams &p, int64_t t, bool in) {
  TreeFrame f{false, 0, 0, 0};
  const int32_t tid = in ? p.ali[t] : 0;
  if (in && tree_tid_ok(tid, p.n_tids)) {
    const int32_t phone = p.tid_phone[tid], cls = p.tid_class[tid];
    if (tree_entry_ok(phone, cls, p.n_phones)) { f.ok = true; f.phone = phone; f.cls = cls; f.flags = p.tid_flags[tid]; }
  }
  return f;
}

// grid: ceil(n_utt / 4) workgroups of 4 wavefronts; wavefront = utterance.
__global__ __launch_bounds__(256) void tree_keys_kernel(KeyParams p) {
  const int lane = threadIdx.x & 63, u = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (u >= p.n_utt) return;
  const int64_t f0 = p.frame_off[u], f1 = p.frame_off[u + 1];
  if (f0 < 0 || f1 <= f0 || f1 > p.n) return;            // empty, or offsets that do not describe the batch: nothing is read
  const unsigned long long upto = ~0ull >> (63 - lane);    // lanes 0..lane

  // forward: a frame is in its segment's tail when the nearest frame at or before it that is no plain self-loop is final
  // (tree_tail, as a scan); the segment ends at the tail frame no self-loop follows; the next one starts after it
  bool bad = false, carry_final = true, carry_tail = false;
  int32_t carry_phone = 0, carry_left = 0, carry_last = 0;  // the open segment's phone and left neighbour; the last frame's phone
  for (int64_t b = f0; b < f1; b += 64) {
    const int64_t t = b + lane;
    const bool in = t < f1;
    const TreeFrame f = tree_frame(p, t, in);
    const int32_t next_tid = t + 1 < f1 ? p.ali[t + 1] : 0;
    const int32_t next_flags = tree_tid_ok(next_tid, p.n_tids) ? p.tid_flags[next_tid] : 0;
    const unsigned long long final_mask = __ballot((f.flags & kTreeFinal) != 0);
    const unsigned long long anchors = __ballot(tree_tail(f.flags, false) || !tree_tail(f.flags, true));   // final, or no self-loop
    const unsigned long long am = anchors & upto;
    const bool tail = am ? ((final_mask >> (63 - __clzll((long long)am))) & 1ull) != 0 : carry_tail && tree_tail(f.flags, true);
    const bool end = in && tree_segment_end(tail, next_flags);
    const unsigned long long finals = __ballot(end);
    const unsigned long long starts = (finals << 1) | (carry_final ? 1ull : 0ull);
    const unsigned long long m = starts & upto;
    const int src = m ? 63 - __clzll((long long)m) : -1;    // the lane that opens this lane's segment, or an earlier step
    const int32_t before = __shfl_up(f.phone, 1);            // lane - 1's phone
    const int32_t prev = lane == 0 ? carry_last : before;    // the phone of the frame before this one (0 at the start)
    const int32_t sp = __shfl(f.phone, src < 0 ? 0 : src), sl = __shfl(prev, src < 0 ? 0 : src);
    const int32_t seg_phone = src >= 0 ? sp : carry_phone, seg_left = src >= 0 ? sl : carry_left;
    if (in && (!f.ok || f.phone != seg_phone)) bad = true;
    if (in) p.left[t] = seg_left | (end ? kEndBit : 0);
    const int last = (int)min((int64_t)63, f1 - 1 - b);
    carry_tail = __shfl((int)tail, last) != 0;
    carry_phone = __shfl(seg_phone, last);
    carry_left = __shfl(seg_left, last);
    carry_last = __shfl(f.phone, last);
    carry_final = (finals >> last) & 1ull;
  }
  if (__ballot(bad) != 0ull || !carry_final) {
    if (lane == 0) atomicAdd(p.skipped, 1ull);
    return;
  }

  // backward: the right neighbour is the phone of the frame after the segment's last one (0 at the utterance's end)
  int32_t carry_right = 0, carry_first = 0;                // of the segment open at the later step; the later step's first phone
  const int64_t steps = (f1 - f0 + 63) >> 6;
  for (int64_t k = steps - 1; k >= 0; k--) {
    const int64_t b = f0 + (k << 6), t = b + lane;
    const bool in = t < f1;
    const TreeFrame f = tree_frame(p, t, in);
    const int32_t packed = in ? p.left[t] : 0;               // this lane's own store of the forward pass
    const unsigned long long finals = __ballot((packed & kEndBit) != 0);
    const int32_t after = __shfl_down(f.phone, 1);          // lane + 1's phone: 0 past the utterance's end
    const int32_t next = lane == 63 ? carry_first : after;
    const unsigned long long m = finals >> lane;
    const int end = m ? lane + __ffsll((long long)m) - 1 : 0;
    const int32_t nr = __shfl(next, end);
    const int32_t right = m ? nr : carry_right;
    if (in) {
      const uint64_t key = tree_event_key(packed & ~kEndBit, f.phone, right, f.cls, p.phone_ci[f.phone] != 0);
      p.key[t] = tree_sort_key(key, p.bits);
    }
    carry_right = __shfl(right, 0);
    carry_first = __shfl(f.phone, 0);
  }
}

__global__ __launch_bounds__(256) void tree_heads_kernel(const uint64_t *key, int64_t n, uint64_t none, uint32_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  flag[i] = k < none && (i == 0 || key[i - 1] != k) ? 1u : 0u;
}

struct EventParams {
  const uint64_t *key; const uint32_t *val; const uint32_t *rank; int64_t n; uint64_t none; int bits; int64_t cap;
  int32_t *frame_event; int32_t *ev_start;   // ev_start [n + 1]: first sorted position of every event, then the end of the last
  int64_t *n_events; uint64_t *ev_key;
};

// One thread per sorted position.  rank[i] = heads among positions 0..i, so rank[n - 1] is the number of events.
__global__ __launch_bounds__(256) void tree_events_kernel(EventParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t k = p.key[i];
  const bool part = k < p.none, first = i == 0 || p.key[i - 1] != k;
  const uint32_t r = p.rank[i], ne = p.rank[p.n - 1];
  p.frame_event[p.val[i]] = part ? (int32_t)r - 1 : -1;
  if (part && first) {
    p.ev_start[r - 1] = (int32_t)i;
    if ((int64_t)ne <= p.cap) p.ev_key[r - 1] = tree_key_of_sort_key(k, p.bits);
  }
  if (!part && first) p.ev_start[r] = (int32_t)i;          // the first frame that takes no part closes the last event
  if (i == p.n - 1) {
    if (part) p.ev_start[r] = (int32_t)p.n;
    *p.n_events = (int64_t)ne;
  }
}

// Σx and Σx² of column `lane` over sorted positions [s0, s0 + n), from zero, in order.  The whole wavefront calls it.
// (row0, col0): row and column of element `lane` of a tile; (dq, dr): 64 = dq·dim + dr.
__device__ inline void tree_chunk_sum(const float *feats, const uint32_t *idx, int s0, int n, int dim, float *tile, int lane,
                                      int row0, int col0, int dq, int dr, double &sum, double &sumsq) {
  sum = 0.0; sumsq = 0.0;
  float v[kLoads];
  auto fetch = [&](int r0) {
    const int ne = min(kRows, n - r0) * dim;
    int row = row0, col = col0;
#pragma unroll
    for (int j = 0; j < kLoads; j++) {
      v[j] = lane + 64 * j < ne ? feats[(size_t)idx[s0 + r0 + row] * dim + col] : 0.0f;
      row += dq; col += dr;
      if (col >= dim) { col -= dim; row++; }
    }
  };
  fetch(0);
  for (int r0 = 0; r0 < n; r0 += kRows) {
    const int nr = min(kRows, n - r0);
    TREE_WAVE_SYNC();                                      // the previous tile's readers are done
#pragma unroll
    for (int j = 0; j < kLoads; j++) tile[lane + 64 * j] = v[j];
    TREE_WAVE_SYNC();
    if (r0 + kRows < n) fetch(r0 + kRows);                 // in flight while this tile is added
    if (lane < dim)
      for (int r = 0; r < nr; r++) tree_acc_add(tile[r * dim + lane], sum, sumsq);
  }
}

struct SumParams {
  const float *feats; const uint32_t *idx; const int32_t *ev_start; const int64_t *n_events; int64_t cap; int dim;
  int64_t *ev_count; double *ev_sum, *ev_sumsq;
  int32_t *counters;               // {big events, big units}
  int32_t *big_ev;                 // [big events][2]: event, first partial row
  int32_t *unit_desc;              // [big units][2]: event, chunk
  double *partial;                 // [big units][2·dim]
  int32_t big_ev_cap, unit_cap;
};

struct WaveIds { int lane, wave, gwave, nwaves, row0, col0, dq, dr; };
__device__ inline WaveIds tree_wave_ids(int dim) {
  WaveIds w;
  w.lane = threadIdx.x & 63; w.wave = threadIdx.x >> 6;
  w.gwave = blockIdx.x * kWaves + w.wave; w.nwaves = gridDim.x * kWaves;
  w.row0 = w.lane / dim; w.col0 = w.lane - w.row0 * dim; w.dq = 64 / dim; w.dr = 64 - w.dq * dim;
  return w;
}

__global__ __launch_bounds__(256) void tree_small_kernel(SumParams p) {
  __shared__ float tiles[kWaves][kTileFloats];
  const int64_t ne = *p.n_events;
  if (ne > p.cap) return;
  const int dim = p.dim;
  const WaveIds w = tree_wave_ids(dim);
  for (int64_t e = w.gwave; e < ne; e += w.nwaves) {
    const int s0 = p.ev_start[e], n = p.ev_start[e + 1] - s0;
    if (w.lane == 0) p.ev_count[e] = n;
    if (n <= kChunk) {
      double sum, sumsq;
      tree_chunk_sum(p.feats, p.idx, s0, n, dim, tiles[w.wave], w.lane, w.row0, w.col0, w.dq, w.dr, sum, sumsq);
      if (w.lane < dim) { p.ev_sum[(size_t)e * dim + w.lane] = sum; p.ev_sumsq[(size_t)e * dim + w.lane] = sumsq; }
    } else {
      const int nch = (n + kChunk - 1) / kChunk;
      int slot = 0, base = 0;
      if (w.lane == 0) { slot = atomicAdd(&p.counters[0], 1); base = atomicAdd(&p.counters[1], nch); }
      slot = __shfl(slot, 0); base = __shfl(base, 0);
      if (slot < p.big_ev_cap && base + nch <= p.unit_cap) {   // always: the bounds are those of the workspace's arithmetic
        if (w.lane == 0) { p.big_ev[2 * slot] = (int32_t)e; p.big_ev[2 * slot + 1] = base; }
        for (int k = w.lane; k < nch; k += 64) { p.unit_desc[2 * (base + k)] = (int32_t)e; p.unit_desc[2 * (base + k) + 1] = k; }
      }
    }
  }
}

__global__ __launch_bounds__(256) void tree_big_kernel(SumParams p) {
  __shared__ float tiles[kWaves][kTileFloats];
  if (*p.n_events > p.cap) return;
  const int dim = p.dim;
  const WaveIds w = tree_wave_ids(dim);
  const int nu = min(p.counters[1], p.unit_cap);
  for (int u = w.gwave; u < nu; u += w.nwaves) {
    const int e = p.unit_desc[2 * u], k = p.unit_desc[2 * u + 1];
    const int s0 = p.ev_start[e] + k * kChunk, n = min(kChunk, p.ev_start[e + 1] - s0);
    double sum, sumsq;
    tree_chunk_sum(p.feats, p.idx, s0, n, dim, tiles[w.wave], w.lane, w.row0, w.col0, w.dq, w.dr, sum, sumsq);
    if (w.lane < dim) { p.partial[(size_t)u * 2 * dim + w.lane] = sum; p.partial[(size_t)u * 2 * dim + dim + w.lane] = sumsq; }
  }
}

// Wavefronts striding over the long events: lane = column; the event's partials in chunk order, from the first one (an
// event's row is written, not added to).  acc_ordered_sum's order (acc_segments.hpp), for Σx and Σx² at once: the 16 loads of
// 8 chunks are issued together.  Two calls of acc_ordered_sum gave the same bits and cost 1 % of the sums stage
// (1.177 ms against 1.165 ms at tools/tree_acc_rate.py's shape), so the loop stays here.
__global__ __launch_bounds__(256) void tree_big_reduce_kernel(SumParams p) {
  if (*p.n_events > p.cap) return;
  const int dim = p.dim;
  const WaveIds w = tree_wave_ids(dim);
  const int nb = min(p.counters[0], p.big_ev_cap);
  if (w.lane >= dim) return;
  for (int s = w.gwave; s < nb; s += w.nwaves) {
    const int e = p.big_ev[2 * s], base = p.big_ev[2 * s + 1];
    const int nch = (p.ev_start[e + 1] - p.ev_start[e] + kChunk - 1) / kChunk;
    const double *src = p.partial + (size_t)base * 2 * dim + w.lane;
    double a = src[0], b = src[dim];
    int ch = 1;
    for (; ch + 8 <= nch; ch += 8) {
      double va[8], vb[8];
#pragma unroll
      for (int i = 0; i < 8; i++) { va[i] = src[(size_t)(ch + i) * 2 * dim]; vb[i] = src[(size_t)(ch + i) * 2 * dim + dim]; }
#pragma unroll
      for (int i = 0; i < 8; i++) { a += va[i]; b += vb[i]; }
    }
    for (; ch < nch; ch++) { a += src[(size_t)ch * 2 * dim]; b += src[(size_t)ch * 2 * dim + dim]; }
    p.ev_sum[(size_t)e * dim + w.lane] = a;
    p.ev_sumsq[(size_t)e * dim + w.lane] = b;
  }
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_tree_acc_chunk_frames(void) { return kChunk; }
MFA_API int32_t mfa_tree_acc_max_dim(void) { return kTreeMaxDim; }

MFA_API int mfa_tree_acc_batch(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                               int32_t dim, const int32_t *d_ali, const int32_t *d_tid_phone, const int32_t *d_tid_class,
                               const int32_t *d_tid_flags, int32_t n_tids, const uint8_t *d_phone_ci, int32_t n_phones,
                               int64_t cap, int32_t *d_frame_event, int64_t *d_n_events, int64_t *d_skipped, uint64_t *d_ev_key,
                               int64_t *d_ev_count, double *d_ev_sum, double *d_ev_sumsq) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (dim <= 0) return c->fail("tree statistics: feature dim %d", dim);
  if (dim > kTreeMaxDim) return c->fail("tree statistics: feature dim %d > %d (the GMM statistics' limit)", dim, kTreeMaxDim);
  if (n_utt < 0 || total_frames < 0 || cap < 0) return c->fail("tree statistics: negative count (utterances %d, frames %lld, event rows %lld)", n_utt, (long long)total_frames, (long long)cap);
  if (n_phones < 0 || n_phones >= kTreeMaxPhones) return c->fail("tree statistics: %d phones (the key holds phone ids below %d)", n_phones, kTreeMaxPhones);
  if (total_frames >= ((int64_t)1 << 31)) return c->fail("tree statistics: %lld frames in one call (at most 2^31 - 1)", (long long)total_frames);
  if (!d_n_events || !d_skipped) return c->fail("tree statistics: NULL output array");
  MFA_HIP_CHECK(c, hipMemsetAsync(d_n_events, 0, 8, c->stream));
  MFA_HIP_CHECK(c, hipMemsetAsync(d_skipped, 0, 8, c->stream));
  if (total_frames == 0 || n_utt == 0) return 0;
  if (n_tids <= 0) return c->fail("tree statistics: empty transition-id table");
  if (!d_feats || !d_frame_off || !d_ali || !d_tid_phone || !d_tid_class || !d_tid_flags || !d_phone_ci) return c->fail("tree statistics: NULL input array");
  if (!d_frame_event || (cap > 0 && (!d_ev_key || !d_ev_count || !d_ev_sum || !d_ev_sumsq))) return c->fail("tree statistics: NULL output array");

  const int cus = mfa_num_cus(c);
  if (cus <= 0) return c->fail("tree statistics: the device's compute units could not be queried");
  const size_t T = (size_t)total_frames;
  const int bits = tree_phone_bits(n_phones);
  const uint64_t none = tree_sort_key(kTreeNoKey, bits);
  const unsigned end_bit = (unsigned)(3 * bits + 9);
  const size_t big_ev_cap = T / kChunk + 1, unit_cap = 2 * (T / kChunk) + 2;   // events longer than a chunk; Σ ceil(n / chunk) over them
  size_t sort_bytes = 0, scan_bytes = 0;
  MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, T, 0u, end_bit, c->stream));
  MFA_HIP_CHECK(c, rocprim::inclusive_scan(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, T, rocprim::plus<uint32_t>(), c->stream));
  Workspace ws;
  const size_t o_key = ws.take(T * 8), o_key2 = ws.take(T * 8), o_val = ws.take(T * 4), o_val2 = ws.take(T * 4), o_left = ws.take(T * 4),
               o_rank = ws.take(T * 4), o_start = ws.take((T + 1) * 4), o_cnt = ws.take(8), o_big = ws.take(big_ev_cap * 8),
               o_desc = ws.take(unit_cap * 8), o_part = ws.take(unit_cap * 2 * (size_t)dim * 8),
               o_tmp = ws.take(std::max(sort_bytes, scan_bytes));
  if (ws.reserve(c, "the tree statistics workspace")) return -1;
  uint64_t *key = ws.at<uint64_t>(o_key), *key2 = ws.at<uint64_t>(o_key2);
  uint32_t *val = ws.at<uint32_t>(o_val), *val2 = ws.at<uint32_t>(o_val2), *rank = ws.at<uint32_t>(o_rank);
  uint32_t *flag = ws.at<uint32_t>(o_left);                // the left neighbours are done with when the heads are flagged
  int32_t *left = ws.at<int32_t>(o_left), *ev_start = ws.at<int32_t>(o_start), *counters = ws.at<int32_t>(o_cnt);
  const unsigned frame_blocks = (unsigned)((T + 255) / 256);

  {
    KernelTimer kt(c, MFA_K_TREE_KEYS);
    hipLaunchKernelGGL(tree_init_kernel, dim3(frame_blocks), dim3(256), 0, c->stream, key, val, total_frames, none);
    KeyParams kp{d_ali, d_frame_off, n_utt, total_frames, d_tid_phone, d_tid_class, d_tid_flags, n_tids, d_phone_ci, n_phones, bits,
                 left, key, (unsigned long long *)d_skipped};
    hipLaunchKernelGGL(tree_keys_kernel, dim3((unsigned)((n_utt + kWaves - 1) / kWaves)), dim3(256), 0, c->stream, kp);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  {
    KernelTimer kt(c, MFA_K_TREE_ORDER);
    MFA_HIP_CHECK(c, rocprim::radix_sort_pairs(ws.at<char>(o_tmp), sort_bytes, key, key2, val, val2, T, 0u, end_bit, c->stream));
    hipLaunchKernelGGL(tree_heads_kernel, dim3(frame_blocks), dim3(256), 0, c->stream, key2, total_frames, none, flag);
    MFA_HIP_CHECK(c, rocprim::inclusive_scan(ws.at<char>(o_tmp), scan_bytes, flag, rank, T, rocprim::plus<uint32_t>(), c->stream));
    EventParams ep{key2, val2, rank, total_frames, none, bits, cap, d_frame_event, ev_start, d_n_events, d_ev_key};
    hipLaunchKernelGGL(tree_events_kernel, dim3(frame_blocks), dim3(256), 0, c->stream, ep);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  if (cap > 0) {
    KernelTimer kt(c, MFA_K_TREE_SUMS);
    MFA_HIP_CHECK(c, hipMemsetAsync(counters, 0, 8, c->stream));
    SumParams sp{d_feats, val2, ev_start, d_n_events, cap, dim, d_ev_count, d_ev_sum, d_ev_sumsq, counters,
                 ws.at<int32_t>(o_big), ws.at<int32_t>(o_desc), ws.at<double>(o_part), (int32_t)big_ev_cap, (int32_t)unit_cap};
    // eight workgroups a CU at the most: a wavefront walks the events (units) its stride gives it
    const size_t ev_max = std::min(T, (size_t)cap);
    const unsigned g_small = (unsigned)std::min((ev_max + kWaves - 1) / kWaves, (size_t)cus * 8);
    const unsigned g_big = (unsigned)std::min((unit_cap + kWaves - 1) / kWaves, (size_t)cus * 8);
    const unsigned g_red = (unsigned)std::min((big_ev_cap + kWaves - 1) / kWaves, (size_t)cus * 8);
    hipLaunchKernelGGL(tree_small_kernel, dim3(g_small), dim3(256), 0, c->stream, sp);
    hipLaunchKernelGGL(tree_big_kernel, dim3(g_big), dim3(256), 0, c->stream, sp);
    hipLaunchKernelGGL(tree_big_reduce_kernel, dim3(g_red), dim3(256), 0, c->stream, sp);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  return 0;
}

}  // extern "C"
