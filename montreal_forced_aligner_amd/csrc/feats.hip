// CMVN statistics and final-feature kernels for gfx950.
//   mfa_cmvn_stats : per-speaker Σx, Σx², count in float64 (Kaldi AccCmvnStats), deterministic order.
//   mfa_feats_batch: ApplyCmvn → Δ+ΔΔ (Kaldi DeltaFeatures order 2 window 2) (+fMLLR) or splice(±ctx)+LDA(+fMLLR)
//                    (Kaldi SpliceFrames / ApplyAffineTransform; Appendix A.3) — the chain of
//                    MFA/alignment/multiprocessing.py:1287-1304 / MFA/db.py:2101-2136.
// HBM-bound streaming stages: each input row is read once per tile (+halo) and each output row written once.
// -ffp-contract=off: the fmaf() chains below are exactly the oracle's.
#include <algorithm>
#include <cstdlib>

#include "ctx.hpp"

namespace {

constexpr int kTile = 64;       // frames per block
constexpr int kMaxDim = 16;     // base feature dim (13 MFCC; 16 with pitch)
constexpr int kMaxOut = 64;     // LDA rows
constexpr size_t kMaxLdsBytes = 64 << 10;   // dynamic LDS of a launch that sets no function attribute

// ---- CMVN statistics -------------------------------------------------------------------------------------------
// One block per utterance: thread (stripe s = tid/16, dim d = tid%16) sums frames s, s+16, … in double; the 16
// stripes are then added in stripe order.  Output: per-utterance partial [2][dim+1].
__global__ __launch_bounds__(256) void cmvn_utt_kernel(const float *__restrict__ feats, const int64_t *__restrict__ frame_off,
                                                       int dim, double *__restrict__ partial) {
  __shared__ double sx[16][kMaxDim], sxx[16][kMaxDim];
  const int utt = blockIdx.x, d = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int64_t f0 = frame_off[utt];
  const int T = (int)(frame_off[utt + 1] - f0);
  double a = 0.0, b = 0.0;
  if (d < dim)
    for (int t = s; t < T; t += 16) {
      float x = feats[(f0 + t) * dim + d];
      a += (double)x;
      b += (double)(x * x);
    }
  sx[s][d] = a; sxx[s][d] = b;
  __syncthreads();
  if (s == 0 && d < dim) {
    double ta = 0.0, tb = 0.0;
    for (int k = 0; k < 16; k++) { ta += sx[k][d]; tb += sxx[k][d]; }
    partial[(size_t)utt * 2 * (dim + 1) + d] = ta;
    partial[(size_t)utt * 2 * (dim + 1) + (dim + 1) + d] = tb;
  }
  if (threadIdx.x == 0) {
    partial[(size_t)utt * 2 * (dim + 1) + dim] = (double)T;
    partial[(size_t)utt * 2 * (dim + 1) + (dim + 1) + dim] = 0.0;
  }
}

// One thread per (speaker, stat entry): adds the speaker's utterance partials in list order.
__global__ void cmvn_spk_kernel(const double *__restrict__ partial, const int32_t *__restrict__ spk_utt_off,
                                const int32_t *__restrict__ spk_utt, int n_spk, int dim, double *__restrict__ stats) {
  const int width = 2 * (dim + 1);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_spk * width) return;
  const int spk = idx / width, e = idx % width;
  double acc = 0.0;
  for (int k = spk_utt_off[spk]; k < spk_utt_off[spk + 1]; k++) acc += partial[(size_t)spk_utt[k] * width + e];
  stats[idx] = acc;
}

// ---- final features --------------------------------------------------------------------------------------------
struct FeatParams {
  int dim, mode, ctx, lda_rows, lda_cols;
  const float *mfcc; const int64_t *frame_off; const int32_t *utt2spk; const double *cmvn;
  const float *lda; const float *fmllr; float *out;
};

// Kaldi DeltaFeatures scales for order 2, window 2 (float arithmetic of feature-functions.cc: each level is
// Σ_j j·prev(k) scaled by 1/Σj²).
__constant__ float kDelta1[5];
__constant__ float kDelta2[9];

__global__ __launch_bounds__(256) void feats_kernel(FeatParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int utt = blockIdx.y;
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const int t0 = blockIdx.x * kTile;
  if (t0 >= T) return;
  const int halo = (p.mode == 0) ? 4 : p.ctx;
  const int rows = kTile + 2 * halo;
  float *x = smem;                       // [rows][dim] CMVN-applied base features (frame t0-halo+r, clamped)
  float *mat = x + rows * p.dim;         // mode 1: LDA [lda_rows][lda_cols] then fMLLR [lda_rows][lda_rows+1]
                                         // mode 0 with fMLLR: the speaker's matrix [3·dim][3·dim+1]
  const int od0 = 3 * p.dim;
  float *y = mat + (p.mode == 1 ? p.lda_rows * p.lda_cols + p.lda_rows * (p.lda_rows + 1)
                                : (p.fmllr ? od0 * (od0 + 1) : 0));  // [kTile][lda_rows] | [kTile][3·dim] Δ rows before fMLLR
  // CMVN offsets (Kaldi ApplyCmvn without variance normalisation): offset = (float)(-mean)
  const int spk = p.utt2spk ? p.utt2spk[utt] : 0;
  for (int i = threadIdx.x; i < rows * p.dim; i += blockDim.x) {
    int r = i / p.dim, d = i % p.dim;
    int t = t0 - halo + r;
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    float v = p.mfcc[(f0 + t) * p.dim + d];
    if (p.cmvn) {
      const double *st = p.cmvn + (size_t)spk * 2 * (p.dim + 1);
      float offset = (float)(-(st[d] / st[p.dim]));
      v += offset;
    }
    x[i] = v;
  }
  if (p.mode == 1) {
    for (int i = threadIdx.x; i < p.lda_rows * p.lda_cols; i += blockDim.x) mat[i] = p.lda[i];
    if (p.fmllr) {
      const float *fm = p.fmllr + (size_t)spk * p.lda_rows * (p.lda_rows + 1);
      float *fdst = mat + p.lda_rows * p.lda_cols;
      for (int i = threadIdx.x; i < p.lda_rows * (p.lda_rows + 1); i += blockDim.x) fdst[i] = fm[i];
    }
  } else if (p.fmllr) {
    const float *fm = p.fmllr + (size_t)spk * od0 * (od0 + 1);
    for (int i = threadIdx.x; i < od0 * (od0 + 1); i += blockDim.x) mat[i] = fm[i];
  }
  __syncthreads();
  if (p.mode == 0) {
    const int od = 3 * p.dim;
    for (int i = threadIdx.x; i < kTile * od; i += blockDim.x) {
      int r = i / od, c = i % od, t = t0 + r;
      if (t >= T) continue;
      int level = c / p.dim, d = c % p.dim;
      float acc = 0.0f;
      const float *xc = x + (r + halo) * p.dim + d;  // row of frame t
      if (level == 0) acc = fmaf(1.0f, xc[0], acc);
      else if (level == 1) {
#pragma unroll
        for (int j = -2; j <= 2; j++) {
          int tf = t + j; tf = tf < 0 ? 0 : (tf >= T ? T - 1 : tf);
          float s = kDelta1[j + 2];
          if (s != 0.0f) acc = fmaf(s, xc[(tf - t) * p.dim], acc);
        }
      } else {
#pragma unroll
        for (int j = -4; j <= 4; j++) {
          int tf = t + j; tf = tf < 0 ? 0 : (tf >= T ? T - 1 : tf);
          float s = kDelta2[j + 4];
          if (s != 0.0f) acc = fmaf(s, xc[(tf - t) * p.dim], acc);
        }
      }
      if (p.fmllr) y[r * od + c] = acc;
      else p.out[(f0 + t) * od + c] = acc;
    }
    if (!p.fmllr) return;
    // per-speaker fMLLR on the Δ rows: acc = 0, fmaf over ascending d, offset column last (the oracle's affine chain)
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * od; i += blockDim.x) {
      int r = i / od, o = i % od, t = t0 + r;
      if (t >= T) continue;
      const float *m = mat + o * (od + 1);
      float acc = 0.0f;
      for (int d = 0; d < od; d++) acc = fmaf(m[d], y[r * od + d], acc);
      acc += m[od];
      p.out[(f0 + t) * od + o] = acc;
    }
    return;
  }
  // mode 1: splice ±ctx → LDA (fmaf chain over the spliced vector, offset column last) → optional fMLLR
  const int nsp = 2 * p.ctx + 1, sdim = nsp * p.dim;
  const bool lda_offset = (p.lda_cols == sdim + 1);
  for (int i = threadIdx.x; i < kTile * p.lda_rows; i += blockDim.x) {
    int r = i / p.lda_rows, o = i % p.lda_rows, t = t0 + r;
    if (t >= T) continue;
    const float *m = mat + o * p.lda_cols;
    float acc = 0.0f;
    for (int j = 0; j < nsp; j++) {
      int tf = t + j - p.ctx; tf = tf < 0 ? 0 : (tf >= T ? T - 1 : tf);
      const float *xr = x + (tf - t0 + halo) * p.dim;
      for (int d = 0; d < p.dim; d++) acc = fmaf(m[j * p.dim + d], xr[d], acc);
    }
    if (lda_offset) acc += m[sdim];
    if (p.fmllr) y[r * p.lda_rows + o] = acc;
    else p.out[(f0 + t) * p.lda_rows + o] = acc;
  }
  if (!p.fmllr) return;
  __syncthreads();
  const float *fm = mat + p.lda_rows * p.lda_cols;
  for (int i = threadIdx.x; i < kTile * p.lda_rows; i += blockDim.x) {
    int r = i / p.lda_rows, o = i % p.lda_rows, t = t0 + r;
    if (t >= T) continue;
    const float *m = fm + o * (p.lda_rows + 1);
    float acc = 0.0f;
    for (int d = 0; d < p.lda_rows; d++) acc = fmaf(m[d], y[r * p.lda_rows + d], acc);
    acc += m[p.lda_rows];
    p.out[(f0 + t) * p.lda_rows + o] = acc;
  }
}

// splice ±ctx → LDA → optional fMLLR with the FRAME in registers and the matrices as wavefront-uniform operands.
// A lane owns a frame: it holds the frame's kSdim spliced, CMVN-offset inputs in VGPRs (read once from a coalesced LDS
// tile; the clamped halo rows make the spliced vector of frame r the contiguous floats X[r·dim .. r·dim + sdim)), runs the
// kR LDA chains over them, keeps the kR results in registers and runs the kR fMLLR chains over those.  The multipliers
// are the same for every lane.  Output rows go in pairs (o, o + 1) on the packed FMA — two IEEE fused multiply-adds, so
// every output keeps the fmaf chain of feats_kernel and the oracle, in the same order — which wants the two rows'
// multipliers next to each other: both matrices are regrouped as [group of 8 rows][column][8 rows].
//   LDA   (one per model, 14.7 KB): regrouped by feats_regroup_rows_kernel ahead of the launch, read with scalar loads
//         into SGPRs — it stays in the 16 KB scalar cache and costs no LDS read at all.
//   fMLLR (one per speaker, 6.5 KB): regrouped by the block into LDS and read with one address per wavefront, 16 bytes at
//         a time.  Through the scalar cache as well it pushed the LDA matrix out (every block brings another speaker's):
//         every scalar load then went to L2 and the kernel took 2.31 ms per 8 192-utterance step against 1.44 ms this way
//         (DESIGN §4).
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kTileRows = 256;  // frames per block of the frame-per-lane kernel: one per thread, 64 per wavefront
constexpr int kRowGroup = 8;    // output rows whose chains run together: four packed accumulators

// dst[(g·cols + d)·8 + j] = src[(8 g + j)·cols + d]: the columns of a group of eight rows, one after the other
__global__ __launch_bounds__(256) void feats_regroup_rows_kernel(const float *__restrict__ src, int rows, int cols, float *__restrict__ dst) {
  for (int i = threadIdx.x; i < rows * cols; i += blockDim.x) {
    const int j = i % kRowGroup, d = (i / kRowGroup) % cols, g = i / (kRowGroup * cols);
    dst[i] = src[(g * kRowGroup + j) * cols + d];
  }
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// a ← m · (x.lo, x.lo) + a, or with x.hi, on both halves: two IEEE fused multiply-adds.  m is a uniform pair of multipliers
// (rows o, o + 1 at one column) in SGPRs.  Written as the instruction because the compiler, given the vector form, builds
// every (x, x) pair in registers of its own, keeps them from one row group to the next and spills them.
template <bool kHi>
__device__ __forceinline__ void pk_fma_bcast(f32x2 &a, f32x2 m, f32x2 x) {
  if (kHi) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0]" : "+v"(a) : "s"(m), "v"(x));
  else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(a) : "s"(m), "v"(x));
}

template <bool kHi>                                  // the same with the multipliers in VGPRs
__device__ __forceinline__ void pk_fma_bcast_v(f32x2 &a, f32x2 m, f32x2 x) {
  if (kHi) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0]" : "+v"(a) : "v"(m), "v"(x));
  else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(a) : "v"(m), "v"(x));
}

// Four columns of a regrouped matrix: [column][8 rows], 32 floats, two 64-byte scalar loads.
struct RowSet { f32x16 lo, hi; };
__device__ __forceinline__ RowSet load_row_set(const float *__restrict__ s, int set) {
  const f32x16 *q = reinterpret_cast<const f32x16 *>(s + set * 4 * kRowGroup);
  return RowSet{q[0], q[1]};
}

// The eight chains of one row group over kN inputs, a[q] = rows (2q, 2q + 1): acc = 0, fma over ascending columns, then the
// offset column when there is one — feats_kernel's chain.  `s` is the group's [column][8 rows] block; `x` the inputs in
// pairs (x[c/2] holds inputs c, c + 1).  The multipliers arrive a set of four columns ahead: scalar loads return out of
// order, so the only wait there is waits for all of them, and the wait for a set is therefore written BEFORE the request
// for the next one — the next set's latency then lies under this set's packed FMAs (the compiler moves the set's first
// column across the wait; twelve of the sixteen FMAs remain).  The last set may reach up to three columns past the block:
// loaded, not used (the workspace is padded for it).
template <int kN>
__device__ __forceinline__ void row_group_chains(const float *__restrict__ s, bool offset, const f32x2 *x, f32x2 (&a)[4]) {
  constexpr int kSets = (kN + 1 + 3) / 4;
#pragma unroll
  for (int q = 0; q < 4; q++) a[q] = f32x2{0.0f, 0.0f};
  RowSet cur = load_row_set(s, 0);
#pragma unroll
  for (int i = 0; i < kSets; i++) {
    __builtin_amdgcn_s_waitcnt(0xc07f);              // lgkmcnt(0): `cur` is here
    RowSet nxt = cur;
    if (i + 1 < kSets) nxt = load_row_set(s, i + 1);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int col = 4 * i + c;
      const f32x16 v = c < 2 ? cur.lo : cur.hi;
      const int e = (c & 1) * kRowGroup;
      const f32x2 m[4] = {{v[e], v[e + 1]}, {v[e + 2], v[e + 3]}, {v[e + 4], v[e + 5]}, {v[e + 6], v[e + 7]}};
      if (col < kN) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (col & 1) pk_fma_bcast<true>(a[q], m[q], x[col / 2]);
          else pk_fma_bcast<false>(a[q], m[q], x[col / 2]);
        }
      } else if (col == kN) {
        if (offset)
#pragma unroll
          for (int q = 0; q < 4; q++) a[q] += m[q];
      }
    }
    cur = nxt;
  }
}

// The same chains with the group's block in LDS, read with one address for the whole wavefront, 16 bytes at a time.
template <int kN>
__device__ __forceinline__ void row_group_chains_lds(const float *s, const f32x2 *x, f32x2 (&a)[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++) a[q] = f32x2{0.0f, 0.0f};
#pragma unroll
  for (int col = 0; col <= kN; col++) {
    const float4 m01 = *reinterpret_cast<const float4 *>(s + col * kRowGroup);
    const float4 m23 = *reinterpret_cast<const float4 *>(s + col * kRowGroup + 4);
    const f32x2 m[4] = {{m01.x, m01.y}, {m01.z, m01.w}, {m23.x, m23.y}, {m23.z, m23.w}};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (col == kN) a[q] += m[q];
      else if (col & 1) pk_fma_bcast_v<true>(a[q], m[q], x[col / 2]);
      else pk_fma_bcast_v<false>(a[q], m[q], x[col / 2]);
    }
  }
}

template <int kDim, int kCtx, int kR>   // exact base dimension, splice context and output rows: the chains are fully unrolled
__global__ __launch_bounds__(kTileRows, 3) void feats_rows_kernel(FeatParams p, const float *__restrict__ lda_p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int kSdim = (2 * kCtx + 1) * kDim;
  constexpr int kGroups = kR / kRowGroup, kPairs = kRowGroup / 2;
  static_assert(kR % kRowGroup == 0 && kPairs == 4, "output rows run in groups of eight");
  const int utt = blockIdx.y;
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const int t0 = blockIdx.x * kTileRows;
  if (t0 >= T) return;
  constexpr int rows = kTileRows + 2 * kCtx;
  // X: [rows][kDim] CMVN-applied base features (frame t0-kCtx+r, clamped), then the kDim CMVN offsets.  Once every lane
  // holds its inputs the whole of LDS is the staging area of the outputs, [wavefront][64 frames][kR].
  // F: the speaker's fMLLR matrix, regrouped like the LDA matrix, behind the staging area.
  float *X = smem, *off = smem + rows * kDim, *F = smem + kTileRows * kR;
  const int spk = p.utt2spk ? p.utt2spk[utt] : 0;
  if (p.fmllr) {
    const float *fm = p.fmllr + (size_t)spk * kR * (kR + 1);
    for (int i = threadIdx.x; i < kR * (kR + 1); i += kTileRows) {
      const int j = i % kRowGroup, k = (i / kRowGroup) % (kR + 1), g = i / (kRowGroup * (kR + 1));
      F[i] = fm[(g * kRowGroup + j) * (kR + 1) + k];
    }
  }
  if (p.cmvn) {
    if (threadIdx.x < kDim) {
      const double *st = p.cmvn + (size_t)spk * 2 * (kDim + 1);
      off[threadIdx.x] = (float)(-(st[threadIdx.x] / st[kDim]));
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < rows * kDim; i += kTileRows) {
    int r = i / kDim, d = i % kDim;
    int t = t0 - kCtx + r;
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    float v = p.mfcc[(f0 + t) * kDim + d];
    if (p.cmvn) v += off[d];
    X[i] = v;
  }
  __syncthreads();
  f32x2 x[(kSdim + 1) / 2];                         // inputs in pairs: a packed FMA broadcasts either half
  {
    const float *xs = X + threadIdx.x * kDim;        // frames t-ctx .. t+ctx: rows r .. r+2·ctx of the tile (a frame past
#pragma unroll                                       // the utterance's end reads clamped rows and is not stored)
    for (int k = 0; k < kSdim; k++) x[k / 2][k & 1] = xs[k];
    if (kSdim & 1) x[kSdim / 2][1] = 0.0f;
  }
  __syncthreads();                                   // X is dead
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tw = t0 + 64 * wave;                     // the wavefront's first frame
  if (tw >= T) return;
  const bool lda_offset = (p.lda_cols == kSdim + 1);
  f32x2 y[kR / 2];
#pragma unroll
  for (int g = 0; g < kGroups; g++) {
    f32x2 a[kPairs];
    row_group_chains<kSdim>(lda_p + (size_t)g * p.lda_cols * kRowGroup, lda_offset, x, a);
#pragma unroll
    for (int q = 0; q < kPairs; q++) y[g * kPairs + q] = a[q];
  }
  f32x2 *S = reinterpret_cast<f32x2 *>(smem + wave * 64 * kR) + lane * (kR / 2);
  if (p.fmllr) {
#pragma unroll
    for (int g = 0; g < kGroups; g++) {
      f32x2 a[kPairs];
      row_group_chains_lds<kR>(F + g * (kR + 1) * kRowGroup, y, a);
#pragma unroll
      for (int q = 0; q < kPairs; q++) S[g * kPairs + q] = a[q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < kR / 2; q++) S[q] = y[q];
  }
  // the wavefront's frames are kR·64 contiguous floats of the output: written as 16-byte segments, lane after lane
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int nf = T - tw < 64 ? T - tw : 64;
  const float4 *src = reinterpret_cast<const float4 *>(smem + wave * 64 * kR);
  float4 *dst = reinterpret_cast<float4 *>(p.out + (f0 + tw) * kR);
  for (int i = lane; i < nf * (kR / 4); i += 64) dst[i] = src[i];
}

// __constant__ data lives once per device: every context uploads for its own device (mfa_ctx::delta_uploaded).
int upload_delta_scales(mfa_ctx *c) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  // Kaldi DeltaFeatures::DeltaFeatures, order 2, window 2, float arithmetic
  float s0[1] = {1.0f}, s1[5] = {0}, s2[9] = {0};
  {
    float normalizer = 0.0f;
    for (int j = -2; j <= 2; j++) { normalizer += j * j; s1[j + 2] += (float)j * s0[0]; }
    float sc = (float)(1.0 / normalizer);
    for (float &v : s1) v *= sc;
  }
  {
    float normalizer = 0.0f;
    for (int j = -2; j <= 2; j++) {
      normalizer += j * j;
      for (int k = -2; k <= 2; k++) s2[j + k + 4] += (float)j * s1[k + 2];
    }
    float sc = (float)(1.0 / normalizer);
    for (float &v : s2) v *= sc;
  }
  MFA_HIP_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(kDelta1), s1, sizeof(s1)));
  MFA_HIP_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(kDelta2), s2, sizeof(s2)));
  return 0;
}

}  // namespace

extern "C" {

MFA_API int mfa_cmvn_stats(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int32_t dim,
                           const int32_t *d_spk_utt_off, const int32_t *d_spk_utt, int32_t n_spk, double *d_stats) {
  if (dim > kMaxDim) return c->fail("CMVN: feature dim %d > %d", dim, kMaxDim);
  if (n_utt <= 0 || n_spk <= 0) return 0;
  size_t need = (size_t)n_utt * 2 * (dim + 1) * sizeof(double);
  if (c->d_ws.reserve(c, need, "the CMVN workspace")) return -1;
  KernelTimer kt(c, MFA_K_CMVN);
  hipLaunchKernelGGL(cmvn_utt_kernel, dim3(n_utt), dim3(256), 0, c->stream, d_feats, d_frame_off, dim, c->d_ws.ptr<double>());
  int total = n_spk * 2 * (dim + 1);
  hipLaunchKernelGGL(cmvn_spk_kernel, dim3((total + 255) / 256), dim3(256), 0, c->stream, c->d_ws.ptr<const double>(),
                     d_spk_utt_off, d_spk_utt, n_spk, dim, d_stats);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

MFA_API int mfa_feats_batch(mfa_ctx *c, const float *d_mfcc, const int64_t *d_frame_off, int32_t n_utt, int32_t max_frames,
                            int32_t dim, const int32_t *d_utt2spk, const double *d_cmvn, int32_t mode, int32_t splice_ctx,
                            const float *d_lda, int32_t lda_rows, int32_t lda_cols, const float *d_fmllr, float *d_out) {
  if (dim > kMaxDim) return c->fail("feats: base dim %d > %d", dim, kMaxDim);
  if (n_utt <= 0 || max_frames <= 0) return 0;
  if (n_utt > 65535) return c->fail("at most 65535 utterances per feature launch (got %d)", n_utt);
  if (mode != 0 && mode != 1) return c->fail("feats: bad mode %d", mode);
  if (d_cmvn && !d_utt2spk) return c->fail("feats: CMVN given without utt2spk");
  if (!c->delta_uploaded) { if (upload_delta_scales(c)) return -1; c->delta_uploaded = true; }
  FeatParams p;
  p.dim = dim; p.mode = mode; p.ctx = splice_ctx; p.lda_rows = lda_rows; p.lda_cols = lda_cols;
  p.mfcc = d_mfcc; p.frame_off = d_frame_off; p.utt2spk = d_utt2spk; p.cmvn = d_cmvn; p.lda = d_lda; p.fmllr = d_fmllr;
  p.out = d_out;
  // frame-per-lane kernel for MFA's standard shape (13 MFCCs spliced ±3 → 91, LDA to 40); other shapes take the generic kernel
  constexpr int kDim = 13, kCtx = 3, kR = 40;
  const char *generic = getenv("MFA_FEATS_GENERIC");
  const bool force_generic = generic && generic[0] == '1';
  const bool frame_lanes = mode == 1 && dim == kDim && splice_ctx == kCtx && lda_rows == kR && !force_generic;
  size_t lds = 0;
  if (mode == 0) {
    lds = (size_t)(kTile + 8) * dim * 4;
    if (d_fmllr) {
      const size_t od = 3 * (size_t)dim;
      lds += (od * (od + 1) + (size_t)kTile * od) * 4;
      if (lds > kMaxLdsBytes)
        return c->fail("feats: base dim %d with a %zux%zu fMLLR needs %zu bytes of LDS (a launch may ask for %zu)", dim, od,
                       od + 1, lds, kMaxLdsBytes);
    }
  } else {
    int sdim = (2 * splice_ctx + 1) * dim;
    if (!d_lda || lda_rows <= 0 || lda_rows > kMaxOut || (lda_cols != sdim && lda_cols != sdim + 1))
      return c->fail("feats: LDA %dx%d does not match spliced dim %d", lda_rows, lda_cols, sdim);
    lds = ((size_t)(kTile + 2 * splice_ctx) * dim + (size_t)lda_rows * lda_cols + (size_t)lda_rows * (lda_rows + 1) +
           (size_t)kTile * lda_rows) * 4;
    // kMaxDim × kMaxOut admit shapes whose tile does not fit a launch (16 dims, ±3, 64 rows: 66 KB)
    if (lds > kMaxLdsBytes && !frame_lanes)
      return c->fail("feats: base dim %d, splice ±%d, LDA %dx%d needs %zu bytes of LDS (a launch may ask for %zu)", dim,
                     splice_ctx, lda_rows, lda_cols, lds, kMaxLdsBytes);
  }
  dim3 grid((max_frames + kTile - 1) / kTile, n_utt);
  // the regrouped LDA matrix of the frame-per-lane kernel, padded for the last set of columns it asks for
  const size_t lda_p_floats = (size_t)kR * lda_cols + 3 * kRowGroup;
  if (frame_lanes && c->d_ws.reserve(c, lda_p_floats * sizeof(float), "the regrouped LDA matrix")) return -1;
  KernelTimer kt(c, MFA_K_FEATS);
  if (frame_lanes) {
    float *lda_p = c->d_ws.ptr<float>();
    hipLaunchKernelGGL(feats_regroup_rows_kernel, dim3(1), dim3(256), 0, c->stream, d_lda, kR, lda_cols, lda_p);
    const size_t lds_rows = ((size_t)kTileRows * kR + (size_t)kR * (kR + 1)) * sizeof(float);   // staging area + fMLLR matrix
    static_assert((kTileRows + 2 * kCtx) * kDim + kDim <= kTileRows * kR, "the input tile lies inside the staging area");
    dim3 grid2((max_frames + kTileRows - 1) / kTileRows, n_utt);
    hipLaunchKernelGGL((feats_rows_kernel<kDim, kCtx, kR>), grid2, dim3(kTileRows), lds_rows, c->stream, p, lda_p);
  } else {
    hipLaunchKernelGGL(feats_kernel, grid, dim3(256), lds, c->stream, p);
  }
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

}  // extern "C"
