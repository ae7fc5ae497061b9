// Kaldi's CompressedMatrix codec, method kOneByteWithColHeaders ("CM"), for gfx950: the tables the reference's corpus path
// stores its features in (MFA/corpus/features.py:235, :356-365; Kaldi matrix/compressed-matrix.cc).  kaldi_io's
// write_compressed_matrix / _read_compressed are the specification, operation for operation; the arithmetic lives in
// compress_math.hpp, host and device, every float32 sum, product and quotient an _rn intrinsic, and the file is compiled
// with -ffp-contract=off (the *63 of the last piece is inexact: a fused multiply-add there changes bytes).
//
// One kernel, one workgroup of four wavefronts per (utterance, table).
//   staging  a table of at most kResidentFloats values is copied into LDS first: the whole workgroup reads along the rows
//            (independent, coalesced loads) and writes column-major.  A longer table stays in global memory and every
//            pass below reads its columns from there.
//   phase 1  a wavefront owns a column at a time (columns w, w + 4, …), lanes over its rows: take the speaker's mean off
//            (the second trip), reduce the smallest and largest key, and find the two inner order statistics by an exact
//            radix select — four passes over the order-preserving uint32 image of the floats, 8 bits each, most
//            significant first, both ranks in one sweep (a 256-bin LDS histogram per rank and wavefront, then a wavefront
//            scan that names the bin holding the rank).  The select never moves data, costs the same for every length and
//            input order, and needs no second algorithm for long tables.  The four statistics of every column go to the
//            context's scratch.
//   phase 2  the table's min / range from the column extremes, then per column: the header codes (double, as the writer's
//            to_u16), the writer's and the reader's percentile floats (their increments differ, see below), and per value
//            the byte and the float the reader gives back for it.  The floats of a resident table replace its values in
//            LDS and leave as the table came in, written along the rows by the whole workgroup.
// Which of several equal elements a rank names does not matter, only its value; −0.0 sorts below +0.0 here, and both give
// the same code (a table whose minimum is a zero of both signs may get either sign in its header: numpy's min has no rule
// for that either).  Indices never come from data: a digit is 8 bits of a key, a byte goes through codec_q8().  Non-finite
// input has no defined result (the host codec has none) but walks the same bounded loops.
//
// The asymmetry the reader and writer have, kept:
//   writer  inc = f32(range · f32(1/65535)),            f = min + inc · f32(code)      all float32
//   reader  inc = f32(double(range) · double(1/65535)), p = min + inc · f32(code)      one double product, rounded once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#include "compress_math.hpp"
#include "ctx.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaveLanes = 64;
constexpr int kWaves = kThreads / kWaveLanes;
constexpr int kResidentFloats = 13 * 1024;   // a table of at most this many values is staged in LDS (52 KB: 1024 rows × 13)

struct CompressParams {
  const float *feats; const int64_t *frame_off; int stride, c0, ncols;
  const double *cmvn; const int32_t *utt2spk; int cmvn_dim;
  float *out; float *global; uint16_t *colhdr; uint8_t *bytes;
  float *stats;   // scratch [n_utt][ncols][4]: sorted[0], sorted[rank a], sorted[rank b], sorted[rows-1] of every column
};

// order-preserving image of a float32: a < b as floats ⇒ key(a) < key(b) as unsigned (−0.0 just below +0.0)
__device__ inline uint32_t f2key(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float key2f(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__global__ __launch_bounds__(kThreads) void compress_kernel(CompressParams p) {
  __shared__ float tab[kResidentFloats];           // resident tables: column-major [ncols][rows]
  __shared__ __attribute__((aligned(16))) uint32_t hist[kWaves][2][256];
  __shared__ uint32_t wmin[kWaves], wmax[kWaves];
  const int utt = blockIdx.x;
  const int64_t f0 = p.frame_off[utt], n = p.frame_off[utt + 1] - f0;
  if (n <= 0) return;                              // no rows: no table (the whole workgroup leaves)
  const int rows = (int)(n < (int64_t)INT_MAX ? n : (int64_t)INT_MAX);
  const int ncols = p.ncols;
  const bool resident = (int64_t)rows * ncols <= kResidentFloats;
  const int wave = threadIdx.x / kWaveLanes, lane = threadIdx.x % kWaveLanes;
  const int q = rows / 4;
  const uint32_t rank_a = rows >= 5 ? q : (rows > 1 ? 1 : 0);          // small matrices: sorted[1], sorted[2] where they exist
  const uint32_t rank_b = rows >= 5 ? 3 * q : (rows > 2 ? 2 : rows - 1);
  const float *src = p.feats + f0 * p.stride + p.c0;
  const double *st_cmvn = p.cmvn ? p.cmvn + (size_t)p.utt2spk[utt] * 2 * (p.cmvn_dim + 1) : nullptr;
  float *st = p.stats + (size_t)utt * ncols * 4;
  const int rounds = (ncols + kWaves - 1) / kWaves;
  uint32_t *h = &hist[wave][0][0];

  // ---- a resident table is read once, by the whole workgroup and along its rows (independent, coalesced loads: the
  // column loops below would wait for one strided load after the other), and transposed into LDS
  if (resident) {
    const int total = rows * ncols;
#pragma unroll 4
    for (int i = threadIdx.x; i < total; i += kThreads) {
      const int r = i / ncols, c = i - r * ncols;
      tab[c * rows + r] = src[(int64_t)r * p.stride + c];
    }
    __syncthreads();
  }

  // ---- phase 1: column statistics
  uint32_t tmin = 0xFFFFFFFFu, tmax = 0u;
  for (int round = 0; round < rounds; round++) {
    const int c = round * kWaves + wave;
    const bool active = c < ncols;                 // wavefront-uniform; an idle wavefront still meets every barrier
    // ApplyCmvn without variance normalisation: the mean is a double quotient rounded once, the subtraction float32
    const float mean = active && st_cmvn ? (float)(st_cmvn[p.c0 + c] / st_cmvn[p.cmvn_dim]) : 0.0f;
    float *col = tab + (resident && active ? c * rows : 0);
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    if (active)
#pragma unroll 4
      for (int r = lane; r < rows; r += kWaveLanes) {
        float x = resident ? col[r] : src[(int64_t)r * p.stride + c];
        if (st_cmvn) {
          x = __fsub_rn(x, mean);
          if (resident) col[r] = x;                  // (the later passes read the column as it will be compressed)
        }
        const uint32_t k = f2key(x);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t a = __shfl_xor(kmin, o), b = __shfl_xor(kmax, o);
      kmin = a < kmin ? a : kmin;
      kmax = b > kmax ? b : kmax;
    }
    uint32_t pref[2] = {0u, 0u}, want[2] = {rank_a, rank_b};
    for (int pass = 0; pass < 4; pass++) {
      const int shift = 24 - 8 * pass;
      for (int i = lane; i < 2 * 256; i += kWaveLanes) h[i] = 0u;
      __syncthreads();
      if (active)
#pragma unroll 4
        for (int r = lane; r < rows; r += kWaveLanes) {
          float x;
          if (resident) x = col[r];
          else { x = src[(int64_t)r * p.stride + c]; if (st_cmvn) x = __fsub_rn(x, mean); }
          const uint32_t k = f2key(x);
          const uint32_t d = (k >> shift) & 255u;
          const uint32_t hi = pass == 0 ? 0u : k >> (shift + 8);       // the digits already fixed
          if (hi == pref[0]) atomicAdd(&h[d], 1u);
          if (hi == pref[1]) atomicAdd(&h[256 + d], 1u);
        }
      __syncthreads();
      // lane l holds bins 4l … 4l+3 of both histograms; an inclusive scan over the lanes (the two ranks side by side: two
      // independent chains of shuffles) names the lane, then the bin, that holds the rank
      uint32_t b[2][4], s[2] = {0u, 0u}, incl[2];
      for (int w = 0; w < 2; w++)
        for (int j = 0; j < 4; j++) { b[w][j] = h[w * 256 + lane * 4 + j]; s[w] += b[w][j]; }
      incl[0] = s[0]; incl[1] = s[1];
      for (int o = 1; o < kWaveLanes; o <<= 1) {
        const uint32_t up0 = __shfl_up(incl[0], o), up1 = __shfl_up(incl[1], o);
        if (lane >= o) { incl[0] += up0; incl[1] += up1; }
      }
      for (int w = 0; w < 2; w++) {
        uint32_t rem = want[w] - (incl[w] - s[w]);
        const bool mine = incl[w] - s[w] <= want[w] && want[w] < incl[w];
        uint32_t digit = lane * 4;
        if (mine) {
          for (int j = 0; j < 3 && rem >= b[w][j]; j++) { rem -= b[w][j]; digit = lane * 4 + j + 1; }
        }
        const unsigned long long who = __ballot(mine);
        const int from = who ? __ffsll((long long)who) - 1 : 0;        // (no lane: an idle wavefront; its result is not used)
        digit = __shfl(digit, from) & 255u;
        rem = __shfl(rem, from);
        pref[w] = (pref[w] << 8) | digit;
        want[w] = who ? rem : 0u;
      }
      __syncthreads();                              // every lane has read the histogram before the next pass clears it
    }
    if (active) {
      if (lane == 0) {
        st[c * 4 + 0] = key2f(kmin);
        st[c * 4 + 1] = key2f(pref[0]);
        st[c * 4 + 2] = key2f(pref[1]);
        st[c * 4 + 3] = key2f(kmax);
      }
      tmin = kmin < tmin ? kmin : tmin;
      tmax = kmax > tmax ? kmax : tmax;
    }
  }
  if (lane == 0) { wmin[wave] = tmin; wmax[wave] = tmax; }
  __syncthreads();                                  // also: this workgroup's stats are visible to all of it

  // ---- global header (ComputeGlobalHeader)
  for (int w = 0; w < kWaves; w++) {
    tmin = wmin[w] < tmin ? wmin[w] : tmin;
    tmax = wmax[w] > tmax ? wmax[w] : tmax;
  }
  const float mn = key2f(tmin);
  float rng;
  codec_global(mn, key2f(tmax), &rng);
  if (threadIdx.x == 0 && p.global) { p.global[(size_t)utt * 2 + 0] = mn; p.global[(size_t)utt * 2 + 1] = rng; }

  // ---- phase 2: column headers, bytes, and what the reader makes of them
  for (int round = 0; round < rounds; round++) {
    const int c = round * kWaves + wave;
    if (c >= ncols) break;
    const float mean = st_cmvn ? (float)(st_cmvn[p.c0 + c] / st_cmvn[p.cmvn_dim]) : 0.0f;
    const float s[4] = {st[c * 4 + 0], st[c * 4 + 1], st[c * 4 + 2], st[c * 4 + 3]};
    const CodecColumn hd = codec_column(s, rows, mn, rng);
    if (lane < 4 && p.colhdr)
      p.colhdr[((size_t)utt * ncols + c) * 4 + lane] = (uint16_t)(lane == 0 ? hd.code[0] : lane == 1 ? hd.code[1] : lane == 2 ? hd.code[2] : hd.code[3]);
    float *col = tab + (resident ? c * rows : 0);
    uint8_t *bdst = p.bytes ? p.bytes + f0 * ncols + (int64_t)c * rows : nullptr;
    float *odst = p.out ? p.out + f0 * p.stride + p.c0 + c : nullptr;
#pragma unroll 4
    for (int r = lane; r < rows; r += kWaveLanes) {
      float x;
      if (resident) x = col[r];
      else { x = src[(int64_t)r * p.stride + c]; if (st_cmvn) x = __fsub_rn(x, mean); }
      const int b = codec_byte(hd, x);
      if (bdst) bdst[r] = (uint8_t)b;
      if (odst) {
        const float y = codec_value(hd, b);
        if (resident) col[r] = y;                    // leaves along the rows below
        else odst[(int64_t)r * p.stride] = y;
      }
    }
  }
  // a resident table's values go out as they came in: the whole workgroup writes along the rows (a wavefront's column
  // is one 4-byte store per row, a row apart)
  if (resident && p.out) {
    __syncthreads();
    float *dst = p.out + f0 * p.stride + p.c0;
    const int total = rows * ncols;
#pragma unroll 4
    for (int i = threadIdx.x; i < total; i += kThreads) {
      const int r = i / ncols, c = i - r * ncols;
      dst[(int64_t)r * p.stride + c] = tab[c * rows + r];
    }
  }
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_compress_resident_values(void) { return kResidentFloats; }

MFA_API int mfa_compress_batch(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int32_t stride,
                               int32_t c0, int32_t c1, const double *d_cmvn, const int32_t *d_utt2spk, int32_t cmvn_dim,
                               float *d_out, float *d_global, uint16_t *d_colhdr, uint8_t *d_bytes) {
  if (stride <= 0 || c0 < 0 || c1 <= c0 || c1 > stride)
    return c->fail("compress: columns [%d, %d) do not lie inside a row of %d", c0, c1, stride);
  if (d_out && d_out == d_feats)
    return c->fail("compress: the output may not be the input (the once-compressed matrix is kept for the second trip)");
  if ((d_cmvn != nullptr) != (d_utt2spk != nullptr)) return c->fail("compress: CMVN statistics and utt2spk come together");
  if (d_cmvn && cmvn_dim < c1)
    return c->fail("compress: CMVN statistics of %d columns do not cover columns [%d, %d)", cmvn_dim, c0, c1);
  if (n_utt <= 0) return 0;
  if (!d_feats || !d_frame_off) return c->fail("compress: no input");
  const int ncols = c1 - c0;
  if (c->d_ws.reserve(c, (size_t)n_utt * ncols * 4 * sizeof(float), "the codec's column statistics")) return -1;
  CompressParams p;
  p.feats = d_feats; p.frame_off = d_frame_off; p.stride = stride; p.c0 = c0; p.ncols = ncols;
  p.cmvn = d_cmvn; p.utt2spk = d_utt2spk; p.cmvn_dim = cmvn_dim;
  p.out = d_out; p.global = d_global; p.colhdr = d_colhdr; p.bytes = d_bytes;
  p.stats = c->d_ws.ptr<float>();
  KernelTimer kt(c, MFA_K_COMPRESS);
  hipLaunchKernelGGL(compress_kernel, dim3(n_utt), dim3(kThreads), 0, c->stream, p);   // (grid.x: no 65 535 limit)
  MFA_DEBUG_POINT(c, "compress_kernel n_utt %d cols [%d, %d)", n_utt, c0, c1);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

// The same arithmetic on the host for one table (tests): order statistics by a sort of the keys.
MFA_API int mfa_debug_compress_host(const float *h_table, int32_t rows, int32_t cols, float *h_global, uint16_t *h_colhdr,
                                    uint8_t *h_bytes, float *h_out) {
  if (!h_table || rows <= 0 || cols <= 0) return -1;
  float mn = h_table[0], mx = h_table[0], rng;
  for (int64_t i = 0; i < (int64_t)rows * cols; i++) { mn = h_table[i] < mn ? h_table[i] : mn; mx = h_table[i] > mx ? h_table[i] : mx; }
  codec_global(mn, mx, &rng);
  if (h_global) { h_global[0] = mn; h_global[1] = rng; }
  std::vector<float> sd(rows);
  const int q = rows / 4;
  const int a = rows >= 5 ? q : (rows > 1 ? 1 : 0), b = rows >= 5 ? 3 * q : (rows > 2 ? 2 : rows - 1);
  for (int c = 0; c < cols; c++) {
    for (int r = 0; r < rows; r++) sd[r] = h_table[(int64_t)r * cols + c];
    std::sort(sd.begin(), sd.end());
    const float s[4] = {sd[0], sd[a], sd[b], sd[rows - 1]};
    const CodecColumn hd = codec_column(s, rows, mn, rng);
    for (int k = 0; k < 4 && h_colhdr; k++) h_colhdr[c * 4 + k] = (uint16_t)hd.code[k];
    for (int r = 0; r < rows; r++) {
      const int v = codec_byte(hd, h_table[(int64_t)r * cols + c]);
      if (h_bytes) h_bytes[(int64_t)c * rows + r] = (uint8_t)v;
      if (h_out) h_out[(int64_t)r * cols + c] = codec_value(hd, v);
    }
  }
  return 0;
}

}  // extern "C"
