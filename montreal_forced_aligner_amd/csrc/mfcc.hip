// Batched MFCC for gfx950: framing (edge reflection) → DC removal → pre-emphasis → Povey window → 512-point real FFT →
// power spectrum → mel bins → log → DCT-II → lifter.  Replaces kalpy MfccComputer.compute_mfccs (MFA/corpus/features.py:235;
// Kaldi feat/feature-mfcc.cc).
//
// Layout (round 2): a wavefront works on FOUR frames at a time — one 16-lane row per frame — and the 512-point real FFT
// is a 256-point complex FFT done as 16 × 16: lane i of a row holds the 16 packed samples z[i + 16 j] in registers, runs a
// 16-point DFT on them (two radix-4 levels, no memory traffic), applies the twiddle W256^(i·k1), the rows are transposed
// through a padded, conflict-free LDS tile (the only exchange of the whole transform), and a second in-register 16-point
// DFT leaves lane i with Z[i + 16 k2].  Round 1's kernel (one frame per wavefront, four radix-4 Stockham stages through
// LDS) spent as many LDS cycles as VALU cycles, 95 % of them on bank conflicts of its scattered 8-byte stores
// (SQ_LDS_BANK_CONFLICT ≈ SQ_ACTIVE_INST_LDS in the profile): 5.2 ms per 4.1 M frames; the butterflies now run on packed
// float2 arithmetic (v_pk_add/mul/fma_f32) out of registers.
// Row-local steps use the DPP crossbar: the sample before a lane's first one lives in the previous lane (row_shr:1), the
// frame sum is a row reduction, Z[256 − k] lives in lane 16 − i (row_mirror + row_shr:1).
// The mel filterbank reads the power spectrum back from LDS: every triangle is cut into pieces of at most `piece_taps`
// taps, piece p is summed by lane p mod 16 of each row, the pieces of a bin are then added in ascending order (fixed
// order: results are reproducible run to run); lane k of a row finishes cepstral coefficient k.
// Compiled with -ffp-contract=off: the only fused multiply-adds are the explicit ones.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ctx.hpp"

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kNfft = 512;
constexpr int kHalf = 256;
#ifndef MFA_MFCC_WAVES
#define MFA_MFCC_WAVES 8
#endif
constexpr int kWavesPerBlock = MFA_MFCC_WAVES;
constexpr int kFramesPerWave = 16;      // four passes of four frames
constexpr int kFramesPerBlock = kWavesPerBlock * kFramesPerWave;
constexpr int kMaxBins = 32;
constexpr int kMaxCeps = 16;            // one lane of a row per cepstral coefficient
constexpr int kMaxDct = 384;            // coefficients × bins
constexpr int kMaxPieces = 96;          // filterbank pieces (16 lanes × at most 6 rounds)
constexpr int kPieceTaps = 8;           // FFT bins per piece (short pieces are zero padded)
constexpr int kMaxMelW = kMaxPieces * kPieceTaps;
constexpr int kRowPad = 17;             // float2 row stride of the transposition tile: 34 dwords ≡ 2 (mod 32)
constexpr int kTileFloats = 4 * 16 * kRowPad * 2;   // one wavefront's LDS tile: 2 176 floats
// row strides of the reused tile are chosen so that the two rows of a 32-lane LDS group land on different banks
constexpr int kPStride = 273;           // power spectrum of one frame: 256 bins + room for a piece's zero-weight tail
constexpr int kPartStride = kMaxPieces + 8;
constexpr int kMelStride = kMaxBins + 8;
constexpr int kPartOff = 4 * kPStride;  // [4][kPartStride] piece sums
constexpr int kMelOff = kPartOff + 4 * kPartStride;   // [4][kMelStride] log mel energies
static_assert(kMelOff + 4 * kMelStride <= kTileFloats, "tile reuse");
// ---- the specialised tail (kFast): fixed trip counts over zero-padded tables, so that the reads of a stage are issued
// together and waited for once.  Plans within the bounds take it; anything else (a bin of more than kFastNp pieces) and
// MFA_MFCC_GENERIC=1 take the generic tail, which is the bit reference.
constexpr int kFastRounds = kMaxPieces / 16;   // mel rounds: every plan the tables hold
constexpr int kFastNp = 8;                     // pieces per bin (MFA's 23 bins need 7, 40 bins 4)
static_assert(kMaxPieces + kFastNp <= kPartStride + 1, "a bin's batch of piece sums stays inside its row");
static_assert(kMelOff % 4 == 0 && kMelStride % 4 == 0 && kTileFloats % 4 == 0, "16-byte reads of the log energies");
// a lane's entries of the window / twiddle tables and its DCT row are contiguous; 36 dwords from lane to lane put the sixteen
// lanes' 16-byte units on the 64 banks exactly once (36 l mod 64 = 0, 36, 8, 44, ...: sixteen distinct multiples of four)
constexpr int kLaneStride = 36;
// constant tables in LDS (float offsets).  generic: [e][lane] float2 tables, pieces [piece][tap], DCT [ceps][bins], plan
constexpr int kGenTw256 = 0, kGenTw512 = 512, kGenWnd = 1024, kGenMelw = 1536, kGenDct = kGenMelw + kMaxMelW,
              kGenInfo = kGenDct + kMaxDct, kGenConst = kGenInfo + kMaxPieces + kMaxBins;
// fast: [lane][e] float2 tables, pieces [round][half][lane][4 taps], DCT [ceps][kLaneStride] (the plan stays in registers)
constexpr int kFastTab = 16 * kLaneStride;
constexpr int kFastTw256 = 0, kFastTw512 = kFastTab, kFastWnd = 2 * kFastTab, kFastMelw = 3 * kFastTab,
              kFastDct = kFastMelw + kMaxMelW, kFastConst = kFastDct + kMaxCeps * kLaneStride;
static_assert(kMaxBins <= kLaneStride - 4 && kFastMelw % 4 == 0 && kFastDct % 4 == 0, "16-byte units");

struct MfccParams {
  int win, shift, nbins, nceps, snip_edges, remove_dc;
  int n_pieces, n_rounds, np_max;
  int raw_energy;           // use_energy (kEnergy instantiations): C0 is the frame's log energy, before (1) or after (0) pre-emphasis and window
  float log_energy_floor;   // log(energy_floor) or -inf
  float preemph;
  const float *window;      // [16][16][2]: window[2m], window[2m+1] for m = i + 16 j (0 beyond the window)
  const float *tw256;       // [16][16][2]: W256^(i·k1) at [k1][i]
  const float *tw512;       // [16][16][2]: −i · W512^(i + 16 k2) at [k2][i]
  const float *melw;        // [n_pieces][kPieceTaps] (zero padded)
  const int32_t *melinfo;   // [kMaxPieces] first FFT bin of the piece, then [kMaxBins] (first piece | pieces << 8) per bin
  const float *dct;         // [nceps][nbins]
  const float *lifter;      // [nceps]
};

// LDS operations of one wavefront execute in program order; the fences only stop the compiler from moving accesses
// across a hand-over between lanes.
#define WAVE_SYNC()                                              \
  do {                                                           \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       \
    __builtin_amdgcn_wave_barrier();                             \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");       \
  } while (0)

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// permutations that give every lane a source: no `old` value to keep (and no register copy to set one up)
template <int CTRL>
__device__ __forceinline__ float dpp_perm(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
// Σ over the 16 lanes of a row, returned in every lane of the row.  The addends are integer-valued and the total stays
// below 2^24, so the order of the additions does not matter.
__device__ __forceinline__ float row_sum_exact(float v) {
  v += dpp_f32<0xB1>(0.0f, v);          // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E>(0.0f, v);          // quad_perm [2,3,0,1]
  v += dpp_f32<0x141>(0.0f, v);         // row_half_mirror
  v += dpp_f32<0x140>(0.0f, v);         // row_mirror
  return v;
}

__device__ __forceinline__ v2f splat(float x) { return (v2f){x, x}; }
// a·b (complex): one packed multiply (operand halves picked by op_sel) and two fused multiply-adds
__device__ __forceinline__ v2f cmul(v2f a, v2f b) {
  const v2f t = splat(a.y) * (v2f){b.y, b.x};                       // (a.y b.y, a.y b.x)
  float re = fmaf(a.x, b.x, -t.x);
  const float im = fmaf(a.x, b.y, t.y);
  asm("" : "+v"(re));   // keeps the two apart: paired into one v_pk_fma the compiler first builds (−t.x, t.y) with three more instructions
  return (v2f){re, im};
}
// 4-point DFT in place (W4 = −i): a_k ← Σ_n a_n (−i)^(nk).  kZero3: a3 is known to be zero (samples beyond the window).
template <bool kZero3 = false>
__device__ __forceinline__ void dft4(v2f &a0, v2f &a1, v2f &a2, v2f &a3) {
  const v2f s02 = a0 + a2, d02 = a0 - a2;
  const v2f s13 = kZero3 ? a1 : a1 + a3, d13 = kZero3 ? a1 : a1 - a3;
  a0 = s02 + s13; a2 = s02 - s13;
  a1 = (v2f){d02.x + d13.y, d02.y - d13.x};                          // d02 − i·d13
  a3 = (v2f){d02.x - d13.y, d02.y + d13.x};                          // d02 + i·d13
}
// 16-point DFT of a[0..15] (W16 = e^(−2πi/16)); result in natural order.  kLive: a[kLive..15] are known to be zero.
template <int kLive = 16>
__device__ __forceinline__ void dft16(v2f (&a)[16]) {
  constexpr float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, h = 0.70710678118654752f;
  // n = na + 4 nb, k = kb + 4 ka:  Y[kb + 4 ka] = Σ_na W4^(na ka) · W16^(na kb) · Σ_nb a[na + 4 nb] W4^(nb kb)
#pragma unroll
  for (int na = 0; na < 4; na++) {                                                  // a[na + 4 kb] = inner sum
    if (na + 12 >= kLive && na + 8 < kLive) dft4<true>(a[na], a[na + 4], a[na + 8], a[na + 12]);
    else dft4<false>(a[na], a[na + 4], a[na + 8], a[na + 12]);
  }
  a[1 + 4] = cmul(a[1 + 4], (v2f){c1, -s1});    // W16^1
  a[1 + 8] = cmul(a[1 + 8], (v2f){h, -h});      // W16^2
  a[1 + 12] = cmul(a[1 + 12], (v2f){s1, -c1});  // W16^3
  a[2 + 4] = cmul(a[2 + 4], (v2f){h, -h});      // W16^2
  a[2 + 8] = (v2f){a[2 + 8].y, -a[2 + 8].x};    // W16^4 = −i
  a[2 + 12] = cmul(a[2 + 12], (v2f){-h, -h});   // W16^6
  a[3 + 4] = cmul(a[3 + 4], (v2f){s1, -c1});    // W16^3
  a[3 + 8] = cmul(a[3 + 8], (v2f){-h, -h});     // W16^6
  a[3 + 12] = cmul(a[3 + 12], (v2f){-c1, s1});  // W16^9
#pragma unroll
  for (int kb = 0; kb < 4; kb++) dft4(a[4 * kb], a[4 * kb + 1], a[4 * kb + 2], a[4 * kb + 3]);   // a[4 kb + ka] = Y[kb + 4 ka]
  // natural order: Y[kb + 4 ka] ← a[4 kb + ka] (a register renaming once the loops are unrolled)
#pragma unroll
  for (int kb = 0; kb < 4; kb++)
#pragma unroll
    for (int ka = kb + 1; ka < 4; ka++) { const v2f t = a[4 * kb + ka]; a[4 * kb + ka] = a[4 * ka + kb]; a[4 * ka + kb] = t; }
}

// kJ = ⌈window / 32⌉ packed sample pairs per lane (13 for MFA's 25 ms at 16 kHz).  kFast: the tail after the power spectrum
// with compile-time trip counts and the per-lane tables in [lane][entry] order (above); same arithmetic in the same order.
template <int kJ, bool kEnergy, bool kFast>
__global__ __launch_bounds__(64 * kWavesPerBlock, 4) void mfcc_kernel(MfccParams p, const int16_t *__restrict__ pcm,
                                                                        const int64_t *__restrict__ sample_off,
                                                                        const int64_t *__restrict__ frame_off,
                                                                        float *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_tile[kWavesPerBlock][kTileFloats];
  __shared__ __attribute__((aligned(16))) float s_const[kFast ? kFastConst : kGenConst];
  constexpr int kTw256 = kFast ? kFastTw256 : kGenTw256, kTw512 = kFast ? kFastTw512 : kGenTw512,
                kWnd = kFast ? kFastWnd : kGenWnd, kMelw = kFast ? kFastMelw : kGenMelw, kDct = kFast ? kFastDct : kGenDct;
  const int utt = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane >> 4, i = lane & 15;
  const int64_t s0 = sample_off[utt], n = sample_off[utt + 1] - s0;
  const int64_t f0 = frame_off[utt];
  const int T = (int)(frame_off[utt + 1] - f0);
  if ((int)blockIdx.x * kFramesPerBlock >= T) return;  // whole workgroup: nothing to do
  for (int k = threadIdx.x; k < 256; k += 64 * kWavesPerBlock) {
    const int at = kFast ? (k & 15) * kLaneStride + 2 * (k >> 4) : 2 * k;      // entry k >> 4 of lane k & 15
    s_const[kTw256 + at] = p.tw256[2 * k]; s_const[kTw256 + at + 1] = p.tw256[2 * k + 1];
    s_const[kTw512 + at] = p.tw512[2 * k]; s_const[kTw512 + at + 1] = p.tw512[2 * k + 1];
    s_const[kWnd + at] = p.window[2 * k]; s_const[kWnd + at + 1] = p.window[2 * k + 1];
  }
  if constexpr (kFast) {
    // taps 4 h … 4 h + 3 of piece 16 r + l at [r][h][l]: one 16-byte unit per lane, sixteen lanes contiguous; absent pieces,
    // bins and coefficients carry zero weights
    for (int k = threadIdx.x; k < kMaxMelW; k += 64 * kWavesPerBlock) {
      const int piece = k / kPieceTaps, t = k % kPieceTaps;
      s_const[kMelw + (((piece >> 4) * 2 + (t >> 2)) * 16 + (piece & 15)) * 4 + (t & 3)] = piece < p.n_pieces ? p.melw[k] : 0.0f;
    }
    for (int k = threadIdx.x; k < kMaxCeps * kLaneStride; k += 64 * kWavesPerBlock) {
      const int row = k / kLaneStride, b = k % kLaneStride;
      s_const[kDct + k] = row < p.nceps && b < p.nbins ? p.dct[row * p.nbins + b] : 0.0f;
    }
  } else {
    for (int k = threadIdx.x; k < p.n_pieces * kPieceTaps; k += 64 * kWavesPerBlock) s_const[kMelw + k] = p.melw[k];
    for (int k = threadIdx.x; k < p.nceps * p.nbins; k += 64 * kWavesPerBlock) s_const[kDct + k] = p.dct[k];
    for (int k = threadIdx.x; k < kMaxPieces + kMaxBins; k += 64 * kWavesPerBlock) s_const[kGenInfo + k] = __int_as_float(p.melinfo[k]);
  }
  float *tile = s_tile[wave];
  for (int k = lane; k < kTileFloats; k += 64) tile[k] = 0.0f;   // nothing non-finite may ever sit under a zero weight
  __syncthreads();
  const int fbase = blockIdx.x * kFramesPerBlock + wave * kFramesPerWave;
  const int nfr = min(kFramesPerWave, T - fbase);
  if (nfr <= 0) return;  // wavefronts are independent from here on
  const int16_t *x = pcm + s0;

  // ---- per-lane constants (the window / twiddle tables are read from LDS in every pass: 60 registers otherwise)
  // With 13 sample pairs per lane, what a lane takes from the small tables (its lifter, its part of the filterbank plan)
  // is loop-invariant and the compiler keeps it in registers.  With 16 there is no room beside the FFT (it was spilled
  // to scratch), so it is fetched again in every pass, through the lane index the compiler cannot see through.
  auto lane_lifter = [&](int l) { return l < p.nceps ? p.lifter[l] : 0.0f; };
  v2f *tq = (v2f *)tile + q * (16 * kRowPad);     // this row's transposition tile
  float *pq = tile + q * kPStride;                  // … power spectrum
  float *partq = tile + kPartOff + q * kPartStride;  // … filterbank piece sums
  float *melq = tile + kMelOff + q * kMelStride;     // … log mel energies
  // kFast: lane l's part of the plan: the first FFT bin of its piece in each of the six rounds, and the
  // (first piece | pieces << 8) words of its two bins (0 pieces beyond the last bin)
  auto lane_plan = [&](int l, int (&poff)[kFastRounds], int (&binfo)[2]) {
#pragma unroll
    for (int r = 0; r < kFastRounds; r++) poff[r] = p.melinfo[16 * r + l];
    binfo[0] = p.melinfo[kMaxPieces + l]; binfo[1] = p.melinfo[kMaxPieces + 16 + l];
  };
  constexpr bool kKeep = kJ <= 13;
  float lift_k = 0.0f;
  int poff[kFastRounds] = {}, binfo[2] = {};
  if constexpr (kKeep) {
    lift_k = lane_lifter(i);
    if constexpr (kFast) lane_plan(i, poff, binfo);
  }

  // samples of frame f as packed pairs (x[2m] | x[2m+1] << 16), m = i + 16 j
  auto load_frame = [&](int f, int li, unsigned (&raw)[kJ]) {
    const int64_t start = p.snip_edges ? (int64_t)f * p.shift : (int64_t)p.shift * f + p.shift / 2 - p.win / 2;
    const bool fast = start >= 0 && start + 32 * kJ <= n && (((s0 + start) & 1) == 0);
    if (__all(fast)) {          // interior frames (all but the first and last one or two): aligned 4-byte loads
      const unsigned *xs = reinterpret_cast<const unsigned *>(x + start);
#pragma unroll
      for (int j = 0; j < kJ; j++) raw[j] = xs[16 * j + li];
      return;
    }
    // edge frames, sample by sample.  A rolled loop (register j is picked by a uniform compare): unrolled, its 64-bit
    // address arithmetic was most of the kernel's code and held registers across the hot path
#pragma unroll 1
    for (int j = 0; j < kJ; j++) {
      unsigned both = 0;
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int s = 2 * (16 * j + i) + e;
        unsigned val = 0;
        if (s < p.win) {
          int64_t si = start + s;
          while (si < 0 || si >= n) si = (si < 0) ? (-si - 1) : (2 * n - 1 - si);  // reflection at the edges
          val = (unsigned short)x[si];
        }
        both |= val << (16 * e);
      }
#pragma unroll
      for (int jj = 0; jj < kJ; jj++) raw[jj] = jj == j ? both : raw[jj];
    }
  };
  // the frame a row works on (rows past the wavefront's share repeat its last frame and do not store)
  auto frame_of = [&](int it) { return fbase + min(4 * it + q, nfr - 1); };
  // entries first … kN − 1 of this lane in one of the three float2 tables; `at` is the lane's float offset in the table
  auto load_tab = [&](const float *tab, int at, int first, int kN, v2f (&w)[16]) {
    if constexpr (kFast) {
#pragma unroll
      for (int c = 0; c < 8; c++)
        if (2 * c < kN) {
          v4f t = *reinterpret_cast<const v4f *>(tab + at + 4 * c);
          asm("" : "+v"(t));   // one 16-byte read even where half of it is not used (entry 0 of W256)
          w[2 * c] = (v2f){t.x, t.y}; w[2 * c + 1] = (v2f){t.z, t.w};
        }
    } else {
#pragma unroll
      for (int e = 0; e < 16; e++)
        if (e >= first && e < kN) w[e] = *reinterpret_cast<const v2f *>(tab + at + 32 * e);
    }
  };

  unsigned nxt[kJ];
#pragma unroll
  for (int j = 0; j < kJ; j++) nxt[j] = 0;
  load_frame(frame_of(0), i, nxt);
  const int npass = (nfr + 3) >> 2;
  for (int it = 0; it < npass; it++) {
    const int f = frame_of(it);
    const bool live = 4 * it + q < nfr;
    int ti = i;
    asm volatile("" : "+v"(ti));   // table index the compiler cannot see through: the 60 table values are read per pass, not hoisted into registers
    const int tab_at = kFast ? ti * kLaneStride : 2 * ti;
    const int li = kKeep ? i : ti;     // lane index of this pass's addresses (PCM, tile, output): with 16 pairs they are not kept either
    v2f a[16];
#pragma unroll
    for (int j = 0; j < 16; j++) a[j] = (v2f){0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < kJ; j++) a[j] = (v2f){(float)(short)(nxt[j] & 0xFFFFu), (float)(short)(nxt[j] >> 16)};
    if (it + 1 < npass) load_frame(frame_of(it + 1), li, nxt);   // in flight while this pass is processed
    // ---- samples at and beyond the window's end are zero.  load_frame's fast path brings 32·kJ samples whatever the window:
    // at 385–416 (kJ 13) and 481–512 (kJ 16) samples only the last pair can lie beyond it, but a shorter window of the same
    // instantiation (257–383, 417–479) leaves real audio in whole registers before that one.  The window weights are 0
    // there, so the FFT never sees it — the DC sum and the raw energy would.  (Pairs below j = 8 lie inside every window
    // the 512-point FFT admits; the branch is uniform and not taken at 400 samples.)
    const bool ok_e = 2 * (16 * (kJ - 1) + i) < p.win, ok_o = 2 * (16 * (kJ - 1) + i) + 1 < p.win;
    auto clear_tail = [&]() {
      if (p.win < 32 * (kJ - 1)) {
#pragma unroll
        for (int j = 8; j < kJ - 1; j++) {
          if (2 * (16 * j + i) >= p.win) a[j].x = 0.0f;
          if (2 * (16 * j + i) + 1 >= p.win) a[j].y = 0.0f;
        }
      }
      if (!ok_e) a[kJ - 1].x = 0.0f;
      if (!ok_o) a[kJ - 1].y = 0.0f;
    };
    clear_tail();
    // ---- DC removal (int16-valued samples: the sum is an exact integer ≤ 2^24 in any order)
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < kJ; j++) sum += a[j].x + a[j].y;
    sum = row_sum_exact(sum);
    const float off = p.remove_dc ? (-sum / (float)p.win) : 0.0f;
#pragma unroll
    for (int j = 0; j < kJ; j++) a[j] += splat(off);
    clear_tail();
    // ---- use_energy: Kaldi's ProcessWindow takes the log energy here when raw_energy (default), after the window otherwise
    // (VecVec over the frame, floored at FLT_EPSILON; the sum's order is this kernel's, the result agrees to float rounding)
    float log_energy = 0.0f;
    auto frame_log_energy = [&]() {
      float e = 0.0f;
#pragma unroll
      for (int j = 0; j < kJ; j++) e = fmaf(a[j].y, a[j].y, fmaf(a[j].x, a[j].x, e));
      e = row_sum_exact(e);
      return __builtin_amdgcn_logf(fmaxf(e, 1.1920928955078125e-07f)) * 0.693147180559945309f;
    };
    if constexpr (kEnergy) { if (p.raw_energy) log_energy = frame_log_energy(); }
    // ---- pre-emphasis + window.  x[2m−1] is the odd sample of the previous lane (row_shr:1); lane 0 takes it from lane 15
    // of the previous register (row_ror:1 → kept where row_shr has no source); sample 0 uses itself (Kaldi)
    {
      v2f w[16];
      load_tab(s_const + kWnd, tab_at, 0, kJ, w);
      float prev_e[kJ];
#pragma unroll
      for (int j = 0; j < kJ; j++) {
        const float up = a[j > 0 ? j - 1 : 0].y;
        const float carry = j == 0 ? a[0].x : dpp_perm<0x121>(up);                            // row_ror:1
        prev_e[j] = dpp_f32<0x111>(carry, a[j].y);                                            // row_shr:1, lane 0 keeps `carry`
      }
#pragma unroll
      for (int j = 0; j < kJ; j++) {
        const v2f prev = (v2f){prev_e[j], a[j].x};
        a[j] = (a[j] - splat(p.preemph) * prev) * w[j];
      }
    }
    if constexpr (kEnergy) { if (!p.raw_energy) log_energy = frame_log_energy(); }
    // ---- 256-point complex FFT of z[m] = x[2m] + i x[2m+1]: 16-point DFTs over j, twiddle, transpose, 16-point DFTs over i
    dft16<kJ>(a);
    {
      v2f w[16];
      load_tab(s_const + kTw256, tab_at, 1, 16, w);
#pragma unroll
      for (int k1 = 1; k1 < 16; k1++) a[k1] = cmul(a[k1], w[k1]);
    }
#pragma unroll
    for (int k1 = 0; k1 < 16; k1++) tq[k1 * kRowPad + li] = a[k1];
    WAVE_SYNC();
#pragma unroll
    for (int n2 = 0; n2 < 16; n2++) a[n2] = tq[li * kRowPad + n2];
    WAVE_SYNC();
    dft16(a);                        // a[k2] = Z[i + 16 k2]
    // ---- real-FFT post-processing → power spectrum.  Z[256 − k] sits in lane 16 − i, register 15 − k2 (lane 0: its own
    // register 16 − k2): row_mirror brings lane 15 − i, row_shr:1 the lane before that one, and lane 0 keeps the `old` value.
    //   2E = Z[k] + conj(Z[N−k]),  2O = −i (Z[k] − conj(Z[N−k])),  2X[k] = 2E + w^k · 2O,  P = |2X|² / 4  (halving is exact)
    {
      v2f w[16];
      load_tab(s_const + kTw512, tab_at, 0, 16, w);
#pragma unroll
      for (int k2 = 0; k2 < 16; k2++) {
        const v2f zk = a[k2], own = a[(16 - k2) & 15], far = a[15 - k2];
        const float cx = dpp_f32<0x111>(own.x, dpp_perm<0x140>(far.x));
        const float cy = dpp_f32<0x111>(own.y, dpp_perm<0x140>(far.y));
        // 2E = (zk.x + cx, zk.y − cy), D = (zk.x − cx, zk.y + cy), 2O = −i·D: the table holds −i·w^k, so 2X = 2E + (−i w^k)·D
        float ex = zk.x + cx, ey = zk.y - cy, dx = zk.x - cx, dy = zk.y + cy;
        asm("" : "+v"(ex), "+v"(dx));   // (kept scalar: packed, the mixed signs cost three moves per pair)
        const v2f xk = (v2f){ex, ey} + cmul(w[k2], (v2f){dx, dy});
        float pw = 0.25f * fmaf(xk.y, xk.y, xk.x * xk.x);
        if (k2 == 0 && i == 0) pw = 0.25f * (xk.x * xk.x);      // Kaldi ComputePowerSpectrum: bin 0 = DC² (the Nyquist bin is never used)
        pq[16 * k2 + li] = pw;
      }
    }
    WAVE_SYNC();
    float c_out;
    if constexpr (kFast) {
      // ---- mel filterbank: piece (16 r + i) of the table is summed by lane i in round r; every round's 8 weights (two
      // 16-byte units) and 8 powers are independent reads, and the sums are written after the last round (a store between
      // two rounds would order the next round's reads behind it): the rounds wait for LDS together, not twice each
      if constexpr (!kKeep) lane_plan(ti, poff, binfo);
      const float *mw = s_const + kMelw + 4 * ti;
      float psum[kFastRounds];
#pragma unroll
      for (int r = 0; r < kFastRounds; r++) {
        const v4f wa = *reinterpret_cast<const v4f *>(mw + (2 * r) * 64), wb = *reinterpret_cast<const v4f *>(mw + (2 * r + 1) * 64);
        const float *pv = pq + poff[r];
        float acc = 0.0f;
        acc = fmaf(wa.x, pv[0], acc); acc = fmaf(wa.y, pv[1], acc); acc = fmaf(wa.z, pv[2], acc); acc = fmaf(wa.w, pv[3], acc);
        acc = fmaf(wb.x, pv[4], acc); acc = fmaf(wb.y, pv[5], acc); acc = fmaf(wb.z, pv[6], acc); acc = fmaf(wb.w, pv[7], acc);
        psum[r] = acc;
      }
#pragma unroll
      for (int r = 0; r < kFastRounds; r++) partq[16 * r + li] = psum[r];     // (an absent piece: +0 under zero weights, never taken below)
      WAVE_SYNC();
      // ---- pieces of a bin in ascending order as one batch of kFastNp reads, both bins of the lane together: an absent
      // piece adds +0.0, which changes no bit because a bin's sum of non-negative products is never −0.0; floor, log as in
      // the generic tail.  Bins beyond the last one are written as 0: the DCT below runs over kMaxBins under zero weights
      float v[2][kFastNp];
#pragma unroll
      for (int half = 0; half < 2; half++)
#pragma unroll
        for (int r = 0; r < kFastNp; r++) v[half][r] = partq[(binfo[half] & 0xFF) + r];
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int np = binfo[half] >> 8;
        float e = v[half][0];
#pragma unroll
        for (int r = 1; r < kFastNp; r++) e += r < np ? v[half][r] : 0.0f;
        const float le = __builtin_amdgcn_logf(fmaxf(e, 1.1920928955078125e-07f)) * 0.693147180559945309f;
        v[half][0] = np > 0 ? le : 0.0f;
      }
      melq[li] = v[0][0]; melq[li + 16] = v[1][0];
      WAVE_SYNC();
      // ---- DCT-II row i + lifter: the row (lane stride kLaneStride) and the row's log energies in 16-byte units
      const float *d = s_const + kDct + tab_at;
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < kMaxBins / 4; c++) {
        const v4f dw = *reinterpret_cast<const v4f *>(d + 4 * c), m = *reinterpret_cast<const v4f *>(melq + 4 * c);
        acc = fmaf(dw.x, m.x, acc); acc = fmaf(dw.y, m.y, acc); acc = fmaf(dw.z, m.z, acc); acc = fmaf(dw.w, m.w, acc);
      }
      c_out = acc * (kKeep ? lift_k : lane_lifter(ti));
    } else {
      // ---- mel filterbank: piece (16 r + i) of the table is summed by lane i in round r
      const float *s_melw = s_const + kMelw, *s_dct = s_const + kDct, *s_info = s_const + kGenInfo;
      for (int r = 0; r < p.n_rounds; r++) {
        const int piece = 16 * r + i;
        const int pc = min(piece, p.n_pieces - 1);
        const float *wv = s_melw + pc * kPieceTaps;
        const float *pv = pq + __float_as_int(s_info[pc]);
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < kPieceTaps; t++) acc = fmaf(wv[t], pv[t], acc);
        if (piece < p.n_pieces) partq[piece] = acc;
      }
      WAVE_SYNC();
      // ---- pieces of a bin in ascending order, floor at FLT_EPSILON, log (hardware log2: ≲1e-6 absolute on values of
      // 10–25, far inside the 2e-3 the FFT leaves); lane i finishes bins i and i + 16
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int b = i + 16 * half;
        if (b < p.nbins) {
          const int info = __float_as_int(s_info[kMaxPieces + b]);
          const int first = info & 0xFF, np = info >> 8;
          float e = partq[first];
          for (int r = 1; r < p.np_max; r++) if (r < np) e += partq[first + r];
          melq[b] = __builtin_amdgcn_logf(fmaxf(e, 1.1920928955078125e-07f)) * 0.693147180559945309f;
        }
      }
      WAVE_SYNC();
      // ---- DCT-II row i + lifter
      float acc = 0.0f;
      if (i < p.nceps) {
        const float *d = s_dct + i * p.nbins;
        for (int b = 0; b < p.nbins; b++) acc = fmaf(d[b], melq[b], acc);
      }
      c_out = acc * (kKeep ? lift_k : lane_lifter(ti));
    }
    if constexpr (kEnergy) { if (i == 0) c_out = fmaxf(log_energy, p.log_energy_floor); }   // C0 := log energy (MfccComputer::Compute)
    if (i < p.nceps && live) out[(f0 + f) * p.nceps + li] = c_out;
    WAVE_SYNC();
  }
}

float mel_scale(float f) { return 1127.0f * logf(1.0f + f / 700.0f); }

template <int kJ, bool kEnergy, bool kFast>
void mfcc_launch(mfa_ctx *c, dim3 grid, const MfccParams &p, const int16_t *d_pcm, const int64_t *d_sample_off,
                        const int64_t *d_frame_off, float *d_mfcc) {
  hipLaunchKernelGGL((mfcc_kernel<kJ, kEnergy, kFast>), grid, dim3(64 * kWavesPerBlock), 0, c->stream, p, d_pcm, d_sample_off,
                     d_frame_off, d_mfcc);
}

}  // namespace

extern "C" {

MFA_API int mfa_mfcc_configure(mfa_ctx *c, const mfa_mfcc_opts *o) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  int win = (int)(o->sample_frequency * 0.001f * o->frame_length_ms);
  int shift = (int)(o->sample_frequency * 0.001f * o->frame_shift_ms);
  int nfft = 1;
  while (nfft < win) nfft <<= 1;
  if (nfft != kNfft) return c->fail("MFCC kernel supports a 512-point FFT (window %d samples → %d)", win, nfft);
  if (o->num_mel_bins > kMaxBins || o->num_coefficients > kMaxCeps || o->num_coefficients > o->num_mel_bins ||
      o->num_mel_bins * o->num_coefficients > kMaxDct)
    return c->fail("unsupported num_mel_bins/num_coefficients %d/%d", o->num_mel_bins, o->num_coefficients);
  int nb = o->num_mel_bins, nc = o->num_coefficients;
  // window ("povey"), Kaldi FeatureWindowFunction
  std::vector<float> window(win);
  double a = 2.0 * M_PI / (win - 1);
  for (int i = 0; i < win; i++) window[i] = (float)pow(0.5 - 0.5 * cos(a * (double)i), 0.85);
  // lane tables: window pairs at [j][i] for m = i + 16 j; W256^(i·k1) at [k1][i]; W512^(i + 16 k2) at [k2][i]
  std::vector<float> wpairs(16 * 16 * 2, 0.0f);
  for (int j = 0; j < 16; j++)
    for (int i = 0; i < 16; i++)
      for (int e = 0; e < 2; e++) {
        const int sidx = 2 * (16 * j + i) + e;
        wpairs[2 * (16 * j + i) + e] = sidx < win ? window[sidx] : 0.0f;
      }
  std::vector<float> tw(2 * 256 * 2);
  for (int k = 0; k < 16; k++)
    for (int i = 0; i < 16; i++) {
      const double a256 = 2.0 * M_PI * (double)(i * k) / 256.0, a512 = 2.0 * M_PI * (double)(i + 16 * k) / 512.0;
      tw[2 * (16 * k + i)] = (float)cos(a256);
      tw[2 * (16 * k + i) + 1] = (float)(-sin(a256));
      // −i · W512^k = (Im w, −Re w) with w = (cos, −sin): the real-FFT step multiplies D = Z[k] − conj(Z[N−k]) by it
      tw[512 + 2 * (16 * k + i)] = (float)(-sin(a512));
      tw[512 + 2 * (16 * k + i) + 1] = (float)(-cos(a512));
    }
  // Kaldi MelBanks (float arithmetic as in mel-computations.cc)
  float nyquist = 0.5f * o->sample_frequency;
  float low = o->low_frequency, high = o->high_frequency > 0.0f ? o->high_frequency : nyquist + o->high_frequency;
  if (low < 0.0f || low >= nyquist || high <= 0.0f || high > nyquist || high <= low)
    return c->fail("bad mel frequency range [%f, %f]", low, high);
  float fft_bin_width = o->sample_frequency / nfft;
  float mel_low = mel_scale(low), mel_high = mel_scale(high);
  float mel_delta = (mel_high - mel_low) / (nb + 1);
  std::vector<float> melw;
  std::vector<int32_t> first_of(nb), len_of(nb), woff_of(nb);
  for (int bin = 0; bin < nb; bin++) {
    float left = mel_low + bin * mel_delta, center = mel_low + (bin + 1) * mel_delta, right = mel_low + (bin + 2) * mel_delta;
    int first = -1, last = -1;
    std::vector<float> w(nfft / 2, 0.0f);
    for (int i = 0; i < nfft / 2; i++) {
      float mel = mel_scale(fft_bin_width * i);
      if (mel > left && mel < right) {
        w[i] = (mel <= center) ? (mel - left) / (center - left) : (right - mel) / (right - center);
        if (first == -1) first = i;
        last = i;
      }
    }
    if (first == -1) return c->fail("mel bin %d is empty (num_mel_bins too large)", bin);
    first_of[bin] = first;
    len_of[bin] = last + 1 - first;
    woff_of[bin] = (int32_t)melw.size();
    melw.insert(melw.end(), w.begin() + first, w.begin() + last + 1);
  }
  // Filterbank plan: every triangle is cut into pieces of kPieceTaps consecutive FFT bins (the last one zero padded);
  // piece p is summed by lane p mod 16 of a row in round p / 16, the pieces of a bin are then added in ascending order.
  const int best_taps = kPieceTaps;
  {
    int np = 0;
    for (int b = 0; b < nb; b++) np += (len_of[b] + best_taps - 1) / best_taps;
    if (np > kMaxPieces) return c->fail("mel filterbank needs %d pieces of %d bins (kernel table holds %d)", np, best_taps, kMaxPieces);
  }
  std::vector<float> piecew;
  std::vector<int32_t> melinfo(kMaxPieces + kMaxBins, 0);
  int n_pieces = 0, np_max = 1;
  for (int b = 0; b < nb; b++) {
    const int k = (len_of[b] + best_taps - 1) / best_taps;
    melinfo[kMaxPieces + b] = n_pieces | (k << 8);
    np_max = std::max(np_max, k);
    for (int q = 0; q < k; q++, n_pieces++) {
      melinfo[n_pieces] = first_of[b] + q * best_taps;
      for (int t = 0; t < best_taps; t++) {
        const int at = q * best_taps + t;
        piecew.push_back(at < len_of[b] ? melw[woff_of[b] + at] : 0.0f);
      }
    }
  }
  std::vector<float> dct((size_t)nc * nb), lifter(nc);
  float norm0 = std::sqrt(1.0f / (float)nb), norm = std::sqrt(2.0f / (float)nb);
  for (int k = 0; k < nc; k++)
    for (int n = 0; n < nb; n++)
      dct[(size_t)k * nb + n] = (k == 0) ? norm0 : (float)(norm * std::cos((double)M_PI / nb * (n + 0.5) * k));
  for (int i = 0; i < nc; i++)
    lifter[i] = o->cepstral_lifter != 0.0f ? (float)(1.0 + 0.5 * o->cepstral_lifter * sin(M_PI * i / o->cepstral_lifter)) : 1.0f;

  // a refused option set or a failed upload leaves the previous options and tables in force
  return dev_upload_commit<MfaHipDev>(
      c, "the MFCC tables",
      {{&c->d_window, wpairs.data(), wpairs.size() * 4}, {&c->d_twiddle, tw.data(), tw.size() * 4},
       {&c->d_melw, piecew.data(), piecew.size() * 4}, {&c->d_melidx, melinfo.data(), melinfo.size() * 4},
       {&c->d_dct, dct.data(), dct.size() * 4}, {&c->d_lifter, lifter.data(), lifter.size() * 4}},
      [&] {
        c->n_melw = n_pieces; c->mel_np_max = np_max;
        c->mfcc = *o;
        c->win = win; c->shift = shift; c->nfft = nfft;
        c->mfcc_ready = true;
      });
}

MFA_API int32_t mfa_mfcc_num_frames(mfa_ctx *c, int64_t n) {
  if (!c->mfcc_ready) return -1;
  if (c->mfcc.snip_edges) return n < c->win ? 0 : (int32_t)(1 + (n - c->win) / c->shift);
  return (int32_t)((n + c->shift / 2) / c->shift);
}

// Which tail the next mfa_mfcc_batch launches: 1 the specialised one, 2 the generic one (a plan beyond its bounds, or
// MFA_MFCC_GENERIC=1, read at every call), 0 before mfa_mfcc_configure.
MFA_API int mfa_mfcc_path(mfa_ctx *c) {
  if (!c->mfcc_ready) return 0;
  const char *generic = getenv("MFA_MFCC_GENERIC");
  const bool force_generic = generic && generic[0] == '1';
  return !force_generic && c->mel_np_max <= kFastNp ? 1 : 2;
}

MFA_API int mfa_mfcc_batch(mfa_ctx *c, const int16_t *d_pcm, const int64_t *d_sample_off, const int64_t *d_frame_off,
                           int32_t n_utt, int32_t max_frames, float *d_mfcc) {
  if (!c->mfcc_ready) return c->fail("mfa_mfcc_configure has not been called");
  if (n_utt <= 0 || max_frames <= 0) return 0;
  if (n_utt > 65535) return c->fail("at most 65535 utterances per MFCC launch (got %d)", n_utt);
  MfccParams p;
  p.win = c->win; p.shift = c->shift; p.nbins = c->mfcc.num_mel_bins; p.nceps = c->mfcc.num_coefficients;
  p.snip_edges = c->mfcc.snip_edges; p.remove_dc = c->mfcc.remove_dc_offset; p.preemph = c->mfcc.preemphasis;
  p.raw_energy = c->mfcc.raw_energy;
  p.log_energy_floor = c->mfcc.energy_floor > 0.0f ? logf(c->mfcc.energy_floor) : -INFINITY;
  p.window = c->d_window.ptr<float>(); p.tw256 = c->d_twiddle.ptr<float>(); p.tw512 = p.tw256 + 512;
  p.melw = c->d_melw.ptr<float>(); p.melinfo = c->d_melidx.ptr<int32_t>(); p.dct = c->d_dct.ptr<float>(); p.lifter = c->d_lifter.ptr<float>();
  p.n_pieces = c->n_melw; p.n_rounds = (c->n_melw + 15) / 16; p.np_max = c->mel_np_max;
  dim3 grid((max_frames + kFramesPerBlock - 1) / kFramesPerBlock, n_utt);
  KernelTimer kt(c, MFA_K_MFCC);
  // instantiations: 13 or 16 sample pairs per lane; with use_energy (the default kernel carries nothing for it); tail
  const int which = (c->win <= 32 * 13 ? 0 : 4) + (c->mfcc.use_energy != 0 ? 2 : 0) + (mfa_mfcc_path(c) == 1 ? 1 : 0);
  switch (which) {
    case 0: mfcc_launch<13, false, false>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    case 1: mfcc_launch<13, false, true>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    case 2: mfcc_launch<13, true, false>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    case 3: mfcc_launch<13, true, true>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    case 4: mfcc_launch<16, false, false>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    case 5: mfcc_launch<16, false, true>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    case 6: mfcc_launch<16, true, false>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
    default: mfcc_launch<16, true, true>(c, grid, p, d_pcm, d_sample_off, d_frame_off, d_mfcc); break;
  }
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

}  // extern "C"
