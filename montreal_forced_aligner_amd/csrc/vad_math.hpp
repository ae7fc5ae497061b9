// The arithmetic of the speech-activity stage (vad.hip), host and device: the contract of include/mfa_hip.h ("Speech
// activity") operation for operation.  The kernels and the host twins of vad_host.cpp both run exactly these functions:
// the integer parts have the same bits on either side by nature, the float64 sums because their order is fixed here, and
// the translation units are compiled with -ffp-contract=off (a fused multiply-add in a running sum of squares would change
// bits).  float64 +, −, ·, / and sqrt are correctly rounded on both sides.  Plain C++: no HIP type, so the twin's
// translation unit also builds with a host compiler alone (tests/native/vad_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mfa_hip.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define MFA_VAD_FN __host__ __device__ inline
#else
#define MFA_VAD_FN inline
#endif

constexpr int kVadScanBlock = 2048;     // frames per block of the scan: 256 threads × 8 consecutive values
constexpr int kVadScanThreads = 256;    // threads of the workgroup that scans the block sums
constexpr int kVadSumLanes = 256;       // lanes of a chunk of the energy sum
constexpr int kVadSumChunk = 2048;      // frames per chunk of the energy sum
constexpr int kCmnTile = 64;            // frames a lane slides through from one directly summed window

// ---- energy VAD
// Lane `lane` of a chunk of n frames: frames lane, lane + 256, … added in that order from 0.0.
template <typename Load>
MFA_VAD_FN double mfa_vad_lane_sum(Load e, int n, int lane) {
  double s = 0.0;
  for (int i = lane; i < n; i += kVadSumLanes) s += (double)e(i);
  return s;
}

// The fold of the 256 lane sums, one level: lane l takes lane l + half.  (half = 128, 64, … 1; the caller keeps the levels apart.)
MFA_VAD_FN void mfa_vad_fold(double *lanes, int l, int half) { lanes[l] += lanes[l + half]; }

MFA_VAD_FN float mfa_vad_threshold(double sum, int64_t T, float energy_threshold, float energy_mean_scale) {
  if (energy_mean_scale == 0.0f || T <= 0) return energy_threshold;
  const double mean = sum / (double)T;
  const double scaled = (double)energy_mean_scale * mean;
  return (float)((double)energy_threshold + scaled);
}

// Frames [*lo, *hi) of [t − ctx, t + ctx] that lie inside an utterance of T frames (ctx >= 0, any size).
MFA_VAD_FN void mfa_vad_context(int64_t t, int64_t T, int32_t ctx, int64_t *lo, int64_t *hi) {
  const int64_t a = t - (int64_t)ctx, b = t + (int64_t)ctx + 1;
  *lo = a < 0 ? 0 : a;
  *hi = b > T ? T : b;
}

// Kaldi: num_count >= den_count * proportion_threshold, the counts ints and the threshold a float32.
MFA_VAD_FN bool mfa_vad_decide(int32_t num, int32_t den, float proportion_threshold) {
  const float need = (float)den * proportion_threshold;
  return (float)num >= need;
}

// ---- sliding-window CMVN
MFA_VAD_FN void mfa_cmn_window(int64_t t, int64_t T, const mfa_sliding_cmvn_opts &o, int64_t *start, int64_t *end) {
  int64_t s, e;
  if (o.center) { s = t - o.cmn_window / 2; e = s + o.cmn_window; }
  else { s = t - o.cmn_window; e = t + 1; }
  if (s < 0) { e -= s; s = 0; }
  if (!o.center && e > t) e = (t + 1 > (int64_t)o.min_window) ? t + 1 : (int64_t)o.min_window;
  if (e > T) { s -= e - T; e = T; if (s < 0) s = 0; }
  *start = s; *end = e;
}

MFA_VAD_FN float mfa_cmn_value(float x, double sum, double sumsq, int64_t n, int norm_vars) {
  const double mean = sum / (double)n;
  double d = (double)x - mean;
  if (norm_vars && n > 1) {
    const double m2 = mean * mean;
    double var = sumsq / (double)n - m2;
    if (!(var > 1e-10)) var = 1e-10;          // (a NaN is floored too)
    d = d * (1.0 / sqrt(var));
  }
  return (float)d;
}

// One column of frames [t0, t1) of an utterance of T frames: x(t) reads the column, y(t, v) takes the result.
template <typename Load, typename Store>
MFA_VAD_FN void mfa_cmn_tile(int64_t t0, int64_t t1, int64_t T, const mfa_sliding_cmvn_opts &o, Load x, Store y) {
  int64_t cs = 0, ce = 0;
  double sum = 0.0, sumsq = 0.0;
  for (int64_t t = t0; t < t1; t++) {
    int64_t s, e;
    mfa_cmn_window(t, T, o, &s, &e);
    if (t == t0 || s < cs || e < ce || s > ce) {
      sum = 0.0; sumsq = 0.0;
      for (int64_t i = s; i < e; i++) { const double v = (double)x(i); const double v2 = v * v; sum += v; sumsq += v2; }
    } else {
      for (int64_t i = cs; i < s; i++) { const double v = (double)x(i); const double v2 = v * v; sum -= v; sumsq -= v2; }
      for (int64_t i = ce; i < e; i++) { const double v = (double)x(i); const double v2 = v * v; sum += v; sumsq += v2; }
    }
    cs = s; ce = e;
    y(t, mfa_cmn_value(x(t), sum, sumsq, e - s, o.norm_vars));
  }
}

// ---- selection
// Rank j (0-based) among an utterance's kept rows → its output row, or −1 when subsampling drops it.
MFA_VAD_FN int32_t mfa_select_row(int32_t j, int32_t n) { return j % n == 0 ? j / n : -1; }
MFA_VAD_FN int32_t mfa_select_count(int32_t kept, int32_t n) { return (kept + n - 1) / n; }
