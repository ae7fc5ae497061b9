// Host side of the resampler: Kaldi's LinearResample restated (feat/resample.cc) — a Hann-windowed sinc low-pass at
// 0.99 × the lower Nyquist frequency, six zero crossings a side, one filter per output phase of a unit of
// gcd(in_hz, out_hz)⁻¹ seconds.  Everything is computed in double precision and every weight is rounded once to float32
// (Kaldi computes them in float32).  Pure host code: the CPU tests check it without a GPU.
// Compiled with -ffp-contract=off: the expressions below are evaluated operation by operation, as written.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "../../include/mfa_hip.h"
#include "resample_plan.hpp"

void mfa_resample_host_plan(int32_t in_hz, int32_t out_hz, bool fill_weights, MfaResampleHostPlan *p) {
  // the MFCC front end's filter: 0.99 x the lower Nyquist frequency, six zeros of the sinc on each side
  mfa_resample_host_plan_general(in_hz, out_hz, 0.99 * 0.5 * (double)(in_hz < out_hz ? in_hz : out_hz), 6, fill_weights, p);
}

void mfa_resample_host_plan_general(int32_t in_hz, int32_t out_hz, double fc, int zeros, bool fill_weights,
                                    MfaResampleHostPlan *p) {
  const int g = std::gcd(in_hz, out_hz);
  const int O = out_hz / g, I = in_hz / g;
  const double fin = (double)in_hz, fout = (double)out_hz;
  const double kZeros = (double)zeros;    // zeros of the sinc kept on each side
  const double ww = kZeros / (2.0 * fc);  // half window, seconds
  p->phases = O; p->in_per_unit = I; p->max_taps = 0;
  p->first.assign(O, 0); p->taps.assign(O, 0);
  for (int i = 0; i < O; i++) {
    const double t = (double)i / fout;
    const int lo = (int)std::ceil((t - ww) * fin), hi = (int)std::floor((t + ww) * fin);
    p->first[i] = lo;
    p->taps[i] = hi - lo + 1;
    if (p->taps[i] > p->max_taps) p->max_taps = p->taps[i];
  }
  p->weights.clear();
  if (!fill_weights) return;
  p->weights.assign((size_t)O * p->max_taps, 0.0f);
  for (int i = 0; i < O; i++) {
    const double t = (double)i / fout;
    float *row = p->weights.data() + (size_t)i * p->max_taps;
    for (int j = 0; j < p->taps[i]; j++) {
      const double d = (double)(p->first[i] + j) / fin - t;
      const double win = std::fabs(d) < ww ? 0.5 * (1.0 + std::cos(2.0 * M_PI * fc / kZeros * d)) : 0.0;
      const double filt = d != 0.0 ? std::sin(2.0 * M_PI * fc * d) / (M_PI * d) : 2.0 * fc;
      row[j] = (float)(win * filt / fin);
    }
  }
}

extern "C" {

MFA_API int64_t mfa_resample_num_samples(int32_t in_hz, int32_t out_hz, int64_t n) {
  if (!mfa_resample_rates_ok(in_hz, out_hz) || n < 0) return -1;
  // Kaldi LinearResample::GetNumOutputSamples with flush: outputs strictly before the end of the input, in ticks of
  // 1 / lcm(in_hz, out_hz) seconds
  const int64_t g = std::gcd(in_hz, out_hz);
  const int64_t ticks_per_in = out_hz / g, ticks_per_out = in_hz / g;   // lcm / in_hz, lcm / out_hz
  const int64_t len = n * ticks_per_in;
  if (len <= 0) return 0;
  int64_t last = len / ticks_per_out;
  if (last * ticks_per_out == len) last -= 1;
  return last + 1;
}

MFA_API int mfa_resample_plan(int32_t in_hz, int32_t out_hz, int32_t *phases, int32_t *in_per_unit, int32_t *max_taps,
                              int32_t *h_first, int32_t *h_taps, float *h_weights) {
  if (!mfa_resample_rates_ok(in_hz, out_hz) || in_hz == out_hz) return -1;
  MfaResampleHostPlan p;
  mfa_resample_host_plan(in_hz, out_hz, h_weights != nullptr, &p);
  if (phases) *phases = p.phases;
  if (in_per_unit) *in_per_unit = p.in_per_unit;
  if (max_taps) *max_taps = p.max_taps;
  for (int i = 0; i < p.phases; i++) {
    if (h_first) h_first[i] = p.first[i];
    if (h_taps) h_taps[i] = p.taps[i];
  }
  if (h_weights) std::copy(p.weights.begin(), p.weights.end(), h_weights);
  return 0;
}

MFA_API int mfa_resample_plan_general(int32_t in_hz, int32_t out_hz, double cutoff_hz, int32_t zeros, int32_t *phases,
                                      int32_t *in_per_unit, int32_t *max_taps, int32_t *h_first, int32_t *h_taps,
                                      float *h_weights) {
  if (!mfa_resample_rates_ok(in_hz, out_hz) || !mfa_resample_filter_ok(in_hz, out_hz, cutoff_hz, zeros)) return -1;
  MfaResampleHostPlan p;
  mfa_resample_host_plan_general(in_hz, out_hz, cutoff_hz, zeros, h_weights != nullptr, &p);
  if (phases) *phases = p.phases;
  if (in_per_unit) *in_per_unit = p.in_per_unit;
  if (max_taps) *max_taps = p.max_taps;
  for (int i = 0; i < p.phases; i++) {
    if (h_first) h_first[i] = p.first[i];
    if (h_taps) h_taps[i] = p.taps[i];
  }
  if (h_weights) std::copy(p.weights.begin(), p.weights.end(), h_weights);
  return 0;
}

}  // extern "C"
