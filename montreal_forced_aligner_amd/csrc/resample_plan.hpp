// Host plan of the polyphase resampler (resample_plan.cpp), shared with the kernel's driver (resample.hip).  Not part of
// the ABI.
#pragma once
#include <cstdint>
#include <vector>

constexpr int kMfaResampleMinHz = 1000, kMfaResampleMaxHz = 384000;

struct MfaResampleHostPlan {
  int phases = 0;        // O = out_hz / gcd: outputs per unit, one filter each
  int in_per_unit = 0;   // I = in_hz / gcd: inputs per unit
  int max_taps = 0;
  std::vector<int32_t> first, taps;   // [phases] lo_i (may be negative) and taps_i
  std::vector<float> weights;         // [phases][max_taps], rows zero padded
};

inline bool mfa_resample_rates_ok(int32_t in_hz, int32_t out_hz) {
  return in_hz >= kMfaResampleMinHz && in_hz <= kMfaResampleMaxHz && out_hz >= kMfaResampleMinHz && out_hz <= kMfaResampleMaxHz;
}
// Fills `p` for a pair of distinct rates inside the limits; with fill_weights false only the sizes, first and taps.
void mfa_resample_host_plan(int32_t in_hz, int32_t out_hz, bool fill_weights, MfaResampleHostPlan *p);
// The same filter bank with the cutoff (Hz) and the zeros kept on each side chosen by the caller: the pitch tracker's
// down-sampler is LinearResample(sample_frequency -> resample_frequency, lowpass_cutoff, lowpass_filter_width).  The rates
// may be equal (one phase: a plain low-pass).  mfa_resample_host_plan is this with (0.99 x the lower Nyquist frequency, 6).
void mfa_resample_host_plan_general(int32_t in_hz, int32_t out_hz, double cutoff_hz, int zeros, bool fill_weights,
                                    MfaResampleHostPlan *p);
// Kaldi's own conditions on the filter: 0 < cutoff, twice the cutoff below both rates; and a filter no longer than the
// longest one the rate limits admit at the default filter (so that no caller can ask for gigabytes of weights).
inline bool mfa_resample_filter_ok(int32_t in_hz, int32_t out_hz, double cutoff_hz, int zeros) {
  if (!(cutoff_hz > 0.0) || !(2.0 * cutoff_hz < (double)in_hz) || !(2.0 * cutoff_hz < (double)out_hz)) return false;
  if (zeros < 1 || zeros > 64) return false;
  return (double)zeros / cutoff_hz * (double)in_hz + 1.0 <= 8192.0;   // taps of one phase
}
