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
