// Host tables of the pitch tracker (pitch_plan.cpp), shared with the kernels' driver (pitch.hip).  Not part of the ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mfa_hip.h"
#include "resample_plan.hpp"

// What one workgroup's LDS holds (pitch.hip): four per-state arrays, the frame's window twice, three per-lag arrays.
constexpr int kMfaPitchMaxStates = 2048;    // also far below what the uint16 back-pointers can name
constexpr int kMfaPitchMaxWindow = 2048;    // resampled samples of a frame's window: N + last lag
constexpr int kMfaPitchMaxLags = 1024;      // measured integer lags

struct MfaPitchHostPlan {
  mfa_pitch_opts o{};
  int in_hz = 0, rs_hz = 0;   // sample_frequency and resample_frequency as integers
  int n_win = 0;              // N: frame_length in resampled samples
  int shift = 0;              // frame_shift in resampled samples
  int first_lag = 0, last_lag = 0, n_lags = 0;   // measured integer lags first .. last
  int n_states = 0;           // S
  int n_cols = 0;             // processed columns: POV, normalised log-pitch, raw log-pitch, each if asked for
  std::vector<float> lags;    // [S] lag_i seconds: the double recurrence, each value rounded once
  std::vector<float> sml;     // [S] soft_min_f0 * lag_i, formed in double, rounded once
  std::vector<float> pen;     // [S] c * (float)(d*d) as ONE float32 product, c = (float)(delta_pitch^2 * penalty_factor)
  int up_max_taps = 0;
  std::vector<int32_t> up_first, up_taps;   // [S] first measured-lag index and taps of state i's up-sampling filter
  std::vector<float> up_w;                  // [S][up_max_taps], rows zero padded
  MfaResampleHostPlan rs;                   // the down-sampler's filter bank
};

// Validates the options and fills the plan; on refusal returns -1 with the reason in *err and leaves *p unspecified.
int mfa_pitch_host_plan(const mfa_pitch_opts *o, MfaPitchHostPlan *p, std::string *err);
// Frames the tracker gives for num_samples input samples (at sample_frequency); see mfa_pitch_num_frames.
int64_t mfa_pitch_host_num_frames(const MfaPitchHostPlan &p, int64_t num_samples);
