// Host side of the pitch tracker: option checks and the tables the kernels read (state lags, the up-sampler's filter of
// every state, the transition penalties, the down-sampler's filter bank).  Kaldi's pitch extractor (feat/pitch-functions.cc,
// feat/resample.cc: SelectLags, ArbitraryResample, LinearResample) restated; everything is computed in double precision and
// every table value is rounded once to float32.  Pure host code: the CPU tests check it without a GPU.
// Compiled with -ffp-contract=off: the expressions below are evaluated operation by operation, as written.
#include <cmath>
#include <cstdio>

#include "pitch_plan.hpp"

namespace {

int refuse(std::string *err, const char *fmt, double a = 0, double b = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b);
  if (err) *err = buf;
  return -1;
}

bool is_int_rate(float f) { return f >= (float)kMfaResampleMinHz && f <= (float)kMfaResampleMaxHz && f == std::floor(f); }

}  // namespace

int mfa_pitch_host_plan(const mfa_pitch_opts *o, MfaPitchHostPlan *p, std::string *err) {
  if (!o) return refuse(err, "pitch: no options");
  if (o->add_delta_pitch)
    return refuse(err, "pitch: add_delta_pitch is not supported (Kaldi adds Gaussian noise to delta-pitch: it has no parity domain)");
  if (o->preemphasis != 0.0f) return refuse(err, "pitch: preemphasis %g is not supported (MFA's value is 0)", o->preemphasis);
  if (!is_int_rate(o->sample_frequency) || !is_int_rate(o->resample_frequency))
    return refuse(err, "pitch: sample_frequency %g and resample_frequency %g must be whole numbers of Hz inside the resampler's limits",
                  o->sample_frequency, o->resample_frequency);
  if (!(o->min_f0 > 0.0f) || !(o->min_f0 < o->max_f0))
    return refuse(err, "pitch: need 0 < min_f0 < max_f0 (got %g, %g)", o->min_f0, o->max_f0);
  if (!(o->max_f0 < 0.5f * o->resample_frequency - 100.0f))
    return refuse(err, "pitch: max_f0 %g must lie more than 100 Hz below half the resample_frequency %g", o->max_f0,
                  o->resample_frequency);
  if (!(o->delta_pitch > 0.0f) || !(o->delta_pitch <= 1.0f)) return refuse(err, "pitch: delta_pitch %g outside (0, 1]", o->delta_pitch);
  if (!(o->penalty_factor >= 0.0f) || !(o->soft_min_f0 >= 0.0f) || !(o->nccf_ballast >= 0.0f))
    return refuse(err, "pitch: penalty_factor, soft_min_f0 and nccf_ballast must not be negative");
  if (!(o->frame_length_ms > 0.0f) || !(o->frame_shift_ms > 0.0f)) return refuse(err, "pitch: frame length and shift must be positive");
  if (o->upsample_filter_width < 1 || o->upsample_filter_width > 64)
    return refuse(err, "pitch: upsample_filter_width %g outside 1 - 64", o->upsample_filter_width);
  if (o->normalization_context < 0 || o->normalization_context > 100000)
    return refuse(err, "pitch: normalization_context %g outside 0 - 100000", o->normalization_context);
  const int in_hz = (int)o->sample_frequency, rs_hz = (int)o->resample_frequency;
  if (!mfa_resample_filter_ok(in_hz, rs_hz, (double)o->lowpass_cutoff, o->lowpass_filter_width))
    return refuse(err, "pitch: lowpass_cutoff %g Hz with filter width %g does not give a filter (twice the cutoff must lie below both rates)",
                  o->lowpass_cutoff, o->lowpass_filter_width);
  const int n_cols = (o->add_pov_feature != 0) + (o->add_normalized_log_pitch != 0) + (o->add_raw_log_pitch != 0);
  if (n_cols == 0) return refuse(err, "pitch: none of add_pov_feature, add_normalized_log_pitch, add_raw_log_pitch is set");

  const double fs = (double)rs_hz;
  const double n_win = fs * (double)o->frame_length_ms / 1000.0, shift = fs * (double)o->frame_shift_ms / 1000.0;
  const double min_lag = 1.0 / (double)o->max_f0, max_lag = 1.0 / (double)o->min_f0;
  const double w = (double)o->upsample_filter_width / (2.0 * fs);
  const double first = std::ceil(fs * (min_lag - w)), last = std::floor(fs * (max_lag + w));
  if (first < 1.0) return refuse(err, "pitch: the first measured lag would be %g (max_f0 too close to the Nyquist frequency)", first);
  if (last - first + 1.0 > (double)kMfaPitchMaxLags)
    return refuse(err, "pitch: %g measured lags, at most %g fit a workgroup", last - first + 1.0, (double)kMfaPitchMaxLags);
  if (n_win < 1.0 || shift < 1.0 || n_win + last > (double)kMfaPitchMaxWindow)
    return refuse(err, "pitch: a window of %g samples (frame + last lag), at most %g fit a workgroup (and frame and shift need a sample each)",
                  n_win + last, (double)kMfaPitchMaxWindow);
  // states: lag_{i+1} = lag_i (1 + delta_pitch) in double while <= 1 / min_f0
  const double ratio = 1.0 + (double)o->delta_pitch;
  if (std::log(max_lag / min_lag) / std::log(ratio) + 1.0 > (double)kMfaPitchMaxStates)
    return refuse(err, "pitch: about %g states, at most %g fit a workgroup", std::log(max_lag / min_lag) / std::log(ratio) + 1.0,
                  (double)kMfaPitchMaxStates);
  std::vector<double> lags;
  for (double lag = min_lag; lag <= max_lag; lag *= ratio) lags.push_back(lag);
  const int S = (int)lags.size();
  if (S < 1 || S > kMfaPitchMaxStates) return refuse(err, "pitch: %g states, at most %g fit a workgroup", (double)S, (double)kMfaPitchMaxStates);

  p->o = *o;
  p->in_hz = in_hz; p->rs_hz = rs_hz;
  p->n_win = (int)n_win; p->shift = (int)shift;
  p->first_lag = (int)first; p->last_lag = (int)last; p->n_lags = p->last_lag - p->first_lag + 1;
  p->n_states = S; p->n_cols = n_cols;
  p->lags.resize(S); p->sml.resize(S); p->pen.resize(S);
  const float c = (float)((double)o->delta_pitch * (double)o->delta_pitch * (double)o->penalty_factor);
  for (int i = 0; i < S; i++) {
    p->lags[i] = (float)lags[i];
    p->sml[i] = (float)((double)o->soft_min_f0 * lags[i]);
    p->pen[i] = c * (float)(i * i);   // one float32 product (i*i < 2^24 is exact)
  }
  // up-sampler: ArbitraryResample(n_lags inputs at resample_frequency, cutoff resample_frequency / 2, sample points
  // lag_i - first / resample_frequency, upsample_filter_width zeros)
  const double fc = 0.5 * fs, zeros = (double)o->upsample_filter_width, fw = zeros / (2.0 * fc);
  p->up_first.assign(S, 0); p->up_taps.assign(S, 0); p->up_max_taps = 0;
  std::vector<double> t(S);
  for (int i = 0; i < S; i++) {
    t[i] = lags[i] - first / fs;
    int lo = (int)std::ceil(fs * (t[i] - fw)), hi = (int)std::floor(fs * (t[i] + fw));
    if (lo < 0) lo = 0;
    if (hi > p->n_lags - 1) hi = p->n_lags - 1;
    p->up_first[i] = lo;
    p->up_taps[i] = hi - lo + 1;
    if (p->up_taps[i] < 1) return refuse(err, "pitch: state %g has no measured lag inside its up-sampling filter", (double)i);
    if (p->up_taps[i] > p->up_max_taps) p->up_max_taps = p->up_taps[i];
  }
  p->up_w.assign((size_t)S * p->up_max_taps, 0.0f);
  for (int i = 0; i < S; i++)
    for (int j = 0; j < p->up_taps[i]; j++) {
      const double d = t[i] - (double)(p->up_first[i] + j) / fs;
      const double win = std::fabs(d) < fw ? 0.5 * (1.0 + std::cos(2.0 * M_PI * fc / zeros * d)) : 0.0;
      const double filt = d != 0.0 ? std::sin(2.0 * M_PI * fc * d) / (M_PI * d) : 2.0 * fc;
      p->up_w[(size_t)i * p->up_max_taps + j] = (float)(filt * win / fs);
    }
  mfa_resample_host_plan_general(in_hz, rs_hz, (double)o->lowpass_cutoff, o->lowpass_filter_width, true, &p->rs);
  return 0;
}

int64_t mfa_pitch_host_num_frames(const MfaPitchHostPlan &p, int64_t num_samples) {
  if (num_samples <= 0) return 0;
  const int64_t n = p.in_hz == p.rs_hz ? num_samples : mfa_resample_num_samples(p.in_hz, p.rs_hz, num_samples);
  if (n < p.n_win) return 0;
  if (p.o.snip_edges) return (n - p.n_win) / p.shift + 1;
  return (int64_t)((double)n / (double)p.shift + 0.5);
}
