// Host twins of the speech-activity stage (vad.hip): the whole contract of include/mfa_hip.h on host arrays, one utterance
// after the other, through the functions of vad_math.hpp in the kernels' order.  No context, no device, no HIP header: this
// file and vad_math.hpp are all tests/native/vad_check.cpp needs.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "vad_math.hpp"

namespace {

// frame_off[0] = 0, ascending, the total below 2^31: what every entry point asks of a batch
bool offsets_ok(const int64_t *fo, int32_t n_utt) {
  if (!fo || fo[0] != 0) return false;
  for (int32_t u = 0; u < n_utt; u++)
    if (fo[u + 1] < fo[u]) return false;
  return fo[n_utt] < ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

MFA_API int mfa_debug_vad_scan_host(const int32_t *h_values, const int64_t *h_frame_off, int32_t n_utt, int32_t *h_scan,
                                    int32_t *h_totals) {
  if (n_utt < 0) return -1;
  if (n_utt == 0) return 0;
  if (!offsets_ok(h_frame_off, n_utt)) return -1;
  if (h_frame_off[n_utt] > 0 && !h_values) return -1;
  for (int32_t u = 0; u < n_utt; u++) {
    int32_t acc = 0;
    for (int64_t f = h_frame_off[u]; f < h_frame_off[u + 1]; f++) {
      if (h_scan) h_scan[f] = acc;
      acc += h_values[f];
    }
    if (h_totals) h_totals[u] = acc;
  }
  return 0;
}

MFA_API int mfa_debug_vad_host(const float *h_feats, int32_t stride, const int64_t *h_frame_off, int32_t n_utt,
                               const mfa_vad_opts *opts, float *h_vad, float *h_thr, int32_t *h_voiced) {
  if (n_utt < 0 || !opts || stride < 1 || opts->frames_context < 0) return -1;
  if (n_utt == 0) return 0;
  if (!offsets_ok(h_frame_off, n_utt) || !h_thr) return -1;
  if (h_frame_off[n_utt] > 0 && (!h_feats || !h_vad)) return -1;
  std::vector<int32_t> scan;
  for (int32_t u = 0; u < n_utt; u++) {
    const int64_t f0 = h_frame_off[u], T = h_frame_off[u + 1] - f0;
    const float *e0 = h_feats + f0 * stride;
    double sum = 0.0;
    for (int64_t c0 = 0; c0 < T; c0 += kVadSumChunk) {
      const int n = (int)(T - c0 < kVadSumChunk ? T - c0 : kVadSumChunk);
      double lanes[kVadSumLanes];
      for (int l = 0; l < kVadSumLanes; l++)
        lanes[l] = mfa_vad_lane_sum([&](int i) { return e0[(c0 + i) * stride]; }, n, l);
      for (int half = kVadSumLanes / 2; half > 0; half >>= 1)
        for (int l = 0; l < half; l++) mfa_vad_fold(lanes, l, half);
      sum += lanes[0];
    }
    const float thr = mfa_vad_threshold(sum, T, opts->energy_threshold, opts->energy_mean_scale);
    h_thr[u] = thr;
    scan.assign((size_t)T + 1, 0);
    for (int64_t t = 0; t < T; t++) scan[t + 1] = scan[t] + (e0[t * stride] > thr ? 1 : 0);
    int32_t voiced = 0;
    for (int64_t t = 0; t < T; t++) {
      int64_t lo, hi;
      mfa_vad_context(t, T, opts->frames_context, &lo, &hi);
      const bool v = mfa_vad_decide(scan[hi] - scan[lo], (int32_t)(hi - lo), opts->proportion_threshold);
      h_vad[f0 + t] = v ? 1.0f : 0.0f;
      voiced += v;
    }
    if (h_voiced) h_voiced[u] = voiced;
  }
  return 0;
}

MFA_API int mfa_debug_sliding_cmvn_host(const float *h_feats, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                        int32_t stride, const mfa_sliding_cmvn_opts *opts, float *h_out) {
  if (n_utt < 0 || !opts || dim < 1 || stride < dim || opts->cmn_window < 1 || opts->min_window < 1) return -1;
  if (n_utt == 0) return 0;
  if (!offsets_ok(h_frame_off, n_utt)) return -1;
  if (h_frame_off[n_utt] > 0 && (!h_feats || !h_out || h_out == h_feats)) return -1;
  for (int32_t u = 0; u < n_utt; u++) {
    const int64_t f0 = h_frame_off[u], T = h_frame_off[u + 1] - f0;
    const float *src = h_feats + f0 * stride;
    float *dst = h_out + f0 * stride;
    for (int64_t t0 = 0; t0 < T; t0 += kCmnTile) {
      const int64_t t1 = t0 + kCmnTile < T ? t0 + kCmnTile : T;
      for (int32_t c = 0; c < dim; c++)
        mfa_cmn_tile(t0, t1, T, *opts, [&](int64_t t) { return src[t * stride + c]; },
                     [&](int64_t t, float v) { dst[t * stride + c] = v; });
      for (int64_t t = t0; t < t1; t++)
        for (int32_t c = dim; c < stride; c++) dst[t * stride + c] = src[t * stride + c];
    }
  }
  return 0;
}

MFA_API int mfa_debug_select_frames_host(const float *h_vad, const int64_t *h_frame_off, int32_t n_utt, int32_t n,
                                         int32_t *h_src, int64_t *h_out_off) {
  if (n_utt < 0 || n < 1) return -1;
  if (!h_out_off) return -1;
  h_out_off[0] = 0;
  if (n_utt == 0) return 0;
  if (!offsets_ok(h_frame_off, n_utt)) return -1;
  if (h_frame_off[n_utt] > 0 && !h_src) return -1;
  int64_t at = 0;
  for (int32_t u = 0; u < n_utt; u++) {
    int32_t kept = 0;
    for (int64_t f = h_frame_off[u]; f < h_frame_off[u + 1]; f++) {
      if (h_vad && h_vad[f] == 0.0f) continue;
      const int32_t row = mfa_select_row(kept++, n);
      if (row >= 0) h_src[at + row] = (int32_t)f;
    }
    at += mfa_select_count(kept, n);
    h_out_off[u + 1] = at;
  }
  return 0;
}

MFA_API int mfa_debug_vad_runs_host(const float *h_vad, const int64_t *h_frame_off, int32_t n_utt, int64_t capacity,
                                    int32_t *h_run_begin, int32_t *h_run_end, int64_t *h_run_off) {
  if (n_utt < 0 || capacity < 0 || !h_run_off) return -1;
  h_run_off[0] = 0;
  if (n_utt == 0) return 0;
  if (!offsets_ok(h_frame_off, n_utt)) return -1;
  if (h_frame_off[n_utt] > 0 && !h_vad) return -1;
  if (capacity > 0 && (!h_run_begin || !h_run_end)) return -1;
  int64_t r = 0;
  for (int32_t u = 0; u < n_utt; u++) {
    const int64_t f0 = h_frame_off[u], T = h_frame_off[u + 1] - f0;
    for (int64_t t = 0; t < T; t++) {
      const bool on = h_vad[f0 + t] != 0.0f;
      if (on && (t == 0 || h_vad[f0 + t - 1] == 0.0f)) { if (r < capacity) h_run_begin[r] = (int32_t)t; }
      if (on && (t == T - 1 || h_vad[f0 + t + 1] == 0.0f)) { if (r < capacity) h_run_end[r] = (int32_t)(t + 1); r++; }
    }
    h_run_off[u + 1] = r;
  }
  return 0;
}

}  // extern "C"
