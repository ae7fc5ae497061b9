// Host twin of the equal alignment (align_equal.hip): the whole contract of include/mfa_hip.h on host arrays, one utterance
// after the other.  No context, no device, no HIP header: this file and align_equal_math.hpp are all
// tests/native/align_equal_check.cpp needs.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "align_equal_math.hpp"

extern "C" MFA_API int mfa_debug_align_equal_host(int32_t n_utt, const int64_t *h_state_off, const int64_t *h_arc_base,
                                                  const int32_t *h_start, const int32_t *h_arc_off, const float *h_final,
                                                  const int32_t *h_arc_next, const int32_t *h_arc_ilabel,
                                                  const int64_t *h_frame_off, const uint32_t *h_utt_key, uint32_t seed,
                                                  int32_t *h_ali, int32_t *h_status) {
  if (n_utt < 0) return -1;
  if (n_utt == 0) return 0;
  if (!h_state_off || !h_arc_base || !h_start || !h_arc_off || !h_final || !h_frame_off || !h_utt_key || !h_status) return -1;
  if (h_frame_off[n_utt] >= ((int64_t)1 << 31)) return -2;
  if (h_frame_off[n_utt] > h_frame_off[0] && !h_ali) return -1;
  if (h_arc_base[n_utt] > h_arc_base[0] && (!h_arc_next || !h_arc_ilabel)) return -1;
  std::vector<int32_t> loop_tid, out_tid;
  for (int32_t u = 0; u < n_utt; u++) {
    const int64_t T = h_frame_off[u + 1] - h_frame_off[u], S = h_state_off[u + 1] - h_state_off[u];
    if (S < 0 || S > INT32_MAX || h_arc_base[u + 1] - h_arc_base[u] < 0 || h_arc_base[u + 1] - h_arc_base[u] > INT32_MAX) return -1;
    if (T < 0) { h_status[u] = 2; continue; }
    MfaAeGraph g{(int32_t)S, (int32_t)(h_arc_base[u + 1] - h_arc_base[u]), h_start[u], h_arc_off + h_state_off[u] + u,
                 h_arc_next + h_arc_base[u], h_arc_ilabel + h_arc_base[u], h_final + h_state_off[u]};
    const size_t cap = (size_t)mfa_ae_path_capacity(T, S);
    loop_tid.assign(cap, 0);
    out_tid.assign(cap, 0);
    int32_t n_pos = 0, n_labels = 0, n_loopable = 0;
    int st = mfa_ae_walk(g, T, seed, h_utt_key[u], loop_tid.data(), out_tid.data(), &n_pos, &n_labels, &n_loopable);
    const int32_t extra = (int32_t)T - n_labels;
    if (st == 0 && n_loopable == 0 && extra > 0) st = 2;
    int32_t *ali = h_ali + h_frame_off[u];
    h_status[u] = st;
    if (st != 0) {
      for (int64_t t = 0; t < T; t++) ali[t] = 0;
      continue;
    }
    int64_t at = 0;
    int32_t rank = 0;
    for (int32_t i = 0; i < n_pos; i++) {
      if (loop_tid[i] != 0) {
        const int32_t loops = mfa_ae_loops(extra, n_loopable, rank++);
        for (int32_t k = 0; k < loops; k++) ali[at++] = loop_tid[i];
      }
      if (out_tid[i] != 0) ali[at++] = out_tid[i];
    }
  }
  return 0;
}
