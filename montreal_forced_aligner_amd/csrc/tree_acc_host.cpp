// Host twin of the tree statistics (tree_acc.hip): the whole contract of include/mfa_hip.h on host arrays, utterances and
// their frames in ascending index, every event summed by one plain loop.  No context, no device, no HIP header: this file and
// tree_acc_math.hpp are all tests/native/tree_acc_check.cpp needs.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "tree_acc_math.hpp"

extern "C" MFA_API int mfa_debug_tree_acc_host(const float *h_feats, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                               const int32_t *h_ali, const int32_t *h_tid_phone, const int32_t *h_tid_class,
                                               const int32_t *h_tid_flags, int32_t n_tids, const uint8_t *h_phone_ci,
                                               int32_t n_phones, int64_t cap, int32_t *h_frame_event, int64_t *h_n_events,
                                               int64_t *h_skipped, uint64_t *h_ev_key, int64_t *h_ev_count, double *h_ev_sum,
                                               double *h_ev_sumsq) {
  if (dim <= 0 || n_utt < 0 || n_tids < 0 || n_phones < 0 || cap < 0 || !h_n_events || !h_skipped) return -1;
  if (dim > kTreeMaxDim) return -2;
  if (n_phones >= kTreeMaxPhones) return -4;
  *h_n_events = 0;
  *h_skipped = 0;
  if (n_utt == 0) return 0;
  if (!h_frame_off) return -1;
  const int64_t total = h_frame_off[n_utt];
  if (total >= ((int64_t)1 << 31)) return -3;
  if (total < 0) return -1;
  if (total > 0 && (!h_feats || !h_ali || !h_tid_phone || !h_tid_class || !h_tid_flags || !h_phone_ci || !h_frame_event)) return -1;
  if (cap > 0 && (!h_ev_key || !h_ev_count || !h_ev_sum || !h_ev_sumsq)) return -1;

  std::vector<uint64_t> key((size_t)total, kTreeNoKey);
  std::vector<int32_t> seg_phone;          // the utterance's segments: phone and first frame; one more entry closes the list
  std::vector<int64_t> seg_start;
  for (int32_t u = 0; u < n_utt; u++) {
    const int64_t f0 = h_frame_off[u], f1 = h_frame_off[u + 1];
    if (f0 < 0 || f1 < f0 || f1 > total) return -1;
    if (f0 == f1) continue;
    seg_phone.clear();
    seg_start.clear();
    bool ok = true, open = false, tail = false;
    for (int64_t t = f0; t < f1 && ok; t++) {
      const int32_t tid = h_ali[t];
      if (!tree_tid_ok(tid, n_tids) || !tree_entry_ok(h_tid_phone[tid], h_tid_class[tid], n_phones)) { ok = false; break; }
      const int32_t phone = h_tid_phone[tid];
      if (!open) { seg_phone.push_back(phone); seg_start.push_back(t); open = true; tail = false; }
      else if (phone != seg_phone.back()) ok = false;
      tail = tree_tail(h_tid_flags[tid], tail);
      const int32_t next = t + 1 < f1 ? h_ali[t + 1] : 0;
      if (tree_segment_end(tail, tree_tid_ok(next, n_tids) ? h_tid_flags[next] : 0)) open = false;
    }
    if (!ok || open) { *h_skipped += 1; continue; }
    const size_t ns = seg_phone.size();
    seg_start.push_back(f1);
    for (size_t s = 0; s < ns; s++) {
      const int32_t c = seg_phone[s], l = s > 0 ? seg_phone[s - 1] : 0, r = s + 1 < ns ? seg_phone[s + 1] : 0;
      for (int64_t t = seg_start[s]; t < seg_start[s + 1]; t++)
        key[(size_t)t] = tree_event_key(l, c, r, h_tid_class[h_ali[t]], h_phone_ci[c] != 0);
    }
  }

  // the event order: ascending key, and inside an event ascending frame index
  std::vector<int64_t> order;
  order.reserve((size_t)total);
  for (int64_t t = 0; t < total; t++) {
    if (key[(size_t)t] != kTreeNoKey) order.push_back(t);
    h_frame_event[t] = -1;
  }
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return key[(size_t)a] < key[(size_t)b]; });
  int64_t n_events = 0;
  for (size_t i = 0; i < order.size(); i++)
    if (i == 0 || key[(size_t)order[i]] != key[(size_t)order[i - 1]]) n_events++;
  *h_n_events = n_events;
  const bool rows = n_events <= cap;
  int64_t e = -1;
  for (size_t i = 0; i < order.size(); i++) {
    const int64_t t = order[i];
    if (i == 0 || key[(size_t)t] != key[(size_t)order[i - 1]]) {
      e++;
      if (rows) {
        h_ev_key[e] = key[(size_t)t];
        h_ev_count[e] = 0;
        for (int k = 0; k < dim; k++) { h_ev_sum[(size_t)e * dim + k] = 0.0; h_ev_sumsq[(size_t)e * dim + k] = 0.0; }
      }
    }
    h_frame_event[t] = (int32_t)e;
    if (rows) {
      h_ev_count[e] += 1;
      const float *x = h_feats + (size_t)t * dim;
      for (int k = 0; k < dim; k++) tree_acc_add(x[k], h_ev_sum[(size_t)e * dim + k], h_ev_sumsq[(size_t)e * dim + k]);
    }
  }
  return 0;
}
