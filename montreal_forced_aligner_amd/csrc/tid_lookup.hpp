// Alignment (transition-ids) → per-frame pdf and weight through the host-built tables: one kernel, shared by the fMLLR
// statistics (fmllr.hip) and the GMM statistics (gmm_acc.hip).  Ids 0 and outside the table: pdf −1, weight 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "acc_segments.hpp"

// What the GMM statistics add to the pass (all NULL for the fMLLR caller): the frame's sort key and value — its pdf, or
// num_pdfs for a frame that takes no part (id 0 or outside the table, weight 0, a pdf the model does not have), and its
// own index —, the pdfs' frame counts and the transition-ids' (integer atomics: exact in any order).
struct TidLookupSort {
  uint32_t *key = nullptr, *val = nullptr;
  int32_t num_pdfs = 0;
  int32_t *pdf_count = nullptr;            // [num_pdfs], zeroed by the caller
  unsigned long long *tid_count = nullptr; // [n_tids] or NULL, added to
};

static __global__ void fmllr_tid_lookup_kernel(const int32_t *ali, int64_t n, const int32_t *tid2pdf, const float *tid_weight,
                                               int32_t n_tids, int32_t *pdf, float *weight, TidLookupSort s) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = t < n;
  const int tid = in ? ali[t] : 0;
  const bool ok = tid > 0 && tid < n_tids;
  const int p = ok ? tid2pdf[tid] : -1;
  const float w = ok ? tid_weight[tid] : 0.0f;
  if (in) {
    if (pdf) pdf[t] = p;
    weight[t] = w;
  }
  if (s.key) {        // (the same for every thread of the launch: the whole wavefront gets here)
    const bool take = in && ok && w != 0.0f && p >= 0 && p < s.num_pdfs;
    if (in) {
      s.key[t] = take ? (uint32_t)p : (uint32_t)s.num_pdfs;
      s.val[t] = (uint32_t)t;
    }
    // one atomic per run of equal transition-ids inside the wavefront (acc_segments.hpp has the reasoning)
    acc_wave_runs(take, tid, [&](int len) {
      atomicAdd(&s.pdf_count[p], len);
      if (s.tid_count) atomicAdd(&s.tid_count[tid], (unsigned long long)len);
    });
  }
}
