// Host twin of the LDA statistics (lda_acc.hip): the whole arithmetic contract of include/mfa_hip.h on host arrays,
// utterances and their frames in ascending index.  No context, no device, no HIP header: this file, lda_acc_math.hpp and
// align_equal_math.hpp are all tests/native/lda_acc_check.cpp needs.
#include <cstdint>
#include <vector>

#include "../../include/mfa_hip.h"
#include "lda_acc_math.hpp"

extern "C" MFA_API int mfa_debug_lda_acc_host(const float *h_mfcc, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                              const int32_t *h_utt2spk, const double *h_cmvn, int32_t splice_ctx,
                                              const int32_t *h_ali, const int32_t *h_tid2class, const float *h_tid_weight,
                                              int32_t n_tids, int32_t n_classes, float rand_prune, const uint32_t *h_utt_key,
                                              uint32_t seed, double *h_zero, double *h_first, double *h_second,
                                              int64_t *h_tid_count) {
  if (dim <= 0 || splice_ctx < 0 || n_utt < 0 || n_classes <= 0 || n_tids <= 0) return -1;
  const int64_t S64 = (2 * (int64_t)splice_ctx + 1) * dim;
  if (S64 > kLdaMaxSpliced) return -2;
  const int S = (int)S64;
  if (n_utt == 0) return 0;
  if (!h_frame_off) return -1;
  const int64_t total = h_frame_off[n_utt];
  if (total >= ((int64_t)1 << 31)) return -3;
  if (total <= 0) return 0;
  if (!h_mfcc || !h_ali || !h_tid2class || !h_tid_weight || !h_zero || !h_first || !h_second) return -1;
  if (h_cmvn && !h_utt2spk) return -1;
  if (rand_prune > 0.0f && !h_utt_key) return -1;
  std::vector<float> x((size_t)S), off((size_t)dim);
  std::vector<double> sec((size_t)S * S, 0.0);          // lower triangle, from zero; added to the caller's at the end
  for (int32_t u = 0; u < n_utt; u++) {
    const int64_t f0 = h_frame_off[u], f1 = h_frame_off[u + 1];
    if (f0 < 0 || f1 < f0 || f1 > total) return -1;
    for (int d = 0; d < dim; d++) off[d] = h_cmvn ? lda_cmvn_offset(h_cmvn + (size_t)h_utt2spk[u] * 2 * (dim + 1), dim, d) : 0.0f;
    for (int64_t t = f0; t < f1; t++) {
      int32_t c;
      float w;
      if (!lda_frame_class(h_ali[t], h_tid2class, h_tid_weight, n_tids, n_classes, &c, &w)) continue;
      w = lda_prune_weight(w, rand_prune, seed, rand_prune > 0.0f ? h_utt_key[u] : 0u, (uint32_t)(t - f0));
      if (w == 0.0f) continue;
      for (int i = 0; i < S; i++) {
        int col;
        const int64_t r = lda_splice_row(t, i, dim, splice_ctx, f0, f1, &col);
        x[i] = lda_cmvn_apply(h_mfcc[r * dim + col], off[col]);
      }
      const double wd = (double)w;
      h_zero[c] += wd;
      double *first = h_first + (size_t)c * S;
      for (int i = 0; i < S; i++) {
        lda_first_add(wd, x[i], first[i]);
        const double wxi = wd * (double)x[i];
        double *row = sec.data() + (size_t)i * S;
        for (int j = 0; j <= i; j++) lda_second_add(wxi, x[j], row[j]);
      }
      if (h_tid_count) h_tid_count[h_ali[t]] += 1;
    }
  }
  for (int i = 0; i < S; i++)
    for (int j = 0; j <= i; j++) {
      const double v = h_second[(size_t)i * S + j] + sec[(size_t)i * S + j];
      h_second[(size_t)i * S + j] = v;
      h_second[(size_t)j * S + i] = v;
    }
  return 0;
}
