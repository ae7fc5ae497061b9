// The pair consumers of plda.hip's sweep as hdbscan.hip calls them (not part of the ABI): the square sweep over N points in
// the pair form of hdbscan_math.hpp (test = y, A = 0, B = y, c = 0, the epilogue (q_i + q_j) + w · sum in the consumer), with
// the core-score consumer (the k-nearest list on v, diagonal excluded) and the best-foreign-edge consumer.  One workspace for
// the whole call: mfa_pair_lay_out take()s the sweep's arrays, the caller take()s its own after it and reserve()s once.
#pragma once
#include "acc_segments.hpp"
#include "ctx.hpp"

struct MfaPairSweep {
  Workspace ws;
  size_t o_at = 0, o_bt = 0, o_c = 0, o_ps = 0, o_pi = 0, o_ks = 0, o_ki = 0;
  int Dpad = 0, keff = 0, passes = 1;
  int64_t Nspad = 0, cols_per_pass = 64;
};

// k: entries of the core consumer's lists (0: none).  Returns 0, or -1 with the context's error set.
int mfa_pair_lay_out(mfa_ctx *c, MfaPairSweep &op, int64_t N, int D, int k);
// The operands from y [N][D]; after reserve(), before the first sweep.
int mfa_pair_pack(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, int64_t N, int D);
// d_core [N]: the k-th best v of the row (−inf: fewer than k finite ones; k = 0: +inf, and without d_v no sweep runs);
// d_v [N][N] or NULL: the scores as the consumer sees them.
int mfa_pair_core_sweep(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, const double *d_q, double w, int64_t N, int D, int k,
                        double *d_core, double *d_v);
// d_row_m, d_row_j [N]: every row's best edge to a point of another component under edge_better (j = −1: none).
int mfa_pair_edge_sweep(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, const double *d_q, double w, const double *d_core,
                        const int32_t *d_comp, int64_t N, int D, double *d_row_m, int32_t *d_row_j);
// The silhouette consumer (silhouette_math.hpp), always one column pass: d_off [C + 1] the clusters' column ranges (checked by
// the caller: the kernel trusts them), d_own [N] every row's cluster; d_sil [N], and d_a, d_b, d_bj [N], d_v [N][N] or NULL.
int mfa_pair_silhouette_sweep(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, const double *d_q, double w, int32_t metric,
                              const int32_t *d_off, int32_t C, const int32_t *d_own, int64_t N, int D, double *d_sil, double *d_a, double *d_b,
                              int32_t *d_bj, double *d_v);
// The pair form's prepare step (hdbscan.hip): d_y [N][D], d_q [N] from d_x; d_flags (two int32, zeroed here) [0] |= a bad psi.
int mfa_pair_prepare(mfa_ctx *c, const double *d_x, int32_t metric, const double *d_psi, int64_t N, int D, double *d_y, double *d_q,
                     int32_t *d_flags);
