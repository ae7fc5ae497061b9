// The arithmetic of the MLLT statistics (mllt_acc.hip) beyond the posteriors, host and device: the contract of
// include/mfa_hip.h ("MLLT statistics") operation for operation.  The posteriors are the GMM statistics' — gmm_acc_math.hpp,
// included here and not restated.  The kernel forms the same three values per term and hands them to the f64 matrix
// instruction; the host twin behind mfa_debug_mllt_acc_host (mllt_acc_host.cpp) runs exactly these functions.
// Compiled with -ffp-contract=off: every fused operation below is written as one.  Plain C++: no HIP type, so the twin's
// translation unit also builds with a host compiler alone (tests/native/mllt_acc_check.cpp).
#pragma once
#include "gmm_acc_math.hpp"

// d_k = x_k − μ_g[k]: float32, one rounding
MFA_ACC_FN float mllt_acc_diff(float x, float mean) { return x - mean; }

// γ·d_i in double: exact (24 + 24 bits)
MFA_ACC_FN double mllt_acc_left(double gamma, float di) { return gamma * (double)di; }

// full_ij = fma(γ·d_i, d_j, full_ij)
MFA_ACC_FN void mllt_acc_add(double gdi, float dj, double &full) { full = fma(gdi, (double)dj, full); }
