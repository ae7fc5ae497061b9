// The f64 matrix product of the i-vector E-step (ivector.hip) and the PLDA transform (plda.hip): one kernel, operands
// straight from memory.  Internal to the library's device code.
#pragma once
#include "ctx.hpp"

namespace {

constexpr int kGemmBlocks = 4;             // 16-wide column blocks a wavefront of the product kernel owns

typedef double f64_gemm_acc_t __attribute__((ext_vector_type(4)));

// C [M][N] = init + A·B on the f64 matrix instruction, k ascending, 4 per step.  A(i, k) = A[i·sai + k·sak], B(k, j) =
// B[k·sbk + j·sbj], C rows of N columns.  kInit 0: the accumulator starts from C's value (C is added to); 1: from the packed
// identity (1 where column j is a diagonal element r (r + 3) / 2); 2: from `offset` in column 0; 3: from bias[j].
// kmask (may be NULL): a k whose kmask is 0 gives A = 0.  grid (column groups of 64, row groups of 64); a wavefront owns 16
// rows and kGemmBlocks column blocks, operands straight from memory (they are served by the L2: the chunk is sized to it).
struct GemmParams {
  const double *A; int64_t sai, sak;
  const double *B; int64_t sbk, sbj;
  double *C;
  int M, N, K;
  const int32_t *kmask;
  double offset;
  const double *bias;
};

template <int kInit>
__global__ __launch_bounds__(256) void f64_gemm_kernel(GemmParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const int row0 = blockIdx.y * 64 + wave * 16, col0 = blockIdx.x * (16 * kGemmBlocks);
  if (row0 >= p.M) return;                             // the whole wavefront
  f64_gemm_acc_t acc[kGemmBlocks];
#pragma unroll
  for (int nb = 0; nb < kGemmBlocks; nb++) {
    const int col = col0 + nb * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + lk + 4 * r;
      double v = 0.0;
      if (kInit == 0) { if (row < p.M && col < p.N) v = p.C[(size_t)row * p.N + col]; }
      else if (kInit == 1) {
        int d = (int)((sqrt(8.0 * (double)col + 1.0) - 1.0) * 0.5);
        while (d * (d + 3) / 2 < col) d++;
        while (d > 0 && d * (d + 3) / 2 > col) d--;
        v = d * (d + 3) / 2 == col ? 1.0 : 0.0;
      } else if (kInit == 2) v = col == 0 ? p.offset : 0.0;
      else v = col < p.N ? p.bias[col] : 0.0;
      acc[nb][r] = v;
    }
  }
  const int arow = row0 + lc;
  const bool arow_in = arow < p.M;
  const double *Ar = p.A + (size_t)(arow_in ? arow : 0) * p.sai;
  for (int k0 = 0; k0 < p.K; k0 += 4) {
    const int k = k0 + lk;
    const bool k_in = k < p.K && (!p.kmask || p.kmask[k] != 0);
    const double a = arow_in && k_in ? Ar[(size_t)k * p.sak] : 0.0;
#pragma unroll
    for (int nb = 0; nb < kGemmBlocks; nb++) {
      const int col = col0 + nb * 16 + lc;
      const double b = k_in && col < p.N ? p.B[(size_t)k * p.sbk + (size_t)col * p.sbj] : 0.0;
      acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int nb = 0; nb < kGemmBlocks; nb++) {
    const int col = col0 + nb * 16 + lc;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = row0 + lk + 4 * r;
      if (row < p.M && col < p.N) p.C[(size_t)row * p.N + col] = acc[nb][r];
    }
  }
}

template <int kInit>
void launch_gemm(mfa_ctx *c, const GemmParams &g) {
  hipLaunchKernelGGL(f64_gemm_kernel<kInit>, dim3((unsigned)((g.N + 16 * kGemmBlocks - 1) / (16 * kGemmBlocks)), (unsigned)((g.M + 63) / 64)),
                     dim3(256), 0, c->stream, g);
}

}  // namespace
