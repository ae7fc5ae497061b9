// The PLDA stage on gfx950: what consumes an i-vector in the reference (MFA/corpus/ivector_corpus.py:123-452 transform_ivectors
// and collect_speaker_ivectors; MFA/diarization/multiprocessing.py PldaClassificationFunction, cluster_matrix,
// calculate_distance_threshold): the transform into the model's space with its length normalisation, and the matrix of
// log-likelihood ratios between test and train vectors with its row-wise consumers (best train vector, k nearest) fused into
// the sweep.  Restated from the algorithm (Kaldi's source is not among this project's references): parity unpinned, DESIGN §2.
// Arithmetic contract: include/mfa_hip.h "PLDA"; the shared arithmetic: plda_math.hpp; the host twins: plda_host.cpp.  The
// model comes with every call as device arrays: no context state.
//
//   transform  f64_gemm_kernel<3> (f64_gemm.hpp: u = x·Tᵀ + offset on the f64 matrix instruction), plda_norm_kernel (a
//              wavefront per row: the sum of the factor in a fixed order, the row scaled in place)
//   prepare    plda_prepare_kernel, a thread per train column: A, B as [k][column] (the sweep's B operands, columns padded to
//              64 and k to 4 with zeros) and c; plda_pack_kernel the same layout from the caller's A, B, c (the debug entry)
//   sweep      plda_sweep_kernel, grid (blocks of 64 test rows × column passes): a wavefront owns 16 rows and walks its pass's
//              columns 64 at a time.  score = c_j + Σ_k p²·A + Σ_k p·B, k ascending, 4 per step: the test operand is loaded
//              once per step and squared in a register for the first of the step's two matrix instructions.  The tile goes
//              to the score matrix straight from the accumulators, and through LDS to put a row's 64 columns on lanes: a
//              row's best list stays in one register pair per lane across the whole sweep (lane j the j-th best)
//   merge      plda_merge_kernel, a wavefront per row: the passes' lists in pass order into one, then the outputs
//   neighbours neighbor_sweep_kernel, the same sweep body (sweep_body<kBits>) with a fourth consumer: a row's 64 columns of a
//              step against a threshold, one ballot, is a finished word of the neighbour bit matrix that cluster.hip works on;
//              metric_prepare_kernel gives the same sweep the euclidean and dot metrics (mfa_neighbor_bits_batch)
//   silhouette pair_sil_sweep_kernel, the same sweep body (sweep_body<kSweepSil>) on the pair form with the columns ordered by
//              cluster: a lane owns (row = lane & 15, quarter = lane >> 4) and keeps one running sum, a, b and bj
// The lists have one strict order (plda_better): whatever the passes are, the merged list is the first k of that order.  No
// atomics; every sum has a fixed order: two calls on the same input give the same bits.
#include <algorithm>

#include "acc_segments.hpp"
#include "ctx.hpp"
#include "f64_gemm.hpp"
#include "hdbscan_math.hpp"
#include "pair_sweep.hpp"
#include "plda_math.hpp"
#include "silhouette_math.hpp"

namespace {

constexpr int kRowBlock = 64;              // test rows of a sweep workgroup: 16 per wavefront
constexpr int kColStep = 64;               // columns of a step: 4 blocks of the instruction's 16, afterwards one per lane
constexpr int kTileStride = 80;            // doubles per LDS tile row: 16 mod 32, so the four rows a store touches share no bank
constexpr int kSilTileStride = 81;         // the silhouette consumer's: 1 mod 32, so an 8-byte read's 32 lanes (16 rows, 2 quarters) share no bank
constexpr int kMinPassCols = 512;          // an automatic split leaves a pass at least this many columns
#ifndef PLDA_STEPS_IN_FLIGHT
#define PLDA_STEPS_IN_FLIGHT 2
#endif
constexpr int kStepsInFlight = PLDA_STEPS_IN_FLIGHT;   // steps of k whose operands a sweep wavefront loads ahead of their instructions
constexpr int kGemmRows = 1 << 20;         // rows per launch of the transform's product (grid.y)

typedef double double4_t __attribute__((ext_vector_type(4)));

// A thread per padded column j: column j < Ns from the train vector, the padding zeros.  flags[0] |= a psi that is not
// positive and finite, flags[1] |= a train_n below 1 (plain stores of the same value).
__global__ __launch_bounds__(256) void plda_prepare_kernel(const double *train, const int32_t *train_n, const double *psi, int Ns, int D,
                                                           int Dpad, int64_t Nspad, double *At, double *Bt, double *c, int32_t *flags) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Nspad) return;
  const bool in = j < Ns;
  const int32_t n = in && train_n ? train_n[j] : 1;
  if (n < 1) flags[1] = 1;
  double s_logr = 0.0, s_quad = 0.0;
  for (int k = 0; k < Dpad; k++) {
    double a = 0.0, b = 0.0;
    if (in && k < D) {
      const double ps = psi[k];
      if (!plda_psi_ok(ps)) flags[0] = 1;
      const PldaTerm t = plda_column_term(train[(size_t)j * D + k], ps, (double)n);
      a = t.A; b = t.B;
      s_logr += t.logr; s_quad += t.quad;
    }
    At[(size_t)k * Nspad + j] = a;
    Bt[(size_t)k * Nspad + j] = b;
  }
  c[j] = in ? plda_column_const(s_logr, s_quad) : 0.0;
}

// The prepare step of metrics 1 and 2 (plda_math.hpp), the same layout.
__global__ __launch_bounds__(256) void metric_prepare_kernel(const double *train, int metric, int Ns, int D, int Dpad, int64_t Nspad,
                                                             double *At, double *Bt, double *c) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Nspad) return;
  const bool in = j < Ns;
  double sum = 0.0;
  for (int k = 0; k < Dpad; k++) {
    const bool kin = in && k < D;
    const double g = kin ? train[(size_t)j * D + k] : 0.0;
    At[(size_t)k * Nspad + j] = kin ? metric_term_A(metric) : 0.0;
    Bt[(size_t)k * Nspad + j] = kin ? metric_term_B(metric, g) : 0.0;
    if (kin) sum = metric_const_add(metric, sum, g);
  }
  c[j] = in ? metric_const(metric, sum) : 0.0;
}

__global__ __launch_bounds__(256) void plda_pack_kernel(const double *A, const double *B, const double *cin, int Ns, int D, int Dpad,
                                                        int64_t Nspad, double *At, double *Bt, double *c) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Nspad) return;
  const bool in = j < Ns;
  for (int k = 0; k < Dpad; k++) {
    const bool kin = in && k < D;
    At[(size_t)k * Nspad + j] = kin ? A[(size_t)j * D + k] : 0.0;
    Bt[(size_t)k * Nspad + j] = kin ? B[(size_t)j * D + k] : 0.0;
  }
  c[j] = in ? cin[j] : 0.0;
}

// One candidate per lane (cand: it is one) into the row's sorted list (cs, ci): lane j the j-th best of plda_better's order,
// (-inf, -1) an empty entry; the first keff lanes are the answer.  The candidates are tested against the keff-th best with
// one ballot; those that pass are inserted one at a time, lowest lane first: the position is the number of better entries,
// the entries from there on move up a lane.
__device__ __forceinline__ void plda_insert(double &cs, int32_t &ci, double s, int32_t idx, bool cand, int keff, int lane) {
  double ts = __shfl(cs, keff - 1);
  int32_t ti = __shfl(ci, keff - 1);
  uint64_t mask = __ballot(cand && plda_better(s, idx, ts, ti));
  while (mask) {
    const int l = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const double ks = __shfl(s, l);
    const int32_t ki = __shfl(idx, l);
    if (plda_better(ks, ki, ts, ti)) {
      const int pos = __popcll(__ballot(plda_better(cs, ci, ks, ki)));
      const double us = __shfl_up(cs, 1);
      const int32_t ui = __shfl_up(ci, 1);
      cs = lane < pos ? cs : (lane == pos ? ks : us);
      ci = lane < pos ? ci : (lane == pos ? ki : ui);
      ts = __shfl(cs, keff - 1);
      ti = __shfl(ci, keff - 1);
    }
  }
}

struct SweepParams {
  const double *test; int Nt, Ns, D, Dpad; int64_t Nspad;
  const double *At, *Bt, *c;       // [Dpad][Nspad], [Dpad][Nspad], [Nspad]
  int64_t cols_per_pass;           // a multiple of kColStep
  int keff;                        // entries of a row's list; 0: no lists
  int exclude_diag;
  double *scores;                  // [Nt][Ns] or NULL
  double *part_s; int32_t *part_i; // [passes][Nt][keff]
};

// kSteps steps of 4 k onto the accumulators, in order: all their operands are loaded first, so that kSteps × 9 loads are in
// flight before the first matrix instruction waits for one; the order of the instructions is that of single steps.
template <int kSteps>
__device__ __forceinline__ void sweep_steps(const SweepParams &p, const double *Ar, bool arow_in, int k, int64_t col, double4_t (&acc)[4]) {
  double a[kSteps], bA[kSteps][4], bB[kSteps][4];
#pragma unroll
  for (int s = 0; s < kSteps; s++) {
    const int ks = k + 4 * s;
    a[s] = arow_in && ks < p.D ? Ar[ks] : 0.0;
    const double *Ak = p.At + (size_t)ks * p.Nspad + col, *Bk = p.Bt + (size_t)ks * p.Nspad + col;
#pragma unroll
    for (int nb = 0; nb < 4; nb++) { bA[s][nb] = Ak[nb * 16]; bB[s][nb] = Bk[nb * 16]; }
  }
#pragma unroll
  for (int s = 0; s < kSteps; s++) {
    const double a2 = a[s] * a[s];
#pragma unroll
    for (int nb = 0; nb < 4; nb++) {
      acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bA[s][nb], acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bB[s][nb], acc[nb], 0, 0, 0);
    }
  }
}

// The fourth consumer's output: a row's 64 columns of a step as one word of the neighbour matrix.
struct BitsOut {
  uint64_t *bits;                  // [Nt][W], W = Nspad / 64
  double threshold;                // bit set iff score >= threshold (a NaN score: never)
};

// The pair consumers' inputs (hdbscan_math.hpp): the epilogue's q and w, and per mode: the core consumer's optional score
// matrix; the edge consumer's core scores, components and per-pass outputs.
struct PairIn {
  const double *q; double w;       // [N]
  double *v;                       // [N][N] or NULL
  const double *core; const int32_t *comp;   // [N], [N]
  double *part_m; int32_t *part_j; // [passes][N]
};

// The silhouette consumer's inputs and outputs (silhouette_math.hpp): the metric of the distance, the clusters' column ranges
// and every row's cluster; q and w come in PairIn.
struct SilIn {
  int32_t metric, C;
  const int32_t *off, *own;        // [C + 1], [N]
  double *sil, *a, *b;             // [N]; a, b or NULL
  int32_t *bj;                     // [N] or NULL
  double *v;                       // [N][N] or NULL
};

constexpr int kSweepPlain = 0, kSweepBits = 1, kSweepCore = 2, kSweepEdge = 3, kSweepSil = 4;

// grid (blocks of 64 rows, passes).  Lane l of a step gives A[i = l & 15][k = l >> 4] = the test row's p_k (squared for the
// first instruction) and B[k][j = l & 15] = A_jk or B_jk of column j.  Register r of lane l is D[row = (l >> 4) + 4 r][col =
// l & 15].  The accumulator starts from c_j.  One body for both kernels below: kBits adds the neighbour words (b is not
// looked at without it), everything else is the same text, so the instantiation without them is the sweep it always was.
// The pair modes (kSweepCore, kSweepEdge; pr is not looked at without them) run the same sum with A = 0, c = 0 on a square
// problem and finish the score in the consumer, after the tile is staged: s = (q_row + q_col) + w · sum, the same bits for
// (i, j) and (j, i).  A row's q, core score and component sit in lane (row & 15) and are broadcast per row; a column's are
// read once per 64-column step.  Core: the k-nearest lists on s, diagonal excluded.  Edge: one running best per lane per row
// under edge_better (ls, li: the score and the far end), one butterfly per row at the end of the pass.
// The silhouette mode (kSweepSil; sl is not looked at without it) is the pair form's sum again, in one column pass (grid.y ==
// 1: a cluster is never split).  The columns are ordered by cluster, so a cluster boundary is the same column for every row:
// after staging, lane l owns row l & 15 and reads that row's 16 columns of quarter l >> 4 from the tile (contiguous; the tile's
// stride is kSilTileStride here), makes distances of them and adds them, columns ascending, into one running sum; the
// clusters that meet the step are walked in wave-uniform segments (a column outside the segment, a padding column and the
// diagonal add +0).  At a cluster's end the four quarters are added with two xor shuffles (16, then 32: (P0 + P1) + (P2 + P3)
// in every lane) and the mean is folded into the row's a or b (sil_fold).  The state of a lane is one sum, a, b, bj.
template <int kMode>
__device__ __forceinline__ void sweep_body(const SweepParams &p, const BitsOut &b, const PairIn &pr, const SilIn &sl) {
  constexpr bool kBits = kMode == kSweepBits, kPair = kMode == kSweepCore || kMode == kSweepEdge, kSil = kMode == kSweepSil;
  __shared__ double tile[4][16][kSil ? kSilTileStride : kTileStride];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kRowBlock + wave * 16;
  const bool wave_has = row0 < p.Nt;
  const int64_t c_begin = (int64_t)blockIdx.y * p.cols_per_pass, c_end = min(p.Nspad, c_begin + p.cols_per_pass);
  double ls[16];
  int32_t li[16];
#pragma unroll
  for (int rr = 0; rr < 16; rr++) { ls[rr] = -INFINITY; li[rr] = -1; }
  const int64_t arow = row0 + lc;
  const bool arow_in = arow < p.Nt;
  const double *Ar = p.test + (size_t)(arow_in ? arow : 0) * p.D;
  double q_l = 0.0, core_l = 0.0;                    // of row row0 + (lane & 15)
  int32_t comp_l = -1;
  if constexpr (kPair || kSil) {
    q_l = arow_in ? pr.q[arow] : 0.0;
    if constexpr (kMode == kSweepEdge) { core_l = arow_in ? pr.core[arow] : 0.0; comp_l = arow_in ? pr.comp[arow] : -1; }
  }
  SilRow sr = sil_row_init();                        // kSil: of row row0 + (lane & 15), the same in its four lanes
  double sil_sum = 0.0;                              // this lane's partial of the cluster sil_c
  int32_t sil_c = 0, own_l = -1;                     // sil_c: the cluster that holds the next column (wave-uniform)
  if constexpr (kSil) own_l = arow_in ? sl.own[arow] : -1;
  for (int64_t c0 = c_begin; c0 < c_end; c0 += kColStep) {
    double4_t acc[4];
    if (wave_has) {
#pragma unroll
      for (int nb = 0; nb < 4; nb++) {
        const double cj = p.c[c0 + nb * 16 + lc];
        acc[nb] = double4_t{cj, cj, cj, cj};
      }
      int k0 = 0;
      for (; k0 + 4 * kStepsInFlight <= p.Dpad; k0 += 4 * kStepsInFlight)
        sweep_steps<kStepsInFlight>(p, Ar, arow_in, k0 + lk, c0 + lc, acc);
      for (; k0 < p.Dpad; k0 += 4) sweep_steps<1>(p, Ar, arow_in, k0 + lk, c0 + lc, acc);
      if (p.scores) {
#pragma unroll
        for (int nb = 0; nb < 4; nb++) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int64_t row = row0 + lk + 4 * r, col = c0 + nb * 16 + lc;
            if (row < p.Nt && col < p.Ns) p.scores[(size_t)row * p.Ns + col] = acc[nb][r];
          }
        }
      }
    }
    if (!kBits && !kPair && !kSil && p.keff == 0) continue;   // the same for the whole grid
    __syncthreads();                                 // the previous step's readers are done
    if (wave_has) {
#pragma unroll
      for (int nb = 0; nb < 4; nb++) {
#pragma unroll
        for (int r = 0; r < 4; r++) tile[wave][lk + 4 * r][nb * 16 + lc] = acc[nb][r];
      }
    }
    __syncthreads();
    if (!wave_has) continue;
    if constexpr (kSil) {
      const int64_t colq = c0 + 16 * lk;             // this lane's first column of the step
      double d[16];
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const int64_t cl = colq + t;
        const bool cin = cl < p.Ns;
        const double s = pair_score(q_l, cin ? pr.q[cl] : 0.0, pr.w, tile[wave][lc][16 * lk + t]);
        if (sl.v && cin && arow_in) sl.v[(size_t)arow * p.Ns + cl] = s;
        d[t] = cin && cl != arow ? sil_distance(sl.metric, s) : 0.0;
      }
      const int64_t step_end = min(c0 + kColStep, (int64_t)p.Ns);
      int64_t pos = c0;
      while (pos < step_end && sil_c < sl.C) {       // wave-uniform: the segments of the clusters that meet this step
        const int64_t cl_end = sl.off[sil_c + 1], seg_end = min(cl_end, step_end);
        const int lo = (int)max(pos - colq, (int64_t)0), hi = (int)min(seg_end - colq, (int64_t)16);   // this lane's part [lo, hi)
#pragma unroll
        for (int t = 0; t < 16; t++) sil_sum += t >= lo && t < hi ? d[t] : 0.0;
        if (seg_end == cl_end) {                     // the cluster ends here
          const double h = sil_sum + __shfl_xor(sil_sum, 16);
          sil_fold(sr, own_l, sil_c, h + __shfl_xor(h, 32), cl_end - (int64_t)sl.off[sil_c]);
          sil_sum = 0.0;
          sil_c++;
        }
        pos = seg_end;
      }
      continue;
    }
    const int64_t col = c0 + lane;
    if constexpr (kBits) {
      // a ballot per row is the row's finished word; lane rr keeps row rr's, so that the 16 words leave in one vector store.
      // A pass owns whole words (its columns are a multiple of 64), and columns from Ns on never set a bit.
      uint64_t word = 0;
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const uint64_t w = __ballot(col < p.Ns && plda_neighbor(tile[wave][rr][lane], b.threshold));
        word = lane == rr ? w : word;
      }
      if (lane < 16 && row0 + lane < p.Nt) b.bits[(size_t)(row0 + lane) * (size_t)(p.Nspad / kColStep) + (size_t)(c0 / kColStep)] = word;
      if (p.keff == 0) continue;                     // the same for the whole grid
    }
    if constexpr (kPair) {
      const bool cin = col < p.Ns;
      const double qc = cin ? pr.q[col] : 0.0;
      double corec = 0.0;
      int32_t compc = -1;
      if constexpr (kMode == kSweepEdge) { corec = cin ? pr.core[col] : 0.0; compc = cin ? pr.comp[col] : -1; }
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const int64_t row = row0 + rr;
        if (row >= p.Nt) continue;                   // the same for the whole wavefront
        const double s = pair_score(__shfl(q_l, rr), qc, pr.w, tile[wave][rr][lane]);
        const bool cand = cin && plda_candidate(s) && col != row;
        if constexpr (kMode == kSweepCore) {
          if (pr.v && cin) pr.v[(size_t)row * p.Ns + col] = s;
          if (p.keff > 0) plda_insert(ls[rr], li[rr], s, (int32_t)col, cand, p.keff, lane);
        } else {
          const double m = mreach_score(s, __shfl(core_l, rr), corec);
          const int32_t compr = __shfl(comp_l, rr);  // every lane takes part: not inside the condition
          if (cand && compc != compr && (li[rr] < 0 || row_edge_better((int32_t)row, m, (int32_t)col, ls[rr], li[rr]))) {
            ls[rr] = m;
            li[rr] = (int32_t)col;
          }
        }
      }
      continue;
    }
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int64_t row = row0 + rr;
      if (row >= p.Nt) continue;                     // the same for the whole wavefront
      const double s = tile[wave][rr][lane];
      const bool cand = col < p.Ns && plda_candidate(s) && !(p.exclude_diag && col == row);
      plda_insert(ls[rr], li[rr], s, (int32_t)col, cand, p.keff, lane);
    }
  }
  if constexpr (kSil) {
    if (!arow_in || lk != 0) return;
    sl.sil[arow] = sil_finish((int64_t)sl.off[own_l + 1] - sl.off[own_l], sr.a, sr.b);
    if (sl.a) sl.a[arow] = sr.a;
    if (sl.b) sl.b[arow] = sr.b;
    if (sl.bj) sl.bj[arow] = sr.bj;
    return;
  }
  if constexpr (kMode == kSweepEdge) {
    if (!wave_has) return;
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int64_t row = row0 + rr;
      if (row >= p.Nt) continue;                     // the same for the whole wavefront
      double m = ls[rr];
      int32_t j = li[rr];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {             // a strict total order: every lane ends with the same best
        const double om = __shfl_xor(m, o);
        const int32_t oj = __shfl_xor(j, o);
        if (oj >= 0 && (j < 0 || row_edge_better((int32_t)row, om, oj, m, j))) { m = om; j = oj; }
      }
      if (lane == 0) { pr.part_m[(size_t)blockIdx.y * p.Nt + row] = m; pr.part_j[(size_t)blockIdx.y * p.Nt + row] = j; }
    }
    return;
  }
  if (p.keff == 0 || !wave_has) return;
#pragma unroll
  for (int rr = 0; rr < 16; rr++) {
    const int64_t row = row0 + rr;
    if (row >= p.Nt || lane >= p.keff) continue;
    const size_t at = ((size_t)blockIdx.y * p.Nt + row) * p.keff + lane;
    p.part_s[at] = ls[rr];
    p.part_i[at] = li[rr];
  }
}

__global__ __launch_bounds__(256) void plda_sweep_kernel(SweepParams p) { sweep_body<kSweepPlain>(p, BitsOut{nullptr, 0.0}, PairIn{}, SilIn{}); }
__global__ __launch_bounds__(256) void neighbor_sweep_kernel(SweepParams p, BitsOut b) { sweep_body<kSweepBits>(p, b, PairIn{}, SilIn{}); }
__global__ __launch_bounds__(256) void pair_core_sweep_kernel(SweepParams p, PairIn pr) { sweep_body<kSweepCore>(p, BitsOut{nullptr, 0.0}, pr, SilIn{}); }
__global__ __launch_bounds__(256) void pair_edge_sweep_kernel(SweepParams p, PairIn pr) { sweep_body<kSweepEdge>(p, BitsOut{nullptr, 0.0}, pr, SilIn{}); }
__global__ __launch_bounds__(256) void pair_sil_sweep_kernel(SweepParams p, PairIn pr, SilIn sl) { sweep_body<kSweepSil>(p, BitsOut{nullptr, 0.0}, pr, sl); }

// The pair form's operands, a thread per padded column j: A = 0, B = y as [k][column], c = 0.
__global__ __launch_bounds__(256) void pair_pack_kernel(const double *y, int Ns, int D, int Dpad, int64_t Nspad, double *At, double *Bt, double *c) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= Nspad) return;
  const bool in = j < Ns;
  for (int k = 0; k < Dpad; k++) {
    At[(size_t)k * Nspad + j] = 0.0;
    Bt[(size_t)k * Nspad + j] = in && k < D ? y[(size_t)j * D + k] : 0.0;
  }
  c[j] = 0.0;
}

// A thread per point: the core score is the k-th entry of the merged list (−inf where the list is short); k = 0: +inf.
__global__ __launch_bounds__(256) void pair_core_kernel(const double *knn_score, int64_t N, int k, double *core) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) core[i] = k > 0 ? knn_score[(size_t)i * k + (k - 1)] : INFINITY;
}

// A thread per row: the passes' bests in pass order into one.
__global__ __launch_bounds__(256) void pair_edge_merge_kernel(const double *part_m, const int32_t *part_j, int passes, int64_t N, double *row_m,
                                                              int32_t *row_j) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double m = -INFINITY;
  int32_t j = -1;
  for (int ps = 0; ps < passes; ps++) {
    const double om = part_m[(size_t)ps * N + i];
    const int32_t oj = part_j[(size_t)ps * N + i];
    if (oj >= 0 && (j < 0 || row_edge_better((int32_t)i, om, oj, m, j))) { m = om; j = oj; }
  }
  row_m[i] = m;
  row_j[i] = j;
}

// grid: 4 rows a workgroup, a wavefront each: the passes' lists in pass order into one list, then the outputs.
__global__ __launch_bounds__(256) void plda_merge_kernel(const double *part_s, const int32_t *part_i, int passes, int Nt, int keff, int k,
                                                         int32_t *best_idx, double *best_score, int32_t *knn_idx, double *knn_score) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= Nt) return;
  double cs = -INFINITY;
  int32_t ci = -1;
  for (int ps = 0; ps < passes; ps++) {
    const size_t at = ((size_t)ps * Nt + row) * keff + lane;
    const double s = lane < keff ? part_s[at] : -INFINITY;
    const int32_t idx = lane < keff ? part_i[at] : -1;
    plda_insert(cs, ci, s, idx, idx >= 0, keff, lane);
  }
  if (best_idx && lane == 0) { best_idx[row] = ci; best_score[row] = cs; }
  if (knn_idx && lane < k) { knn_idx[(size_t)row * k + lane] = ci; knn_score[(size_t)row * k + lane] = cs; }
}

// grid: 4 rows a workgroup, a wavefront each.  The row's sum: lane l its elements k = l, l + 64, … ascending, then the
// lanes' sums in a butterfly (xor 32, 16, … 1); the row is multiplied by sqrt(D / sum).
__global__ __launch_bounds__(256) void plda_norm_kernel(double *u, int64_t N, int D, const double *psi, const int32_t *num_examples, int norm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= N) return;
  double *ur = u + (size_t)row * D;
  const double inv_n = 1.0 / (double)(num_examples ? num_examples[row] : 1);
  double sum = 0.0;
  for (int k = lane; k < D; k += 64) sum += plda_norm_term(ur[k], norm == 2 ? psi[k] : 0.0, inv_n, norm);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  const double f = sqrt((double)D / sum);
  for (int k = lane; k < D; k += 64) ur[k] *= f;
}

size_t env_count(const char *name) {
  const char *e = getenv(name);
  const long v = e ? atol(e) : 0;
  return v > 0 ? (size_t)v : 0;
}

int refuse(mfa_ctx *c, const char *who, int rc, int D, int k, long long nt, long long ns) {
  switch (rc) {
    case -2: return c->fail("%s: dimension %d (1 to %d)", who, D, kPldaMaxDim);
    case -3: return c->fail("%s: lists of %d entries (1 to %d: a row's list is one wavefront register)", who, k, kPldaMaxK);
    case -5: return c->fail("%s: %lld test and %lld train vectors in one call (fewer than 2^31 each)", who, nt, ns);
    default: return c->fail("%s: a negative count", who);
  }
}

struct Outputs {
  double *scores; int32_t *best_idx; double *best_score; int32_t *knn_idx; double *knn_score;
  uint64_t *bits = nullptr; double threshold = 0.0;   // the neighbour words and their threshold (the neighbour entries only)
};

// The checks every scoring entry begins with.  Returns 0: go on; 1: nothing to do; -1: refused.
int score_checks(mfa_ctx *c, const char *who, int64_t Nt, int64_t Ns, int D, int k, const void *test, const Outputs &o) {
  const bool knn = o.knn_idx || o.knn_score;
  const int rc = plda_check_shape(D, knn ? k : 1, Nt, Ns);
  if (rc) return refuse(c, who, rc, D, k, (long long)Nt, (long long)Ns);
  if (Nt == 0) return 1;
  if (!o.scores && !o.best_idx && !o.best_score && !knn && !o.bits) return c->fail("%s: every output is NULL", who);
  if (o.bits && o.threshold != o.threshold) return c->fail("%s: a threshold that is not a number", who);
  if ((o.best_idx != nullptr) != (o.best_score != nullptr) || (o.knn_idx != nullptr) != (o.knn_score != nullptr))
    return c->fail("%s: an index output and its score output come together", who);
  if (!test) return c->fail("%s: NULL test vectors", who);
  return 0;
}

struct Operands {
  Workspace ws;
  size_t o_at = 0, o_bt = 0, o_c = 0, o_flags = 0, o_ps = 0, o_pi = 0;
  int Dpad = 0, keff = 0, passes = 1;
  int64_t Nspad = 0, cols_per_pass = kColStep;
};

// The column passes of a sweep of Nt rows over Nspad columns.
int plan_passes(mfa_ctx *c, int64_t Nt, int64_t Nspad, int64_t &cols_per_pass, int &passes) {
  const int64_t row_blocks = (Nt + kRowBlock - 1) / kRowBlock;
  const size_t forced = env_count("MFA_PLDA_PASS_COLS");
  int64_t cols = Nspad;
  if (forced) cols = (int64_t)std::min<size_t>(forced, (size_t)1 << 31);
  else {
    const int cus = mfa_num_cus(c);
    if (cus <= 0) return -1;
    const int64_t want = (2 * (int64_t)cus + row_blocks - 1) / row_blocks;     // passes that fill the device twice
    if (want > 1) cols = std::max<int64_t>(kMinPassCols, (Nspad + want - 1) / want);
  }
  cols = std::max<int64_t>(cols, (Nspad + 65534) / 65535);                    // grid.y
  cols_per_pass = std::max<int64_t>(kColStep, (cols + kColStep - 1) / kColStep * kColStep);
  passes = (int)std::max<int64_t>(1, (Nspad + cols_per_pass - 1) / cols_per_pass);
  return 0;
}

// The workspace of one scoring call: the operands, the flags and the passes' lists.
int lay_out(mfa_ctx *c, Operands &op, int64_t Nt, int64_t Ns, int D, int k, const Outputs &o) {
  op.Dpad = (D + 3) / 4 * 4;
  op.Nspad = (Ns + kColStep - 1) / kColStep * kColStep;
  op.keff = o.knn_idx ? k : (o.best_idx ? 1 : 0);
  if (plan_passes(c, Nt, op.Nspad, op.cols_per_pass, op.passes)) return -1;
  const size_t mat = (size_t)op.Dpad * (size_t)op.Nspad * 8;
  op.o_at = op.ws.take(mat); op.o_bt = op.ws.take(mat); op.o_c = op.ws.take((size_t)op.Nspad * 8); op.o_flags = op.ws.take(8);
  op.o_ps = op.ws.take((size_t)op.passes * Nt * op.keff * 8);
  op.o_pi = op.ws.take((size_t)op.passes * Nt * op.keff * 4);
  return op.ws.reserve(c, "the PLDA scoring workspace");
}

int sweep(mfa_ctx *c, const Operands &op, const double *d_test, int64_t Nt, int64_t Ns, int D, int exclude_diag, int k, const Outputs &o) {
  {
    KernelTimer kt(c, MFA_K_PLDA_SWEEP);
    const SweepParams sp{d_test, (int)Nt, (int)Ns, D, op.Dpad, op.Nspad, op.ws.at<double>(op.o_at), op.ws.at<double>(op.o_bt),
                         op.ws.at<double>(op.o_c), op.cols_per_pass, op.keff, exclude_diag ? 1 : 0, o.scores,
                         op.ws.at<double>(op.o_ps), op.ws.at<int32_t>(op.o_pi)};
    const dim3 grid((unsigned)((Nt + kRowBlock - 1) / kRowBlock), (unsigned)op.passes);
    if (o.bits) hipLaunchKernelGGL(neighbor_sweep_kernel, grid, dim3(256), 0, c->stream, sp, BitsOut{o.bits, o.threshold});
    else hipLaunchKernelGGL(plda_sweep_kernel, grid, dim3(256), 0, c->stream, sp);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "plda_sweep_kernel rows=%lld cols=%lld D=%d passes=%d k=%d bits=%d", (long long)Nt, (long long)Ns, D, op.passes, op.keff,
                    o.bits != nullptr);
  }
  if (op.keff == 0) return 0;
  KernelTimer kt(c, MFA_K_PLDA_MERGE);
  hipLaunchKernelGGL(plda_merge_kernel, dim3((unsigned)((Nt + 3) / 4)), dim3(256), 0, c->stream, op.ws.at<double>(op.o_ps),
                     op.ws.at<int32_t>(op.o_pi), op.passes, (int)Nt, op.keff, k, o.best_idx, o.best_score, o.knn_idx, o.knn_score);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "plda_merge_kernel rows=%lld passes=%d", (long long)Nt, op.passes);
  return 0;
}

// The model's prepare step onto the laid-out operands, and the two refusals that only the data can tell.
int prepare_plda(mfa_ctx *c, const char *who, const Operands &op, const double *d_train, int64_t n_train, int D, const int32_t *d_train_n,
                 const double *d_psi) {
  int32_t *flags = op.ws.at<int32_t>(op.o_flags);
  if (op.Nspad > 0) {
    KernelTimer kt(c, MFA_K_PLDA_PREPARE);
    MFA_HIP_CHECK(c, hipMemsetAsync(flags, 0, 8, c->stream));
    hipLaunchKernelGGL(plda_prepare_kernel, dim3((unsigned)((op.Nspad + 255) / 256)), dim3(256), 0, c->stream, d_train, d_train_n, d_psi,
                       (int)n_train, D, op.Dpad, op.Nspad, op.ws.at<double>(op.o_at), op.ws.at<double>(op.o_bt), op.ws.at<double>(op.o_c),
                       flags);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "plda_prepare_kernel cols=%lld D=%d", (long long)n_train, D);
  }
  if (op.Nspad > 0) {                                  // the two refusals that only the data can tell
    int32_t h_flags[2] = {0, 0};
    MFA_HIP_CHECK(c, hipMemcpyAsync(h_flags, flags, 8, hipMemcpyDeviceToHost, c->stream));
    MFA_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (h_flags[0]) return c->fail("%s: a psi entry that is not positive and finite", who);
    if (h_flags[1]) return c->fail("%s: a train vector's number of examples below 1", who);
  }
  return 0;
}

// The debug entries' prepare step: the caller's operands into the sweep's layout.
int pack_operands(mfa_ctx *c, const Operands &op, const double *d_A, const double *d_B, const double *d_c, int64_t n_train, int D) {
  if (op.Nspad == 0) return 0;
  KernelTimer kt(c, MFA_K_PLDA_PREPARE);
  hipLaunchKernelGGL(plda_pack_kernel, dim3((unsigned)((op.Nspad + 255) / 256)), dim3(256), 0, c->stream, d_A, d_B, d_c, (int)n_train, D,
                     op.Dpad, op.Nspad, op.ws.at<double>(op.o_at), op.ws.at<double>(op.o_bt), op.ws.at<double>(op.o_c));
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "plda_pack_kernel cols=%lld D=%d", (long long)n_train, D);
  return 0;
}

SweepParams pair_params(const MfaPairSweep &op, const double *d_y, int64_t N, int D, int keff) {
  return SweepParams{d_y, (int)N, (int)N, D, op.Dpad, op.Nspad, op.ws.at<double>(op.o_at), op.ws.at<double>(op.o_bt), op.ws.at<double>(op.o_c),
                     op.cols_per_pass, keff, 1, nullptr, op.ws.at<double>(op.o_ps), op.ws.at<int32_t>(op.o_pi)};
}

}  // namespace

int mfa_pair_lay_out(mfa_ctx *c, MfaPairSweep &op, int64_t N, int D, int k) {
  op.Dpad = (D + 3) / 4 * 4;
  op.Nspad = (N + kColStep - 1) / kColStep * kColStep;
  op.keff = k;
  if (plan_passes(c, N, op.Nspad, op.cols_per_pass, op.passes)) return -1;
  const size_t mat = (size_t)op.Dpad * (size_t)op.Nspad * 8, per = (size_t)std::max(k, 1);
  op.o_at = op.ws.take(mat); op.o_bt = op.ws.take(mat); op.o_c = op.ws.take((size_t)op.Nspad * 8);
  op.o_ps = op.ws.take((size_t)op.passes * N * per * 8);
  op.o_pi = op.ws.take((size_t)op.passes * N * per * 4);
  op.o_ks = op.ws.take((size_t)N * per * 8);
  op.o_ki = op.ws.take((size_t)N * per * 4);
  return 0;
}

int mfa_pair_pack(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, int64_t N, int D) {
  KernelTimer kt(c, MFA_K_PLDA_PREPARE);
  hipLaunchKernelGGL(pair_pack_kernel, dim3((unsigned)((op.Nspad + 255) / 256)), dim3(256), 0, c->stream, d_y, (int)N, D, op.Dpad, op.Nspad,
                     op.ws.at<double>(op.o_at), op.ws.at<double>(op.o_bt), op.ws.at<double>(op.o_c));
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "pair_pack_kernel cols=%lld D=%d", (long long)N, D);
  return 0;
}

int mfa_pair_core_sweep(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, const double *d_q, double w, int64_t N, int D, int k,
                        double *d_core, double *d_v) {
  const dim3 grid((unsigned)((N + kRowBlock - 1) / kRowBlock), (unsigned)op.passes);
  if (k > 0 || d_v) {
    KernelTimer kt(c, MFA_K_PLDA_SWEEP);
    hipLaunchKernelGGL(pair_core_sweep_kernel, grid, dim3(256), 0, c->stream, pair_params(op, d_y, N, D, k),
                       PairIn{d_q, w, d_v, nullptr, nullptr, nullptr, nullptr});
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "pair_core_sweep_kernel N=%lld D=%d passes=%d k=%d", (long long)N, D, op.passes, k);
  }
  KernelTimer kt(c, MFA_K_PLDA_MERGE);
  if (k > 0)
    hipLaunchKernelGGL(plda_merge_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, op.ws.at<double>(op.o_ps),
                       op.ws.at<int32_t>(op.o_pi), op.passes, (int)N, k, k, (int32_t *)nullptr, (double *)nullptr, op.ws.at<int32_t>(op.o_ki),
                       op.ws.at<double>(op.o_ks));
  hipLaunchKernelGGL(pair_core_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, op.ws.at<double>(op.o_ks), N, k, d_core);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "pair_core_kernel N=%lld k=%d", (long long)N, k);
  return 0;
}

int mfa_pair_edge_sweep(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, const double *d_q, double w, const double *d_core,
                        const int32_t *d_comp, int64_t N, int D, double *d_row_m, int32_t *d_row_j) {
  const dim3 grid((unsigned)((N + kRowBlock - 1) / kRowBlock), (unsigned)op.passes);
  {
    KernelTimer kt(c, MFA_K_PLDA_SWEEP);
    hipLaunchKernelGGL(pair_edge_sweep_kernel, grid, dim3(256), 0, c->stream, pair_params(op, d_y, N, D, 0),
                       PairIn{d_q, w, nullptr, d_core, d_comp, op.ws.at<double>(op.o_ps), op.ws.at<int32_t>(op.o_pi)});
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "pair_edge_sweep_kernel N=%lld D=%d passes=%d", (long long)N, D, op.passes);
  }
  KernelTimer kt(c, MFA_K_PLDA_MERGE);
  hipLaunchKernelGGL(pair_edge_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, op.ws.at<double>(op.o_ps),
                     op.ws.at<int32_t>(op.o_pi), op.passes, N, d_row_m, d_row_j);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "pair_edge_merge_kernel N=%lld passes=%d", (long long)N, op.passes);
  return 0;
}

int mfa_pair_silhouette_sweep(mfa_ctx *c, const MfaPairSweep &op, const double *d_y, const double *d_q, double w, int32_t metric,
                              const int32_t *d_off, int32_t C, const int32_t *d_own, int64_t N, int D, double *d_sil, double *d_a, double *d_b,
                              int32_t *d_bj, double *d_v) {
  SweepParams sp = pair_params(op, d_y, N, D, 0);
  sp.cols_per_pass = op.Nspad;                         // one pass, whatever the plan says: a cluster is never split
  KernelTimer kt(c, MFA_K_SIL_SWEEP);
  hipLaunchKernelGGL(pair_sil_sweep_kernel, dim3((unsigned)((N + kRowBlock - 1) / kRowBlock), 1), dim3(256), 0, c->stream, sp,
                     PairIn{d_q, w, nullptr, nullptr, nullptr, nullptr, nullptr}, SilIn{metric, C, d_off, d_own, d_sil, d_a, d_b, d_bj, d_v});
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "pair_sil_sweep_kernel N=%lld D=%d C=%d", (long long)N, D, C);
  return 0;
}

extern "C" {

MFA_API int mfa_plda_transform_batch(mfa_ctx *c, const double *d_x, int64_t n, int32_t D, const double *d_transform, const double *d_offset,
                                     const double *d_psi, const int32_t *d_num_examples, int32_t norm, double *d_out) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "PLDA transform";
  const int rc = plda_check_shape(D, 1, n, 0);
  if (rc) return refuse(c, who, rc, D, 1, (long long)n, 0);
  if (norm < 0 || norm > 2) return c->fail("%s: length normalisation %d (0 none, 1 simple, 2 the model's)", who, norm);
  if (n == 0) return 0;
  if (!d_x || !d_transform || !d_offset || !d_out || (norm == 2 && !d_psi)) return c->fail("%s: NULL array", who);
  if (d_x == d_out) return c->fail("%s: the output may not be the input", who);
  KernelTimer kt(c, MFA_K_PLDA_TRANSFORM);
  for (int64_t r0 = 0; r0 < n; r0 += kGemmRows) {
    const int m = (int)std::min<int64_t>(kGemmRows, n - r0);
    launch_gemm<3>(c, GemmParams{d_x + (size_t)r0 * D, D, 1, d_transform, 1, D, d_out + (size_t)r0 * D, m, D, D, nullptr, 0.0, d_offset});
  }
  if (norm != 0)
    hipLaunchKernelGGL(plda_norm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, d_out, n, D, d_psi, d_num_examples, norm);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "plda transform rows=%lld D=%d norm=%d", (long long)n, D, norm);
  return 0;
}

MFA_API int mfa_plda_score_batch(mfa_ctx *c, const double *d_test, int64_t n_test, const double *d_train, int64_t n_train, int32_t D,
                                 const int32_t *d_train_n, const double *d_psi, int32_t exclude_diagonal, int32_t k, double *d_scores,
                                 int32_t *d_best_idx, double *d_best_score, int32_t *d_knn_idx, double *d_knn_score) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "PLDA scoring";
  const Outputs o{d_scores, d_best_idx, d_best_score, d_knn_idx, d_knn_score};
  const int st = score_checks(c, who, n_test, n_train, D, k, d_test, o);
  if (st) return st < 0 ? st : 0;
  if (!d_psi || (n_train > 0 && !d_train)) return c->fail("%s: NULL model or train vectors", who);
  Operands op;
  if (lay_out(c, op, n_test, n_train, D, k, o)) return -1;
  if (prepare_plda(c, who, op, d_train, n_train, D, d_train_n, d_psi)) return -1;
  return sweep(c, op, d_test, n_test, n_train, D, exclude_diagonal, k, o);
}

MFA_API int mfa_neighbor_bits_batch(mfa_ctx *c, const double *d_test, int64_t n_test, const double *d_train, int64_t n_train, int32_t D,
                                    int32_t metric, const int32_t *d_train_n, const double *d_psi, int32_t exclude_diagonal, int32_t k,
                                    double threshold, double *d_scores, int32_t *d_best_idx, double *d_best_score, int32_t *d_knn_idx,
                                    double *d_knn_score, uint64_t *d_bits) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "neighbour sweep";
  const Outputs o{d_scores, d_best_idx, d_best_score, d_knn_idx, d_knn_score, d_bits, threshold};
  if (!plda_metric_ok(metric)) return c->fail("%s: metric %d (0 plda, 1 euclidean, 2 dot)", who, metric);
  const int st = score_checks(c, who, n_test, n_train, D, k, d_test, o);
  if (st) return st < 0 ? st : 0;
  if ((metric == kMetricPlda && !d_psi) || (n_train > 0 && !d_train)) return c->fail("%s: NULL model or train vectors", who);
  Operands op;
  if (lay_out(c, op, n_test, n_train, D, k, o)) return -1;
  if (metric == kMetricPlda) {
    if (prepare_plda(c, who, op, d_train, n_train, D, d_train_n, d_psi)) return -1;
  } else if (op.Nspad > 0) {
    KernelTimer kt(c, MFA_K_PLDA_PREPARE);
    hipLaunchKernelGGL(metric_prepare_kernel, dim3((unsigned)((op.Nspad + 255) / 256)), dim3(256), 0, c->stream, d_train, metric, (int)n_train,
                       D, op.Dpad, op.Nspad, op.ws.at<double>(op.o_at), op.ws.at<double>(op.o_bt), op.ws.at<double>(op.o_c));
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "metric_prepare_kernel cols=%lld D=%d metric=%d", (long long)n_train, D, metric);
  }
  return sweep(c, op, d_test, n_test, n_train, D, exclude_diagonal, k, o);
}

MFA_API int mfa_debug_plda_sweep_batch(mfa_ctx *c, const double *d_test, int64_t n_test, int32_t D, const double *d_A, const double *d_B,
                                       const double *d_c, int64_t n_train, int32_t exclude_diagonal, int32_t k, double *d_scores,
                                       int32_t *d_best_idx, double *d_best_score, int32_t *d_knn_idx, double *d_knn_score) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "PLDA sweep";
  const Outputs o{d_scores, d_best_idx, d_best_score, d_knn_idx, d_knn_score};
  const int st = score_checks(c, who, n_test, n_train, D, k, d_test, o);
  if (st) return st < 0 ? st : 0;
  if (n_train > 0 && (!d_A || !d_B || !d_c)) return c->fail("%s: NULL operands", who);
  Operands op;
  if (lay_out(c, op, n_test, n_train, D, k, o)) return -1;
  if (pack_operands(c, op, d_A, d_B, d_c, n_train, D)) return -1;
  return sweep(c, op, d_test, n_test, n_train, D, exclude_diagonal, k, o);
}

MFA_API int mfa_debug_neighbor_sweep_batch(mfa_ctx *c, const double *d_test, int64_t n_test, int32_t D, const double *d_A, const double *d_B,
                                           const double *d_c, int64_t n_train, int32_t exclude_diagonal, int32_t k, double threshold,
                                           double *d_scores, int32_t *d_best_idx, double *d_best_score, int32_t *d_knn_idx,
                                           double *d_knn_score, uint64_t *d_bits) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const char *who = "neighbour sweep";
  const Outputs o{d_scores, d_best_idx, d_best_score, d_knn_idx, d_knn_score, d_bits, threshold};
  const int st = score_checks(c, who, n_test, n_train, D, k, d_test, o);
  if (st) return st < 0 ? st : 0;
  if (n_train > 0 && (!d_A || !d_B || !d_c)) return c->fail("%s: NULL operands", who);
  Operands op;
  if (lay_out(c, op, n_test, n_train, D, k, o)) return -1;
  if (pack_operands(c, op, d_A, d_B, d_c, n_train, D)) return -1;
  return sweep(c, op, d_test, n_test, n_train, D, exclude_diagonal, k, o);
}

}  // extern "C"
