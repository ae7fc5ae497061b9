// Diagonal-GMM acoustic scoring on gfx950's matrix pipe: dense scoring of whole utterances (mfa_gmm_score_batch) and the
// exact-f32 tile walk both scoring modes use.  One translation unit, by role:
//   gmm_f32.hpp    gmm_kernel, exact-f32 MFMA (v_mfma_f32_32x32x2_f32): single-Gaussian pdfs, and everything under
//                  MFA_GMM_BF16=0 — the description below is this kernel's; gmm_band_f32_kernel[_strided], the same tile
//                  walk (score_tile) launched over the band items of a lazy-scoring window;
//   gmm_split.hpp  the split-operand kernels on v_mfma_f32_32x32x16_{f16,bf16}, blocks shared through LDS:
//                  gmm_split_single_kernel (pdfs that are one 32-row block, 17–32 Gaussians), gmm_split_small_kernel (the
//                  16-, 8- and 4-row slot classes as gathered virtual blocks), gmm_bf16_kernel (pdfs of more than 32
//                  Gaussians: runs of blocks merged by an online log-sum-exp);
//   this file      gmm_naive_kernel, a thread per (frame, column) cell: feature dims beyond 48, and MFA_GMM_NAIVE=1 as a
//                  cross-check; gmm_max_first_frame_kernel, the batch's largest first-reachable frame, for gmm_kernel's
//                  phase split; mfa_load_gmm (uploads what gmm_pack.cpp packed); mfa_gmm_score_batch, which decides the
//                  launches a model and the environment call for; mfa_gmm_launch_band_f32 (for gmm_band.hip).
// The headers are included in the order the kernels always had: this unit's register assignment depends on what is
// compiled beside what (see gmm_f32.hpp).  Lazy (windowed) scoring is gmm_band.hip; what the two units share — and the one
// definition of the arithmetic they must agree on — is gmm_common.hpp.
// Replaces DecodableAmDiagGmmScaled::LogLikelihood / gmm_compute_likes (MFA/alignment/multiprocessing.py:846-853, :1415;
// Kaldi gmm/decodable-am-diag-gmm.cc, VectorBase<float>::LogSumExp).
//
// Per Gaussian:  ll = gconst + Σ_d means_invvars[d]·x[d] + Σ_d (−½ inv_vars[d])·x[d]²   — a [rows × 2D]·[2D × frames]
// contraction.  The MFMA accumulates a k-ordered fmaf chain starting from C = gconst, i.e. bit for bit the oracle's chain.
// Per pdf:       LL = max + log Σ_{ll ≥ max+ln ε} exp(ll − max)  (Kaldi: expf, double sum, log; here: hardware exp2/log2
//                and a float32 tree sum — within 1 ulp of the Kaldi value at score magnitudes ≥ 16, see reg_expsum).
//
// Packed model (built once, gmm_pack.cpp): every pdf owns `slot` consecutive rows (slot ∈ {1,4,8,16,32·n}; pad rows have
// zero weights and gconst −1e30 so they fall under the cutoff).  Rows are stored in blocks of 32, operand-major
// (mfa_packed_offset in gmm_pack.hpp): one 16-byte load per lane yields the A operands of four consecutive MFMA steps (lane l
// feeds A[row l&31][k = 2s + (l>>5)]), and the 32 lanes of a half-wavefront read 512 contiguous bytes.
// One 32-row MFMA block then serves 32/slot pdfs of the utterance's (slot-sorted) pdf list; rows ↔ accumulator registers:
// row = (r&3) + 8(r>>2) + 4(l>>5), so 4-row slots reduce inside a lane and 8/16/32-row slots add one cross-half shuffle.
//
// Work decomposition: 1-D grid of (utterance, 256-frame tile) workgroups dealt XCD-aware; a wavefront owns NT×32 frames,
// keeps their x̃ = [x, x²] operands in registers (the B side) and streams the utterance's model rows (the A side,
// L2/MALL-resident).  With reachability information (first_frame) a wavefront only walks the prefix of each class that
// its frames can be asked for.
// Output: [T][P_u] row-major, the layout the Viterbi kernel gathers from.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "gmm_common.hpp"
#include "gmm_f32.hpp"
#include "gmm_split.hpp"

namespace {

// max over the batch of the pdfs' first possible frames → *max_ff (the persistent kernel derives its phase split from it)
__global__ void gmm_max_first_frame_kernel(const int32_t *first_frame, const int64_t *pdf_off, int n_utt, int *out) {
  const int64_t n = pdf_off[n_utt];
  int m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, first_frame[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(out, m);
}

// Straightforward kernel, a thread per (frame, column) cell: used for feature dims the MFMA kernel is not instantiated for
// and, with MFA_GMM_NAIVE=1, as an on-device cross-check of the MFMA path.  Same fmaf chain, same log-sum-exp.  The threads
// of blockIdx.y's utterance stride over its T × P cells: a list may hold a pdf more than once (a column per cluster of
// occurrences), so P is bounded by nothing the launch knows and the grid is sized for a typical utterance only.
__global__ void gmm_naive_kernel(GmmParams p) {
  const int utt = blockIdx.y;
  const int64_t f0 = p.frame_off[utt];
  const int T = (int)(p.frame_off[utt + 1] - f0);
  const int64_t l0 = p.pdf_off[utt];
  const int P = (int)(p.pdf_off[utt + 1] - l0);
  const int64_t cells = (int64_t)T * P, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < cells; idx += stride) {
    const int t = (int)(idx / P), j = (int)(idx % P);
    const int pdf = p.pdf_list[l0 + j];
    const int r0 = p.row0[pdf];
    const int rows = p.slot[pdf] == 32 ? 32 * p.nblk[pdf] : p.slot[pdf];  // pad rows carry gconst -1e30
    const float *x = p.feats + (f0 + t) * p.dim;
    float mx = -INFINITY;
    double sum = 0.0;
    for (int pass = 0; pass < 2; pass++) {
      for (int r = 0; r < rows; r++) {
        float acc = p.gc[r0 + r];
        for (int k = 0; k < 2 * p.dim; k++) {
          float xv = k < p.dim ? x[k] : x[k - p.dim] * x[k - p.dim];
          acc = fmaf(p.w[mfa_packed_offset(r0 + r, k, p.kpad)], xv, acc);
        }
        if (pass == 0) mx = fmaxf(mx, acc);
        else if (acc >= mx + p.min_log_diff) sum += (double)expf(acc - mx);
      }
    }
    p.out[p.ll_off[utt] + (size_t)idx] = (float)((double)mx + log(sum));
  }
}

}  // namespace

extern "C" {

MFA_API int mfa_load_gmm(mfa_ctx *c, int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                         const float *h_means_invvars, const float *h_inv_vars) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (dim <= 0 || num_pdfs <= 0) return c->fail("mfa_load_gmm: bad dim/num_pdfs %d/%d", dim, num_pdfs);
  GmmPacked m;
  const int bad = gmm_pack_model(dim, num_pdfs, h_pdf_offsets, h_gconsts, h_means_invvars, h_inv_vars, m);
  if (bad) return c->fail("mfa_load_gmm: pdf %d has no Gaussians", -bad - 1);
  std::vector<int32_t> ngauss(num_pdfs);
  for (int p = 0; p < num_pdfs; p++) ngauss[p] = h_pdf_offsets[p + 1] - h_pdf_offsets[p];
  const bool split = m.split();
  auto up = [](MfaBuf &dst, const auto &v) { return DevUpload<MfaHipDev>{&dst, v.data(), v.size() * sizeof(v[0])}; };
  // An empty array empties its buffer: the split operands of a model that has none (gmm_pack_model leaves them empty, all
  // but fscale), and d_w_stats, d_nrows and d_acc_tabs, which belonged to the previous layout (fmllr.hip and gmm_acc.hip
  // build them on demand).
  const std::vector<float> none;
  return dev_upload_commit<MfaHipDev>(
      c, "the acoustic model",
      {up(c->d_w, m.w), up(c->d_gc, m.gc), up(c->d_row0, m.row0), up(c->d_nblk, m.nblk), up(c->d_slot, m.slot),
       up(c->d_wb, m.wb), up(c->d_wh, m.wh), up(c->d_gch, m.gch), up(c->d_fscale, split ? m.fscale : none),
       up(c->d_w_stats, none), up(c->d_nrows, none), up(c->d_acc_tabs, none)},
      [&] {
        c->dim = dim; c->kpad = m.kpad; c->num_pdfs = num_pdfs; c->num_rows = m.rows;
        if (split) c->gmm_acc_scale = m.acc_scale;
        c->h_row0.assign(m.row0.begin(), m.row0.begin() + num_pdfs);
        c->h_slot = std::move(m.slot);
        c->h_nblk = std::move(m.nblk);
        c->h_ngauss = std::move(ngauss);
        c->all_pdfs_32row = m.all_pdfs_32row;
        c->has_multi_block = m.has_multi_block;
        c->max_nblk = m.max_nblk;
        for (int q = 0; q < 5; q++) c->has_slot_class[q] = m.has_slot_class[q];
        c->has_single32 = m.has_single32;
        c->xsplit_ready = false;   // d_xsplit was scaled with the previous model's d_fscale
        c->gmm_ready = true;
      });
}

MFA_API int mfa_debug_gmm_trace(mfa_ctx *c, void *d_trace) {
  c->gmm_trace = d_trace;
  return 0;
}

MFA_API int mfa_gmm_score_batch(mfa_ctx *c, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                int32_t max_frames, const int32_t *d_pdf_list, const int64_t *d_pdf_off,
                                const int32_t *d_class_counts, const int32_t *d_pdf_first_frame, const int64_t *d_ll_off,
                                float *d_loglikes) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  if (n_utt <= 0 || max_frames <= 0) return 0;
  if (n_utt > 65535) return c->fail("at most 65535 utterances per scoring launch (got %d)", n_utt);
  GmmParams p;
  memset(&p, 0, sizeof(p));   // every field this function does not set (the band-mode ones) must read as "off"
  p.dim = c->dim; p.kpad = c->kpad; p.num_rows = c->num_rows;
  p.w = c->d_w.ptr<float>(); p.gc = c->d_gc.ptr<float>(); p.row0 = c->d_row0.ptr<int32_t>(); p.nblk = c->d_nblk.ptr<int32_t>(); p.slot = c->d_slot.ptr<int32_t>();
  p.feats = d_feats; p.frame_off = d_frame_off; p.pdf_list = d_pdf_list; p.pdf_off = d_pdf_off;
  p.class_counts = d_class_counts; p.ll_off = d_ll_off; p.out = d_loglikes;
  p.min_log_diff = logf(1.1920928955078125e-07f);
  p.first_frame = d_pdf_first_frame;
  p.trace = (unsigned long long *)c->gmm_trace;
  const char *naive = getenv("MFA_GMM_NAIVE");
  KernelTimer kt(c, MFA_K_GMM);
  if ((naive && naive[0] == '1') || c->kpad > 96) {
    // the longest list is not known on the host side of this call (a list may repeat pdfs): max_frames * num_pdfs threads
    // per utterance, which stride over whatever cells the utterance has
    const int64_t per_utt = (int64_t)max_frames * c->num_pdfs;
    dim3 grid((unsigned)std::min<int64_t>((per_utt + 255) / 256, 1 << 20), n_utt);
    hipLaunchKernelGGL(gmm_naive_kernel, grid, dim3(256), 0, c->stream, p);
  } else {
    // 4 wavefronts per workgroup, 2 frame tiles (64 frames) per wavefront, two workgroups resident per CU (206 VGPRs).
    // Variants measured and dropped in round 1: 1 tile per wavefront (3 per SIMD: 30 TFLOP/s, spills), 8-wavefront
    // workgroups with or without a static s_setprio split (103 TFLOP/s), one wavefront per SIMD with 4 tiles and an
    // in-wavefront MFMA/epilogue software pipeline (97 TFLOP/s).
    constexpr int kFramesPerItem = 256;
    p.n_utt = n_utt;
    p.tiles = (max_frames + kFramesPerItem - 1) / kFramesPerItem;
    // Work-item counters of this call's launches (c->d_gmm_queue, zeroed here).  A launch pops its items from eight per-XCD
    // counters of its own (gmm_kernel from sixteen: two phases), so every launch gets a stretch no other one touches.
    constexpr int kQueueFirst = 0;                 // the call's first launch (under MFA_GMM_BF16=0 that is gmm_kernel: sixteen)
    constexpr int kQueueMaxFf = 16;                // not a counter: the batch's largest first frame (gmm_max_first_frame_kernel)
    constexpr int kQueueF32 = 17;                  // gmm_kernel: [8] phase 1, [8] phase 2
    constexpr int kQueueSingleRedo = 34;           // gmm_split_single_kernel's bf16×3 pass over the tiles the f16 pass declined
    constexpr int kQueueRedoCount = 51;            // not a counter: number of declined tiles
    constexpr int kQueueSmall = 64, kQueueStride = 16;   // the small-slot launches: three classes × two passes
    constexpr int kQueueMulti = kQueueSmall + 6 * kQueueStride;        // gmm_bf16_kernel after gmm_split_single_kernel
    constexpr int kQueueMultiRedo = kQueueSmall + 7 * kQueueStride;    // … and its bf16×3 pass over declined tiles
    constexpr int kQueueInts = kQueueSmall + 8 * kQueueStride;
    if (c->d_gmm_queue.reserve(c, kQueueInts * sizeof(int), "the scoring launches' work counters")) return -1;
    int *const queue = c->d_gmm_queue.ptr<int>();
    MFA_HIP_CHECK(c, hipMemsetAsync(queue, 0, kQueueInts * sizeof(int), c->stream));
    p.queue = queue + kQueueFirst;
    p.max_ff = queue + kQueueMaxFf;
    if (d_pdf_first_frame)
      hipLaunchKernelGGL(gmm_max_first_frame_kernel, dim3(64), dim3(256), 0, c->stream, d_pdf_first_frame, d_pdf_off, n_utt,
                         queue + kQueueMaxFf);
    const int num_cus = mfa_num_cus(c);
    if (num_cus <= 0) return -1;
    const int64_t items = (int64_t)n_utt * p.tiles;
    const int64_t wgs = std::min<int64_t>((int64_t)num_cus * 2, items);
    dim3 grid((unsigned)std::max<int64_t>(wgs, 1));
    const GmmSplitPasses passes = gmm_split_passes(c);
    // one launch of a kernel template whose first parameter is the model's 16-k step count
    auto launch = [&](auto kernel_of) { gmm_with_steps(c->kpad, [&](auto steps) { hipLaunchKernelGGL(kernel_of(steps), grid, dim3(256), 0, c->stream, p); }); };
    p.wb = c->d_wb.ptr<const uint4>();
    p.wh = nullptr; p.gch = nullptr; p.fscale = nullptr; p.acc_scale_inv = 1.0f; p.redo = nullptr; p.redo_mode = 0; p.redo_count = nullptr; p.skip_cc0 = 0;
    p.skip_single = 0;
    if (passes.bf16) {   // default on; MFA_GMM_BF16=0 keeps every class on the f32 kernel
      // class 0 on the bf16×3 kernel, then the f32 kernel for whatever other slot classes the lists hold (second set of
      // queue counters; an item with nothing left returns at once)
      const bool f16_ok = passes.f16;
      const bool use_f16 = f16_ok && c->has_single32;   // single-block 32-row class on the lean f16 kernel
      p.skip_cc0 = 0;
      if (f16_ok) {
        // an f16×2 pass scores every tile it can and flags the others for the bf16×3 pass that follows it
        if (c->d_gmm_redo.reserve(c, (size_t)items * sizeof(int), "the scoring redo list")) return -1;
        MFA_HIP_CHECK(c, hipMemsetAsync(c->d_gmm_redo.ptr(), 0, items * sizeof(int), c->stream));
        p.wh = c->d_wh.ptr<const uint4>(); p.gch = c->d_gch.ptr<float>(); p.fscale = c->d_fscale.ptr<float>();
        p.acc_scale_inv = 1.0f / c->gmm_acc_scale;
        p.redo = c->d_gmm_redo.ptr<int>(); p.redo_mode = 0; p.redo_count = queue + kQueueRedoCount;
      }
      if (use_f16) {
        launch([](auto steps) { return gmm_split_single_kernel<steps(), 2>; });
        p.redo_mode = 2;
        p.queue = queue + kQueueSingleRedo;
        launch([](auto steps) { return gmm_split_single_kernel<steps(), 3>; });
        p.redo_mode = 0;
        p.skip_cc0 = 1;
        p.queue = queue + kQueueMulti;
      }
      if (c->has_multi_block) {                           // pdfs of more than 32 Gaussians (and, without f16, the whole 32-row class)
        if (f16_ok) {                                     // f16×2 pass, then the bf16×3 pass over the tiles it declined
          launch([](auto steps) { return gmm_bf16_kernel<steps(), 2>; });
          p.redo_mode = 2;
          p.queue = queue + kQueueMultiRedo;
        }
        launch([](auto steps) { return gmm_bf16_kernel<steps(), 3>; });
        p.redo_mode = 0;
      } else if (!use_f16 && c->has_single32) {
        launch([](auto steps) { return gmm_split_single_kernel<steps(), 3>; });
      }
      p.skip_single = 1;
      {
        // the 16- / 8- / 4-row classes on the same pipe (f16×2 pass, then the bf16×3 pass over declined tiles), each launch
        // with its own queue counters; classes the model does not have are not launched
        int qbase = kQueueSmall;
        auto small = [&](auto slot_rows, int cls_idx) {
          if (!c->has_slot_class[cls_idx]) return;
          for (int pass = f16_ok ? 0 : 1; pass < 2; pass++) {
            p.redo_mode = f16_ok ? (pass == 0 ? 0 : 2) : 0;
            p.queue = queue + qbase; qbase += kQueueStride;
            if (pass == 0) launch([=](auto steps) { return gmm_split_small_kernel<steps(), 2, slot_rows()>; });
            else launch([=](auto steps) { return gmm_split_small_kernel<steps(), 3, slot_rows()>; });
          }
        };
        small(std::integral_constant<int, 16>{}, 1); small(std::integral_constant<int, 8>{}, 2); small(std::integral_constant<int, 4>{}, 3);
        p.skip_single = 2;
      }
      p.queue = queue + kQueueF32;
    }
    const bool only_split_classes = !c->has_slot_class[4] && p.skip_single == 2;   // no single-Gaussian pdfs left over
    if (p.skip_single && (c->all_pdfs_32row || only_split_classes)) {
      // every pdf of the model went to the split-operand kernels: nothing is left for the f32 kernel
    } else launch([](auto steps) { return gmm_kernel<2 * steps(), 2, 2, 4>; });
  }
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "dense scoring of %d utterances", n_utt);
  return 0;
}

}  // extern "C"

void mfa_gmm_launch_band_f32(mfa_ctx *c, const void *params, dim3 grid, bool strided) {
  const GmmParams &p = *static_cast<const GmmParams *>(params);
  gmm_with_steps(c->kpad, [&](auto steps) {
    if (strided) hipLaunchKernelGGL((gmm_band_f32_strided_kernel<2 * steps()>), grid, dim3(256), 0, c->stream, p);
    else hipLaunchKernelGGL((gmm_band_f32_kernel<2 * steps()>), grid, dim3(256), 0, c->stream, p);
  });
}
