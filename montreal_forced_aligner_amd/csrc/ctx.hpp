// Internal context of libmfa_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mfa_hip.h"

#include "dev_buf.hpp"    // DevBuf, dev_upload_commit: the device memory a context owns
#include "gmm_pack.hpp"   // mfa_packed_offset: the packed model layout
#include "pitch_plan.hpp" // MfaPitchHostPlan: the pitch tracker's host tables

enum { MFA_K_MFCC = 0, MFA_K_CMVN = 1, MFA_K_FEATS = 2, MFA_K_GMM = 3, MFA_K_VITERBI = 4, MFA_K_RESAMPLE = 5, MFA_K_PITCH = 6, MFA_K_COMPRESS = 7,
       MFA_K_ACC_LOOKUP = 8, MFA_K_ACC_SORT = 9, MFA_K_ACC_SUMS = 10, MFA_K_ACC_REDUCE = 11, MFA_K_EQUAL_ALIGN = 12,
       MFA_K_LDA_LOOKUP = 13, MFA_K_LDA_SECOND = 14, MFA_K_LDA_CLASS = 15, MFA_K_LDA_REDUCE = 16,
       MFA_K_MLLT_LOOKUP = 17, MFA_K_MLLT_SORT = 18, MFA_K_MLLT_SUMS = 19, MFA_K_MLLT_REDUCE = 20,
       MFA_K_TREE_KEYS = 21, MFA_K_TREE_ORDER = 22, MFA_K_TREE_SUMS = 23,
       MFA_K_VAD = 24, MFA_K_UBM_SELECT = 25, MFA_K_UBM_POST = 26, MFA_K_UBM_SUMS = 27, MFA_K_UBM_REDUCE = 28,
       MFA_K_IVEC_PRUNE = 29, MFA_K_IVEC_UTT = 30, MFA_K_IVEC_SCATTER = 31, MFA_K_IVEC_PRODUCTS = 32, MFA_K_IVEC_SOLVE = 33, MFA_K_IVEC_ACC = 34,
       MFA_K_PLDA_TRANSFORM = 35, MFA_K_PLDA_PREPARE = 36, MFA_K_PLDA_SWEEP = 37, MFA_K_PLDA_MERGE = 38,
       MFA_K_CLUSTER_SYMM = 39, MFA_K_CLUSTER_DEGREE = 40, MFA_K_CLUSTER_ROUNDS = 41, MFA_K_CLUSTER_LABELS = 42,
       MFA_K_SIL_OFFSETS = 43, MFA_K_SIL_SWEEP = 44,
       MFA_K_COUNT = 45 };

// The device operations of dev_buf.hpp as HIP calls.  Every device pointer a context owns is an MfaBuf: freed with the
// context, grown with reserve(), tables replaced as a set with dev_upload_commit<MfaHipDev>().
struct MfaHipDev {
  static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void free(void *p) { (void)hipFree(p); }   // nothing useful can be done with a failure here
  static int copy_h2d(void *dst, const void *src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
  static int sync(hipStream_t s) { return (int)hipStreamSynchronize(s); }
  static const char *describe(int code) { return hipGetErrorString((hipError_t)code); }
};
using MfaBuf = DevBuf<MfaHipDev>;

// Resampler plan of one pair of rates on the device (resample.hip; the host plan is resample_plan.cpp's)
struct MfaResampleDevicePlan {
  int32_t in_hz = 0, out_hz = 0;
  int phases = 0, in_per_unit = 0, max_taps = 0;
  int taps4 = 0;               // max_taps rounded up to a multiple of 4: taps the kernel runs per output
  int stride = 0;              // floats per row of d_w: taps4 + 1 (odd)
  int back = 0;                // most inputs a phase's first tap lies before its output's position
  int chunk = 0, span = 0;     // outputs per staged run of a workgroup and the inputs staged for it
  bool table_in_lds = false;   // the phase table fits the workgroup's LDS beside the span
  MfaBuf d_first;              // int32 [phases] first input of the phase, relative to its unit
  MfaBuf d_w;                  // float [phases][stride], rows zero padded
};

struct mfa_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;

  // timing
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool kernel_timing = false;
  struct Pending { int which; hipEvent_t a, b; };
  std::vector<Pending> pending;
  double k_ms[MFA_K_COUNT] = {};
  int k_n[MFA_K_COUNT] = {};
  std::vector<hipEvent_t> event_pool;

  // MFCC tables (device)
  mfa_mfcc_opts mfcc{};
  bool mfcc_ready = false;
  int win = 0, shift = 0, nfft = 0;
  MfaBuf d_window;             // float [16][16][2] window pairs in lane order, see mfcc.hip
  MfaBuf d_twiddle;            // float [2][16][16][2] W256^(i k1), W512^(i + 16 k2) in lane order, see mfcc.hip
  MfaBuf d_melw;               // float [pieces][taps] filterbank piece weights, see mfcc.hip
  MfaBuf d_melidx;             // int32 [96] first FFT bin per piece + [32] (first piece | pieces << 8) per mel bin
  int n_melw = 0;              // filterbank pieces
  int mel_np_max = 1;
  MfaBuf d_dct;                // float [nceps][nbins] with lifter folded separately
  MfaBuf d_lifter;             // float [nceps]

  std::vector<MfaResampleDevicePlan> resample_plans;   // one per (in_hz, out_hz) this context has resampled

  // pitch tracker (pitch.hip): the accepted options with their host tables, and the same tables on the device
  bool pitch_ready = false;
  MfaPitchHostPlan pitch;
  MfaBuf d_pitch_f;            // float lags [S] | soft_min_f0 * lag [S] | penalties [S] | up-sampler rows [S][taps] | down-sampler rows
  MfaBuf d_pitch_i;            // int32 up-sampler first [S] | taps [S] | down-sampler first [phases] | taps [phases]
  MfaBuf d_pitch_ws;           // one sub-launch's resampled signals, POV NCCF rows and back-pointers

  bool delta_uploaded = false; // feats.hip: this context has written the delta scales to its device's constant memory

  // GMM model (device).  mfa_load_gmm replaces all of it in one step, the buffers and the fields that describe them.
  bool gmm_ready = false;
  int dim = 0, kpad = 0, num_pdfs = 0, num_rows = 0;
  MfaBuf d_w;                  // float [num_rows][kpad] permuted weights
  MfaBuf d_wb;                 // bf16×3 split of d_w for the bf16×3 kernels (gmm_pack.cpp), or empty
  MfaBuf d_wh;                 // f16×2 split of the column-scaled d_w for gmm_split_single_kernel<…, 2>, or empty
  MfaBuf d_gch;                // float gconsts × gmm_acc_scale
  MfaBuf d_fscale;             // float [kpad] feature column scales of the f16 path
  float gmm_acc_scale = 1.0f;  // S: the f16 path's accumulators are S × the log-likelihood terms (power of two)
  MfaBuf d_gc;                 // float [num_rows]
  MfaBuf d_row0;               // int32 [num_pdfs] first packed row
  MfaBuf d_nblk;               // int32 [num_pdfs] number of 32-row blocks (slot 32) else 1
  MfaBuf d_slot;               // int32 [num_pdfs] slot class rows (1,4,8,16,32)
  std::vector<int32_t> h_slot, h_nblk, h_row0, h_ngauss;
  MfaBuf d_w_stats;            // float packed rows of the fMLLR statistics model (two-model form; mfa_fmllr_stats_model) or empty
  MfaBuf d_nrows;              // int32 [num_pdfs] packed rows per pdf (fmllr.hip builds it on first use)
  MfaBuf d_acc_tabs;           // int32 [num_pdfs] Gaussians per pdf | [num_pdfs + 1] first Gaussian (gmm_acc.hip / mllt_acc.hip build it on first use)
  bool has_slot_class[5] = {false, false, false, false, false};   // model has pdfs of slot 32 / 16 / 8 / 4 / 1 rows
  bool has_single32 = false;       // some pdf is one 32-row block (17–32 Gaussians): gmm_split_single_kernel has work
  int max_nblk = 1;                // most 32-row blocks of any pdf
  bool has_multi_block = false;    // some pdf has more than 32 Gaussians (several blocks, merged by gmm_bf16_kernel)
  bool all_pdfs_32row = false;     // every pdf is a 32-row pdf, of one block or several (no work for the f32 kernel in bf16 mode)

  // scoring scratch, grown on demand
  // d_gmm_redo is shared by the dense scorer (gmm.hip) and the band scorer (gmm_band.hip): each call sizes and zeroes it
  // for itself, and the calls are kept apart by the order of ctx->stream alone.
  MfaBuf d_gmm_redo;           // int tiles the f16 pass handed to the bf16×3 pass
  MfaBuf d_gmm_queue;          // int work-item counters of the dense scoring launches (layout: kQueue… in mfa_gmm_score_batch), zeroed per call
  MfaBuf d_xsplit;             // lazy scoring: f16 hi/lo operands of every 64-frame tile in register layout (gmm_presplit_kernel)
  MfaBuf d_xsplit_bad;         // int … and the tile's "a scaled feature left the f16 range" flag
  bool xsplit_ready = false;   // d_xsplit holds the operands of the batch mfa_align_features_batch is working on
  MfaBuf d_col_row0;           // int32 lazy scoring: first packed model row of every score column of the batch (row0[pdf_list[j]])
  MfaBuf d_col_own_last;       // int32 lazy scoring: per score column of the batch, the largest BFS depth of a state one of its arcs leaves
  MfaBuf d_band_ranges;       // int32 [n_utt][11][2]: per window, the band's index range in each run of class 0 and in classes 2..4
  int num_cus = 0;             // mfa_num_cus
  // caller-owned debug buffers: not owned, never freed here
  void *vit_stamps = nullptr;  // per-utterance phase cycle counters of the decoder (-DVIT_STAMPS builds)
  void *gmm_trace = nullptr;   // per-wavefront timeline records of the scoring kernel (mfa_debug_gmm_trace)

  // d_ws is one scratch buffer shared by the CMVN and feature (feats.hip), Viterbi (viterbi.hip), fMLLR statistics (fmllr.hip), GMM
  // statistics (gmm_acc.hip), feature codec (compress.hip), equal alignment (align_equal.hip), LDA statistics (lda_acc.hip),
  // MLLT statistics (mllt_acc.hip), tree statistics (tree_acc.hip), speech-activity (vad.hip), diagonal-UBM (ubm.hip), i-vector (ivector.hip), PLDA (plda.hip), clustering (cluster.hip) and HDBSCAN (hdbscan.hip) stages: each lays its own workspace over it for the length of one call, and the order of
  // ctx->stream is all that keeps them apart.
  MfaBuf d_ws;
  MfaBuf d_gen_ws;             // workspace of the general-graph decoder (viterbi_general.hip)
  MfaBuf d_gen_list;           // int32 utterances of the general decoder's second tier (full token pool)

  int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return -1;
  }
};

#define MFA_HIP_CHECK(ctx, expr)                                                                 \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) return (ctx)->fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// Debug aid (environment MFA_DEBUG_SYNC=1): name every launch on stderr, wait for it and report the first failing one.
inline bool mfa_debug_sync_enabled() {
  static const bool on = [] { const char *e = getenv("MFA_DEBUG_SYNC"); return e && e[0] == '1'; }();
  return on;
}
#define MFA_DEBUG_POINT(ctx, ...)                                                                         \
  do {                                                                                                    \
    if (mfa_debug_sync_enabled()) {                                                                       \
      fprintf(stderr, "[mfa] " __VA_ARGS__); fprintf(stderr, "\n"); fflush(stderr);                       \
      hipError_t _e = hipStreamSynchronize((ctx)->stream);                                                \
      if (_e == hipSuccess) _e = hipGetLastError();                                                       \
      if (_e != hipSuccess) return (ctx)->fail("launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
    }                                                                                                     \
  } while (0)

// Compute units of the context's device, queried once.  Returns 0, with the context's error set, when the query fails.
inline int mfa_num_cus(mfa_ctx *c) {
  if (c->num_cus <= 0) {
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, c->device);
    if (e != hipSuccess) { c->fail("hipGetDeviceProperties failed: %s", hipGetErrorString(e)); return 0; }
    c->num_cus = prop.multiProcessorCount;
  }
  return c->num_cus;
}

// Workgroups of a strided launch: the list passes' scoring launches and the redo sweeps walk their items on a small fixed
// grid (gmm_band_kernel<…, true>, gmm_band_f32_strided_kernel).  Four workgroups per CU: two rounds of what a CU holds of
// the band kernel (two workgroups at its 256 VGPRs), so that a wavefront which meets real work holds up one item of the
// walk, not a whole share of it — and still 64 times fewer workgroups than a list launch over a batch of 8 192 had.  A
// launch never gets more workgroups than its full grid would have.  MFA_LIST_GRID=<workgroups> overrides (tests: 1 or 3
// make every wavefront walk many items); launches over a grouped plan round up to a multiple of its runs, so there every
// value up to the run count gives one workgroup per run.  Read at every call, as MFA_GMM_BF16 / MFA_GMM_F16 are (tests
// flip it inside one process).  Returns 0, with the context's error set, when the device cannot be queried.
inline int mfa_list_grid(mfa_ctx *c) {
  const char *e = getenv("MFA_LIST_GRID");
  const int forced = e ? atoi(e) : 0;
  return forced > 0 ? forced : 4 * mfa_num_cus(c);
}

// Scoped per-kernel timing (HIP events on the ctx stream, resolved lazily).
struct KernelTimer {
  mfa_ctx *c; int which; hipEvent_t a = nullptr, b = nullptr;
  KernelTimer(mfa_ctx *ctx, int w) : c(ctx), which(w) {
    if (!c->kernel_timing) return;
    a = get(); b = get();
    (void)hipEventRecord(a, c->stream);
  }
  ~KernelTimer() {
    if (!c->kernel_timing) return;
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({which, a, b});
  }
  hipEvent_t get() {
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
  }
};

int mfa_resolve_timers(mfa_ctx *ctx);

// The reduce-then-scan exclusive scan of int32 values (vad.hip), for the stages that number things: d_G [total + 1] from d_v
// [total], total > 0; d_bsum [P] and d_base [P + 1] are its scratch, P = mfa_int_scan_blocks(total).  Three launches on
// ctx->stream.  Not part of the ABI.
size_t mfa_int_scan_blocks(int64_t total);
void mfa_int_scan(mfa_ctx *ctx, const int32_t *d_v, int64_t total, int32_t *d_bsum, int32_t *d_base, int32_t *d_G);

// ---- lazy (windowed) scoring: internal interface between the decoder driver (viterbi.hip) and the scoring kernels
// (gmm_band.hip).  Not part of the ABI.
struct MfaLazyScoring {
  mfa_score_plan plan;
  const float *d_feats;
  int max_frames;
  int window;        // frames per window of the first-beam pass (multiple of 64)
};
struct MfaWindowScore {
  int t_begin, window;          // frames [t_begin, t_begin + window) of every listed utterance
  const int32_t *band;          // [n_utt][2] {min longest-path depth, max BFS depth reachable in the window}; ignored at t_begin 0
  const int32_t *utt_list;      // utterances of this pass (NULL: all) and their count (device scalar, or NULL)
  const int32_t *n_list;
  const int32_t *done;          // per-utterance "finished" word: done[utt * done_stride + done_word] != 0 → skip
  int done_stride, done_word;
  const int32_t *lag;           // per-utterance lag word (or NULL): non-zero → the utterance's window in this call is the PREVIOUS one
  int lag_stride, lag_word;     // (t_begin − window), scored with the proven band whatever hi_slack says
  int cols_per_wave;            // 0: one wavefront walks a sub-tile's whole band; n: one wavefront per n columns of it
  int hi_slack;                 // speculative look-ahead: the band's upper depth bound is lowered by this many arcs (0: the
                                // proven bound); the decoder then checks every score it reads against mfa_band_ranges
};
// Index ranges of the columns mfa_gmm_score_window scored last, per utterance: [n_utt][kMfaRangeSlots][2], relative to the
// first column of the slot's class — slots 0..15: runs of class 0 (only the first `groups` are written), 16..18: classes 2,
// 3, 4, 19: class 1, 20: class 5.  Device memory owned by the context; valid until the next mfa_gmm_score_window call.
constexpr int kMfaRunSlots = MFA_PLAN_MAX_GROUPS;
constexpr int kMfaRangeSlots = kMfaRunSlots + 5;
const int32_t *mfa_band_ranges(mfa_ctx *ctx);
int mfa_gmm_presplit(mfa_ctx *c, const MfaLazyScoring *lazy, const mfa_graph_batch *g, const int64_t *d_frame_off, int n_utt,
                     int64_t total_frames);
int mfa_gmm_lazy_supported(mfa_ctx *ctx);   // the loaded model fits the MFMA kernels (dim <= 48)
// Score, for every listed utterance, the (frame, pdf) cells of the window that lie inside the band.  Enqueues on ctx->stream.
int mfa_gmm_score_window(mfa_ctx *ctx, const MfaLazyScoring *lazy, const MfaWindowScore *ws, const int64_t *d_frame_off,
                         int n_utt, const int64_t *d_ll_off, float *d_loglikes);
