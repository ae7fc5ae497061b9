// Batched beam-pruned token-passing Viterbi for gfx950: one wavefront per utterance, frame loop inside the kernel.
// Replaces GmmAligner.align_utterance / export_alignments (MFA/alignment/multiprocessing.py:846-853;
// MFA/online/alignment.py:107) = Kaldi AlignUtteranceWrapper + FasterDecoder.
//
// The result is REQUIRED to equal the sequential decoder's, so the kernel reproduces its order-dependent rules in
// parallel form rather than approximating them:
//   * tokens live in an ORDERED list (Kaldi HashList order: buckets by first occupancy, insertion order inside);
//   * a candidate (token i, arc k) is created iff its cost is below the running cutoff
//       min(seed from the best token, min over all EARLIER candidates) + adaptive_beam
//     — an exclusive prefix-min over candidates in list×arc order (wave scan, no serial loop);
//   * per destination state the cheapest candidate wins, ties to the earliest candidate (two-phase LDS atomics);
//   * the next list is produced by a prefix-sum compaction keyed by each state's first creating candidate
//     (and its hash bucket's, when the graph has more states than hash buckets);
//   * GetCutoff's min_active=20 rule is evaluated exactly (counting selection of the 21st smallest cost).
// Costs are float64 exactly as Kaldi's tokens; arc weights / acoustic costs float32.
//
// Memory: per-wavefront LDS holds only the atomically updated tables (state→slot map, per-slot cost/first/winner, the
// candidate-ordinal counter array); token lists, the candidate stash and the back-pointer records stream through a
// per-utterance HBM workspace (288 GB lets every in-flight utterance keep its own).  No MFMA: this is min-plus DP.
//
// Sources, one translation unit: viterbi_common.hpp (constants, parameters, wavefront primitives, finalisation),
// viterbi_eps.hpp (slot table and epsilon closures the two frame-loop kernels share), viterbi_wave.hpp (viterbi_kernel),
// viterbi_small.hpp (viterbi_small_kernel, viterbi_finish_kernel), viterbi_plan.hpp (the launch plan: host code without HIP,
// also behind mfa_debug_viterbi_plan and swept by tests/native/viterbi_plan_check.cpp); this file: helper kernels,
// workspace, align_impl, the C entry points.
#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <vector>

#include "viterbi_common.hpp"
#include "viterbi_wave.hpp"
#include "viterbi_small.hpp"
#include "viterbi_plan.hpp"

namespace {

// Build the retry list: utterances left pending by the first pass.
__global__ void collect_pending_kernel(const int32_t *status, int n_utt, int code, int32_t *list, int32_t *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_utt && status[i] == code) list[atomicAdd(count, 1)] = i;
}
__global__ void finalize_pending_kernel(int32_t *status, int n_utt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_utt && status[i] == ST_PENDING) status[i] = ST_FAILED;
}

// One 16-byte record per arc for the frame loop: {destination state, (first arc << 7 | out-degree) of the destination,
// score column, weight}.  The destination's arc range folds the arc_off lookup of the NEXT frame into this frame's arc
// fetch (one dependent HBM/L2 round trip per frame instead of three), and the record makes that fetch one 16-byte load
// touching one line instead of four 4-byte gathers from four arrays.
__global__ void arcnext_kernel(mfa_graph_batch g, uint4 *out, u32 *epsinfo, int max_states) {
  const int utt = blockIdx.x;
  const int64_t so = g.d_state_off[utt], ab = g.d_arc_base[utt];
  const int64_t na = g.d_arc_base[utt + 1] - ab;
  const int S = (int)(g.d_state_off[utt + 1] - so);
  const int32_t *arc_off = g.d_arc_off + so + utt;
  const int32_t *nemit = g.d_state_nemit ? g.d_state_nemit + so : nullptr;   // emitting arcs per state (the rest are epsilon arcs)
  for (int64_t a = threadIdx.x; a < na; a += blockDim.x) {
    const int d = g.d_arc_next[ab + a];
    const u32 deg = nemit ? (u32)nemit[d] : (u32)(arc_off[d + 1] - arc_off[d]);
    const u32 an = ((u32)arc_off[d] << 7) | min(deg, 127u);
    out[ab + a] = make_uint4((u32)d, an, (u32)g.d_arc_col[ab + a], __float_as_uint(g.d_arc_weight[ab + a]));
  }
  if (epsinfo && nemit)
    for (int s_ = threadIdx.x; s_ < S && s_ < max_states; s_ += blockDim.x) {
      const int first = arc_off[s_] + nemit[s_], n_eps = arc_off[s_ + 1] - first;
      epsinfo[(size_t)utt * max_states + s_] = ((u32)first << 7) | (u32)min(max(n_eps, 0), 127);
    }
}

// The launch plan (capacities, LDS bytes, where the token lists live, the state→slot table) is viterbi_plan.hpp's: host code
// without HIP, which restates these constants of the kernels.
constexpr int kLlCap = vplan::kLlCap;
static_assert(vplan::kBmWords == kBmWords && vplan::kEpsWordsPerSlot == kEpsWordsPerSlot && vplan::kSmallN == kSmallN,
              "viterbi_plan.hpp restates the kernels' constants");
static_assert(vplan::kCodePending == ST_PENDING && vplan::kCodeGrow == ST_GROW, "viterbi_plan.hpp restates the status codes");

struct WsLayout {
  size_t arcnext, state, cost, sta, stb, stkey, bp, tokoff, hash, list, count, vstate, band, eps, total;
};
WsLayout ws_layout(int n_utt, int64_t total_frames, int N, int C, int bpf, int64_t total_arcs, int64_t eps_states = 0) {
  WsLayout w; size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  w.arcnext = take((size_t)total_arcs * 16);
  w.state = take((size_t)n_utt * 4 * N * 4);  // token states + their packed arc ranges
  w.cost = take((size_t)n_utt * 2 * N * 8);
  w.sta = take((size_t)n_utt * C * 4);
  w.stb = take((size_t)n_utt * C * 4);
  w.stkey = take((size_t)n_utt * C * 8);
  w.bp = take((size_t)total_frames * bpf * 8);
  w.tokoff = take((size_t)(total_frames + n_utt) * 4);
  w.hash = take((size_t)n_utt * 4);
  w.list = take((size_t)n_utt * 4);
  w.count = take(256);
  w.vstate = take((size_t)n_utt * sizeof(VitState));
  w.band = take((size_t)n_utt * 2 * 4);
  w.eps = take((size_t)eps_states * 4);
  w.total = o;
  return w;
}

}  // namespace

extern "C" {

MFA_API int mfa_debug_viterbi_stamps(mfa_ctx *c, void *d_stamps) {
  c->vit_stamps = d_stamps;
  return 0;
}

MFA_API int mfa_debug_viterbi_plan(const mfa_align_opts *o, int32_t max_states, int32_t max_arcs, int32_t eps, int32_t lazy,
                                   int32_t *h_out, int32_t cap) {
  return vplan::viterbi_plan_rows(o, max_states, max_arcs, eps != 0, lazy != 0, h_out, cap);
}

MFA_API size_t mfa_align_workspace_bytes(mfa_ctx *c, int32_t n_utt, int64_t total_frames, const mfa_align_opts *o) {
  (void)c;
  int N = (o->max_tokens > 0 ? o->max_tokens : 1024) * 4, C = 8 * N;
  return ws_layout(n_utt, total_frames, N, C, o->bp_tokens_per_frame > 0 ? o->bp_tokens_per_frame : 512,
                   (int64_t)n_utt * 8 * N).total;
}

}  // extern "C"

namespace {

// Shared driver of mfa_align_batch (scores given) and mfa_align_features_batch (lazy: `lazy` non-NULL — every pass is a
// loop over windows of `window` frames: score the cells the live tokens can reach, then decode the window).
int align_impl(mfa_ctx *c, const mfa_graph_batch *g, const float *d_loglikes, const int64_t *d_ll_off,
               const int32_t *d_ll_cols, const int64_t *d_frame_off, int64_t total_frames,
               int64_t total_arcs, int32_t max_states, int32_t max_arcs, const mfa_align_opts *o, int32_t *d_ali, int32_t *d_words, int32_t *d_n_words,
               float *d_like, float *d_frame_like, int32_t *d_status, const MfaLazyScoring *lazy) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  const int n_utt = g->n_utt;
  if (n_utt <= 0) return 0;
  if (o->beam <= 0.0f || (o->retry_beam != 0.0f && o->retry_beam <= o->beam))
    return c->fail("Beams do not make sense: beam %f, retry-beam %f", o->beam, o->retry_beam);
  if (max_states <= 0 || max_arcs <= 0) return c->fail("max_states and max_arcs must be positive");
  if (total_frames <= 0 || total_arcs <= 0) return c->fail("total_frames and total_arcs must be positive");
  if (max_arcs >= (1 << 25)) return c->fail("graphs with more than 2^25 arcs are not supported");
  const int bpf = o->bp_tokens_per_frame > 0 ? o->bp_tokens_per_frame : 512;
  const int passes = o->retry_beam != 0.0f ? 2 : 1;
  // graphs with epsilon input arcs: the decoder kernels' kEps instantiations, one {first epsilon arc, count} word per state
  // in the workspace
  const bool eps = g->d_state_nemit != nullptr;
  if (eps && max_arcs >= (1 << 24)) return c->fail("graphs with epsilon arcs and more than 2^24 arcs are not supported");
  const int64_t eps_states = eps ? (int64_t)n_utt * max_states : 0;
  // the launch plan (viterbi_plan.hpp): capacities per pass, then per launch the LDS carve, where the token lists live, the
  // state→slot table
  vplan::Plan plan = vplan::viterbi_plan(o, max_states, max_arcs, eps, lazy != nullptr);
  if (plan.refused >= 0) {
    const vplan::Launch &L = plan.l[plan.refused];
    return c->fail("Viterbi tables need %zu bytes of LDS (> 160 KiB): %d states, %d tokens", L.lds, max_states, L.N);
  }
  const int Nw = passes == 2 ? plan.N[1] : plan.N[0], Cw = passes == 2 ? plan.C[1] : plan.C[0];
  WsLayout w = ws_layout(n_utt, total_frames, Nw, Cw, bpf, total_arcs, eps_states);
  if (c->d_ws.reserve(c, w.total, "the decoder workspace")) return -1;
  unsigned char *base = c->d_ws.ptr<unsigned char>();
  hipLaunchKernelGGL(arcnext_kernel, dim3(n_utt), dim3(256), 0, c->stream, *g, (uint4 *)(base + w.arcnext),
                     eps ? (u32 *)(base + w.eps) : (u32 *)nullptr, max_states);
  // Launch plan.  The decoder is latency-bound (one wavefront walks one utterance frame by frame), so throughput is the
  // number of wavefronts a CU can keep resident, and that is set by the LDS tables, which scale with the token capacity.
  // With the normal beam a frame rarely holds more than a few dozen tokens, so every utterance is first decoded with
  // small tables (the first tier); the few that overflow them are marked ST_GROW and decoded again, from scratch and with
  // the same beam, at the caller's full capacity.  Then the retry-beam pass for utterances that did not reach a final state.
  if (lazy && mfa_gmm_presplit(c, lazy, g, d_frame_off, n_utt, total_frames) != 0) return -1;
  // Speculative look-ahead of the windowed first tier.  The proven band lets a token advance one arc per frame, K − 1
  // arcs by the window's last frame; speech advances a third of that (synthetic 10 s utterances: 21 states per 64 frames on
  // average, 34 at the 99th percentile, 38 at most).  The window is scored for a look-ahead of K / 2 arcs instead (32 for
  // K = 64: a fifth fewer model blocks gathered than with 48, tools/band_study.py), the decoder checks every score it reads
  // against what was scored, and a window in which it asks for more (about 1 % of them) is scored again with the proven band
  // and redone from the state parked at its start by the first tier, one window later (lag mode, see the window loop);
  // results cannot differ.  (Round 2 re-decoded such an utterance from frame 0, which made anything below 48 arcs a loss.)
  // MFA_LAZY_LOOKAHEAD=n overrides (n >= K − 1: off).
  int spec_slack = 0;
  if (lazy) {
    int look = lazy->window / 2;
    { const char *e = getenv("MFA_LAZY_LOOKAHEAD"); if (e && atoi(e) > 0) look = atoi(e); }
    spec_slack = std::max(0, lazy->window - 1 - look);
    if (lazy->plan.max_cols > 32 * kBmWords) spec_slack = 0;   // (the decoder's bitmap of scored columns holds 2 048)
  }
  int eps_pops_env = 0;                  // MFA_VIT_EPS_POPS (tests: forces the hand-over to the general decoder)
  { const char *e = getenv("MFA_VIT_EPS_POPS"); if (e && atoi(e) > 0) eps_pops_env = atoi(e); }
  for (int li = 0; li < plan.n; li++) {
    const vplan::Launch &L = plan.l[li];
    const int ps = L.pass;
    // the windowed first tier of the lazy path: viterbi_small_kernel, then viterbi_finish_kernel
    const bool small_tier = lazy && L.grow;
    const bool lists_in_lds = L.lists_in_lds;
    const size_t lds = L.lds;
    VitParams p;
    memset(&p, 0, sizeof(p));
    p.g = *g; p.ll = d_loglikes; p.ll_off = d_ll_off; p.ll_cols = d_ll_cols; p.frame_off = d_frame_off;
    p.beam = ps == 0 ? o->beam : o->retry_beam; p.scale = o->acoustic_scale;
    p.nmax = L.N; p.cmax = L.C; p.bpf = bpf; p.pass = ps; p.grow = L.grow; p.hbits = L.hbits;
    // workspace strides follow this launch's capacities (lists, parked lists and stash are per-launch scratch; the
    // largest launch's fits in `w`)
    WsLayout wp = ws_layout(n_utt, total_frames, L.N, L.C, bpf, total_arcs, eps_states);
    p.w_state = (u32 *)(base + wp.state); p.w_cost = (double *)(base + wp.cost);
    p.w_stash_a = (u32 *)(base + wp.sta); p.w_stash_b = (u32 *)(base + wp.stb); p.w_stash_key = (u64 *)(base + wp.stkey);
    p.w_bp = (u64 *)(base + wp.bp); p.w_tokoff = (u32 *)(base + wp.tokoff);
    p.w_hash = (u32 *)(base + w.hash);     // fixed location across launches
    p.w_arcnext = (const uint4 *)(base + w.arcnext);
    p.w_epsinfo = eps ? (const u32 *)(base + w.eps) : nullptr; p.eps_stride = max_states;
    p.eps_pops = eps_pops_env ? eps_pops_env : 64 * L.N;
    p.llcap = kLlCap;
    p.stamps = (unsigned long long *)c->vit_stamps;
    p.utt_list = nullptr; p.n_list = nullptr;
    p.ali = d_ali; p.words = d_words; p.n_words = d_n_words; p.like = d_like; p.frame_like = d_frame_like; p.status = d_status;
    if (L.code != 0) {
      int32_t *d_list = (int32_t *)(base + w.list), *d_count = (int32_t *)(base + w.count);
      MFA_HIP_CHECK(c, hipMemsetAsync(d_count, 0, sizeof(int32_t), c->stream));
      hipLaunchKernelGGL(collect_pending_kernel, dim3((n_utt + 255) / 256), dim3(256), 0, c->stream, d_status, n_utt, L.code, d_list, d_count);
      p.utt_list = d_list; p.n_list = d_count;
    }
    p.windowed = 0; p.t_begin = 0; p.t_end = 0x7fffffff; p.next_window = 0;
    p.w_vstate = (VitState *)(base + w.vstate); p.state_depth = nullptr; p.band = nullptr;
    // four instantiations: token lists in LDS or HBM × epsilon-free or not
    void (*k_lds)(VitParams) = eps ? viterbi_kernel<true, true> : viterbi_kernel<true, false>;
    void (*k_hbm)(VitParams) = eps ? viterbi_kernel<false, true> : viterbi_kernel<false, false>;
    MFA_HIP_CHECK(c, hipFuncSetAttribute((const void *)(lists_in_lds ? k_lds : k_hbm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto launch_decoder = [&]() {
      KernelTimer kt(c, MFA_K_VITERBI);
      if (lists_in_lds) hipLaunchKernelGGL(k_lds, dim3(n_utt), dim3(64), lds, c->stream, p);
      else hipLaunchKernelGGL(k_hbm, dim3(n_utt), dim3(64), lds, c->stream, p);
    };
    if (!lazy) {
      launch_decoder();
      MFA_DEBUG_POINT(c, "decoded pass=%d code=%d N=%d C=%d lds=%zu in_lds=%d", ps, L.code, L.N, L.C, lds, (int)lists_in_lds);
    } else {
      // The rare passes (table growth, retry beam) keep far more of the graph alive, so a narrow band buys little there:
      // they take wide windows and few launches.
      const int K = L.code == 0 ? lazy->window : std::max(lazy->window, 256);
      p.windowed = 1; p.next_window = K;
      p.state_depth = lazy->plan.d_state_depth; p.band = (int32_t *)(base + w.band);
      // Lag mode (the first tier): an utterance whose speculative window failed is not handed to a larger tier — a launch
      // that a handful of wavefronts can use, one workgroup with up to 100 KB of LDS per utterance of the batch to find them
      // — but falls one window behind: the next scoring launch scores the failed window again for it, with the proven band,
      // the next first-tier launch redoes it, and so on to the end, where one extra round of launches finishes the
      // stragglers.  Capacity overflows wait for the from-scratch list pass.  Only the first tier speculates.
      const bool spec = small_tier && spec_slack > 0;
      const int t_loop_end = lazy->max_frames + (small_tier ? K : 0);
      constexpr int kSmallRounds = 3;
      const size_t lds_small = SmallLds<size_t>(0, kSmallN, 64 * kSmallRounds, eps).end;
      for (int t0 = 0; t0 < t_loop_end; t0 += K) {
        MfaWindowScore ws;
        memset(&ws, 0, sizeof(ws));
        if (small_tier) { ws.lag = (const int32_t *)(base + w.vstate); ws.lag_stride = (int)(sizeof(VitState) / 4); ws.lag_word = 3; }
        ws.t_begin = t0; ws.window = K; ws.band = p.band; ws.utt_list = p.utt_list; ws.n_list = p.n_list;
        ws.cols_per_wave = L.code == 0 ? 0 : 32;   // list passes: few utterances, wide bands — spread the columns over wavefronts
        ws.hi_slack = spec ? spec_slack : 0;
        ws.done = (const int32_t *)(base + w.vstate); ws.done_stride = (int)(sizeof(VitState) / 4); ws.done_word = 2;
        if (mfa_gmm_score_window(c, lazy, &ws, d_frame_off, n_utt, d_ll_off, (float *)d_loglikes) != 0) return -1;
        MFA_DEBUG_POINT(c, "scored window t0=%d K=%d pass=%d code=%d N=%d C=%d", t0, K, ps, L.code, L.N, L.C);
        p.t_begin = t0; p.t_end = t0 + K;
        p.spec = spec ? 1 : 0; p.spec_ranges = mfa_band_ranges(c); p.spec_class_counts = lazy->plan.d_class_counts;
        p.spec_groups = lazy->plan.groups;
        if (small_tier) {
          KernelTimer kt(c, MFA_K_VITERBI);
          if (eps) hipLaunchKernelGGL((viterbi_small_kernel<kSmallRounds, true>), dim3(n_utt), dim3(64), lds_small, c->stream, p);
          else hipLaunchKernelGGL((viterbi_small_kernel<kSmallRounds, false>), dim3(n_utt), dim3(64), lds_small, c->stream, p);
        } else {
          launch_decoder();
        }
        MFA_DEBUG_POINT(c, "decoded window t0=%d K=%d pass=%d code=%d N=%d C=%d lds=%zu in_lds=%d small=%d", t0, K, ps, L.code, L.N, L.C, lds,
                        (int)lists_in_lds, (int)small_tier);
      }
      if (small_tier) {   // utterances the first tier decoded to their last frame: ReachedFinal, traceback, outputs
        KernelTimer kt(c, MFA_K_VITERBI);
        hipLaunchKernelGGL(viterbi_finish_kernel, dim3(n_utt), dim3(64), 0, c->stream, p);
      }
    }
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  c->xsplit_ready = false;
  hipLaunchKernelGGL(finalize_pending_kernel, dim3((n_utt + 255) / 256), dim3(256), 0, c->stream, d_status, n_utt);
  MFA_HIP_CHECK(c, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

MFA_API int mfa_align_batch(mfa_ctx *c, const mfa_graph_batch *g, const float *d_loglikes, const int64_t *d_ll_off,
                            const int32_t *d_ll_cols, const int64_t *d_frame_off, int64_t total_frames,
                            int64_t total_arcs, int32_t max_states, int32_t max_arcs, const mfa_align_opts *o, int32_t *d_ali, int32_t *d_words, int32_t *d_n_words,
                            float *d_like, float *d_frame_like, int32_t *d_status) {
  return align_impl(c, g, d_loglikes, d_ll_off, d_ll_cols, d_frame_off, total_frames, total_arcs, max_states, max_arcs, o,
                    d_ali, d_words, d_n_words, d_like, d_frame_like, d_status, nullptr);
}

MFA_API int mfa_align_features_batch(mfa_ctx *c, const mfa_graph_batch *g, const mfa_score_plan *plan, const float *d_feats,
                                     const int64_t *d_frame_off, int32_t max_frames, int64_t total_frames, int64_t total_arcs,
                                     int32_t max_states, int32_t max_arcs, const mfa_align_opts *o, int32_t window,
                                     float *d_loglikes, const int64_t *d_ll_off, const int32_t *d_ll_cols, int32_t *d_ali,
                                     int32_t *d_words, int32_t *d_n_words, float *d_like, float *d_frame_like,
                                     int32_t *d_status) {
  if (!plan || !plan->d_pdf_list || !plan->d_pdf_off || !plan->d_class_counts || !plan->d_pdf_first_frame ||
      !plan->d_pdf_last_depth || !plan->d_state_depth)
    return c->fail("mfa_align_features_batch: incomplete score plan");
  if (window <= 0 || window % 64 != 0) return c->fail("mfa_align_features_batch: window must be a positive multiple of 64 frames (got %d)", window);
  if (max_frames <= 0) return c->fail("mfa_align_features_batch: max_frames must be positive");
  if (!mfa_gmm_lazy_supported(c)) {
    // feature dimensions beyond the MFMA kernels' instantiations: dense scoring (naive kernel), then the decoder
    if (mfa_gmm_score_batch(c, d_feats, d_frame_off, g->n_utt, max_frames, plan->d_pdf_list, plan->d_pdf_off,
                            plan->d_class_counts, plan->d_pdf_first_frame, d_ll_off, d_loglikes) != 0) return -1;
    return align_impl(c, g, d_loglikes, d_ll_off, d_ll_cols, d_frame_off, total_frames, total_arcs, max_states, max_arcs, o,
                      d_ali, d_words, d_n_words, d_like, d_frame_like, d_status, nullptr);
  }
  if (plan->max_cols <= 0) return c->fail("mfa_align_features_batch: plan.max_cols must be the largest column count of the batch");
  MfaLazyScoring lazy;
  lazy.plan = *plan; lazy.d_feats = d_feats; lazy.max_frames = max_frames; lazy.window = window;
  return align_impl(c, g, d_loglikes, d_ll_off, d_ll_cols, d_frame_off, total_frames, total_arcs, max_states, max_arcs, o,
                    d_ali, d_words, d_n_words, d_like, d_frame_like, d_status, &lazy);
}

}  // extern "C"
