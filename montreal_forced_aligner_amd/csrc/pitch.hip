// Pitch and voicing features for gfx950: Kaldi's ComputeKaldiPitch (offline) + ProcessPitch restated (include/mfa_hip.h has
// the algorithm; pitch_plan.cpp the host tables).  Three kernels:
//
//  pitch_resample_kernel   int16 at sample_frequency → float32 at resample_frequency, one thread per output sample:
//                          acc = fmaf(w_j, (float)x_j, acc) over the phase's taps in ascending order from 0.0f, taps outside
//                          the utterance skipped (a skipped tap is fmaf(w, 0, acc) = acc).
//  pitch_track_kernel      one workgroup per utterance, frame by frame — the tracker is serial in t and wide in states:
//                          window → NCCF at the measured lags → up-sampling onto the states → forward step, with the
//                          window, the NCCFs and both fwd vectors in LDS; back-pointers uint16 [T][S] and the POV NCCF at
//                          the measured lags [T][L] go to the workspace; thread 0 then traces back (the POV value of the
//                          chosen state is the same fmaf chain over the stored row).
//  pitch_process_kernel    ProcessPitch, one thread per frame: every frame re-evaluates the POV weights of its ±context
//                          neighbours (151 × a few transcendental calls — cheaper than a scratch array and a second pass)
//                          and sums them in double in ascending frame order.
//
// Exact arithmetic of the tracker (a float32 numpy restatement is bit-identical; the file is compiled with
// -ffp-contract=off; sums, products and quotients are spelled with the _rn intrinsics, the square root is sqrtf, which the
// compiler's default -fhip-fp32-correctly-rounded-divide-sqrt keeps IEEE):
//   mean      = (x_0 + x_1 + … + x_{N-1}) / N, float32 adds in ascending order from 0.0f; w_k = x_k − mean
//   e_l       = Σ_{k<N} w_{k+l}², inner_l = Σ_{k<N} w_k w_{k+l}: fmaf chains over ascending k from 0.0f; e_0 likewise
//   nccf      = inner_l / sqrtf(e_0 · e_l + ballast), 0 where the square root is 0; ballast = (float)((ms · N)² · nccf_ballast)
//               in double, ms = Σx²/n in double over the resampled signal: 256 partial sums (sample k goes to partial k mod
//               256, ascending k) added in ascending order
//   up-sample = Σ_j fmaf(W_ij, nccf_{first_i + j}, acc) over ascending j from 0.0f
//   local_i   = fmaf(sml_i, n_i, 1.0f − n_i)
//   fwd_t[i]  = (min_j (prev[j] + pen[|i − j|])) + local_i, candidates compared with strict < in ascending j (ties: smallest j),
//               pen[d] = c · (float)(d²) one float32 product (host table); then fwd_t −= min_i fwd_t[i]
//   pitch     = 1.0f / lag_state
// Nothing here depends on another workgroup's progress.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "ctx.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kRsPerBlock = 1024;   // resampled samples of one utterance per workgroup of pitch_resample_kernel

struct PitchParams {
  int S, L, first_lag, N, W, shift, snip, up_max_taps;
  int O, I, rs_max_taps;
  float nccf_ballast;
  const float *lags, *sml, *pen, *up_w, *rs_w;
  const int32_t *up_first, *up_taps, *rs_first, *rs_taps;
  // ProcessPitch
  float pov_scale, pov_offset, pitch_scale;
  int norm_ctx, add_pov, add_norm, add_raw;
};

// where a sub-launch keeps utterance utt's resampled signal: slots of at least ⌈n·O/I⌉ floats, derived from the sample
// offsets alone (start_{u+1} − start_u ≥ ⌊n_u·O/I⌋ + 1 ≥ the utterance's resampled length)
__host__ __device__ inline int64_t rs_slot(int64_t samples_before, int utts_before, int O, int I) {
  return samples_before * O / I + utts_before;
}
__host__ __device__ inline int64_t rs_count(int64_t n, int O, int I) {   // mfa_resample_num_samples
  if (n <= 0) return 0;
  const int64_t len = n * O;
  int64_t last = len / I;
  if (last * I == len) last -= 1;
  return last + 1;
}

__global__ __launch_bounds__(kThreads) void pitch_resample_kernel(PitchParams p, const int16_t *__restrict__ pcm,
                                                                   const int64_t *__restrict__ sample_off, int u0,
                                                                   float *__restrict__ ws_rs, float *__restrict__ dbg_rs,
                                                                   const int64_t *__restrict__ dbg_rs_off) {
  const int utt = u0 + blockIdx.y;
  const int64_t i0 = sample_off[utt], n = sample_off[utt + 1] - i0;
  const int64_t n_out = rs_count(n, p.O, p.I);
  float *y = ws_rs + rs_slot(i0 - sample_off[u0], utt - u0, p.O, p.I);
  const int16_t *x = pcm + i0;
  for (int c = 0; c < kRsPerBlock / kThreads; c++) {
    const int64_t k = (int64_t)blockIdx.x * kRsPerBlock + c * kThreads + threadIdx.x;
    if (k >= n_out) return;
    const int64_t u = k / p.O;
    const int i = (int)(k - u * p.O);
    const int64_t lo = u * p.I + p.rs_first[i];
    const float *w = p.rs_w + (size_t)i * p.rs_max_taps;
    const int taps = p.rs_taps[i];
    float acc = 0.0f;
    for (int j = 0; j < taps; j++) {
      const int64_t idx = lo + j;
      if (idx >= 0 && idx < n) acc = fmaf(w[j], (float)x[idx], acc);
    }
    y[k] = acc;
    if (dbg_rs) dbg_rs[dbg_rs_off[utt] + k] = acc;
  }
}

__global__ __launch_bounds__(kThreads) void pitch_track_kernel(PitchParams p, const int64_t *__restrict__ sample_off,
                                                                const int64_t *__restrict__ frame_off, int u0,
                                                                const float *__restrict__ ws_rs, float *__restrict__ ws_pov,
                                                                uint16_t *__restrict__ ws_bp, float *__restrict__ raw,
                                                                float *__restrict__ dbg_np, float *__restrict__ dbg_nv,
                                                                int32_t *__restrict__ dbg_path) {
  extern __shared__ float s_mem[];
  const int S = p.S, L = p.L, N = p.N, W = p.W;
  float *fwd_a = s_mem, *fwd_b = fwd_a + S, *loc = fwd_b + S, *pen = loc + S;   // [S] each
  float *xw = pen + S, *w = xw + W;                              // [W] raw and zero-mean window
  float *s_inner = w + W, *s_en = s_inner + L;                   // [L] inner products and energies of the lagged windows
  float *s_np = s_en + L, *s_nv = s_np + L;                      // [L] pitch and POV NCCF at the measured lags
  float *s_red = s_nv + L;                                       // [kThreads / 64 + 2]: wave minima, e_0
  __shared__ double s_part[kThreads];
  __shared__ float s_ballast;
  const int tid = threadIdx.x;
  const int utt = u0 + blockIdx.x;
  const int64_t i0 = sample_off[utt], n_in = sample_off[utt + 1] - i0;
  const int64_t n = rs_count(n_in, p.O, p.I);
  const int64_t f0 = frame_off[utt];
  const int T = (int)(frame_off[utt + 1] - f0);
  if (T <= 0) return;   // whole workgroup
  const float *x = ws_rs + rs_slot(i0 - sample_off[u0], utt - u0, p.O, p.I);
  const int64_t fg = f0 - frame_off[u0];   // first frame of the utterance inside the sub-launch's workspace
  float *pov = ws_pov + fg * L;
  uint16_t *bp = ws_bp + fg * S;

  // ballast from the utterance's mean square
  {
    double acc = 0.0;
    for (int64_t k = tid; k < n; k += kThreads) { const double v = (double)x[k]; acc += v * v; }
    s_part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
      double sum = 0.0;
      for (int k = 0; k < kThreads; k++) sum += s_part[k];
      const double b = sum / (double)n * (double)N;
      s_ballast = (float)(b * b * (double)p.nccf_ballast);
    }
  }
  for (int i = tid; i < S; i += kThreads) { fwd_a[i] = 0.0f; pen[i] = p.pen[i]; }
  __syncthreads();
  const float ballast = s_ballast;
  float *prev = fwd_a, *cur = fwd_b;

  for (int t = 0; t < T; t++) {
    const int64_t start = p.snip ? (int64_t)t * p.shift : (int64_t)t * p.shift + p.shift / 2 - N / 2;
    for (int k = tid; k < W; k += kThreads) {
      const int64_t idx = start + k;
      xw[k] = (idx >= 0 && idx < n) ? x[idx] : 0.0f;
    }
    __syncthreads();
    {
      float sum = 0.0f;   // every thread forms the same mean (LDS broadcasts): no barrier, no divergence in the result
      for (int k = 0; k < N; k++) sum = __fadd_rn(sum, xw[k]);
      const float mean = __fdiv_rn(sum, (float)N);
      for (int k = tid; k < W; k += kThreads) w[k] = __fsub_rn(xw[k], mean);
    }
    __syncthreads();
    // items 0 .. L-1: inner products; L .. 2L-1: energies of the lagged windows; 2L: e_0
    for (int q = tid; q <= 2 * L; q += kThreads) {
      float acc = 0.0f;
      if (q < L) {
        const float *b = w + p.first_lag + q;
        for (int k = 0; k < N; k++) acc = fmaf(w[k], b[k], acc);
        s_inner[q] = acc;
      } else {
        const float *b = q < 2 * L ? w + p.first_lag + (q - L) : w;
        for (int k = 0; k < N; k++) acc = fmaf(b[k], b[k], acc);
        if (q < 2 * L) s_en[q - L] = acc; else s_red[kThreads / 64] = acc;
      }
    }
    __syncthreads();
    {
      const float e0 = s_red[kThreads / 64];
      for (int l = tid; l < L; l += kThreads) {
        const float norm = __fmul_rn(e0, s_en[l]), inner = s_inner[l];
        const float dp = sqrtf(__fadd_rn(norm, ballast)), dv = sqrtf(norm);   // (IEEE: __fsqrt_rn is the native approximation here)
        const float a = dp != 0.0f ? __fdiv_rn(inner, dp) : 0.0f, b = dv != 0.0f ? __fdiv_rn(inner, dv) : 0.0f;
        s_np[l] = a; s_nv[l] = b;
        pov[(int64_t)t * L + l] = b;
      }
    }
    __syncthreads();
    for (int i = tid; i < S; i += kThreads) {
      const float *wv = p.up_w + (size_t)i * p.up_max_taps;
      const int lo = p.up_first[i], taps = p.up_taps[i];
      float a = 0.0f;
      for (int j = 0; j < taps; j++) a = fmaf(wv[j], s_np[lo + j], a);
      loc[i] = fmaf(p.sml[i], a, __fsub_rn(1.0f, a));
      if (dbg_np) {
        float b = 0.0f;
        for (int j = 0; j < taps; j++) b = fmaf(wv[j], s_nv[lo + j], b);
        dbg_np[(f0 + t) * S + i] = a;
        dbg_nv[(f0 + t) * S + i] = b;
      }
    }
    // forward step (loc of a state is read by the thread that wrote it)
    float lmin = __builtin_inff();
    for (int i = tid; i < S; i += kThreads) {
      float best = __fadd_rn(prev[0], pen[i]);
      int arg = 0;
      for (int j = 1; j <= i; j++) {
        const float cand = __fadd_rn(prev[j], pen[i - j]);
        if (cand < best) { best = cand; arg = j; }
      }
      for (int j = i + 1; j < S; j++) {
        const float cand = __fadd_rn(prev[j], pen[j - i]);
        if (cand < best) { best = cand; arg = j; }
      }
      const float v = __fadd_rn(best, loc[i]);
      cur[i] = v;
      bp[(int64_t)t * S + i] = (uint16_t)arg;
      lmin = fminf(lmin, v);
    }
    for (int o = 32; o > 0; o >>= 1) lmin = fminf(lmin, __shfl_xor(lmin, o));
    if ((tid & 63) == 0) s_red[tid >> 6] = lmin;
    __syncthreads();
    float fmin_ = s_red[0];
    for (int k = 1; k < kThreads / 64; k++) fmin_ = fminf(fmin_, s_red[k]);
    for (int i = tid; i < S; i += kThreads) cur[i] = __fsub_rn(cur[i], fmin_);
    __syncthreads();   // cur complete before the next frame reads it as prev; s_red and the window free again
    float *tmp = prev; prev = cur; cur = tmp;
  }
  // trace back (the barrier above made every back-pointer and POV row of this workgroup visible to thread 0)
  if (tid != 0) return;
  int state = 0;
  {
    float best = prev[0];
    for (int i = 1; i < S; i++) if (prev[i] < best) { best = prev[i]; state = i; }
  }
  for (int t = T - 1; t >= 0; t--) {
    const float *wv = p.up_w + (size_t)state * p.up_max_taps;
    const float *row = pov + (int64_t)t * L + p.up_first[state];
    const int taps = p.up_taps[state];
    float b = 0.0f;
    for (int j = 0; j < taps; j++) b = fmaf(wv[j], row[j], b);
    raw[(f0 + t) * 2] = b;
    raw[(f0 + t) * 2 + 1] = __fdiv_rn(1.0f, p.lags[state]);
    if (dbg_path) dbg_path[f0 + t] = state;
    state = bp[(int64_t)t * S + state];
  }
}

__device__ inline float pov_weight(float nccf) {
  const float a = fminf(fabsf(nccf), 1.0f);
  const float r = -5.2f + 5.4f * expf(7.5f * (a - 1.0f)) + 4.8f * a - 2.0f * expf(-10.0f * a) + 4.2f * expf(20.0f * (a - 1.0f));
  return 1.0f / (1.0f + expf(-r));
}

__global__ __launch_bounds__(kThreads) void pitch_process_kernel(PitchParams p, const float *__restrict__ raw,
                                                                  const int64_t *__restrict__ frame_off, float *__restrict__ out,
                                                                  int out_stride, int out_col0) {
  const int utt = blockIdx.y;
  const int64_t f0 = frame_off[utt];
  const int T = (int)(frame_off[utt + 1] - f0);
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const float *r = raw + f0 * 2;
  float *o = out + (f0 + t) * (int64_t)out_stride + out_col0;
  const float nccf = r[2 * t], logf_t = logf(r[2 * t + 1]);
  if (p.add_pov) {
    const float c = fminf(fmaxf(nccf, -1.0f), 1.0f);
    *o++ = p.pov_scale * (powf(1.0001f - c, 0.15f) - 1.0f) + p.pov_offset;
  }
  if (p.add_norm) {
    const int lo = max(0, t - p.norm_ctx), hi = min(T - 1, t + p.norm_ctx);
    double num = 0.0, den = 0.0;
    for (int s = lo; s <= hi; s++) {
      const float pw = pov_weight(r[2 * s]);
      num += (double)pw * (double)logf(r[2 * s + 1]);
      den += (double)pw;
    }
    *o++ = p.pitch_scale * (logf_t - (float)(num / den));
  }
  if (p.add_raw) *o++ = logf_t;
}

// ---- host side -----------------------------------------------------------------------------------------------------

size_t track_lds_bytes(const MfaPitchHostPlan &h) {
  return ((size_t)4 * h.n_states + 2 * (size_t)(h.n_win + h.last_lag) + 4 * (size_t)h.n_lags + kThreads / 64 + 2) * sizeof(float);
}

size_t budget_bytes() {
  const char *e = getenv("MFA_PITCH_WORKSPACE_MB");
  const double mb = e ? atof(e) : 0.0;   // fractions are taken (tests force a handful of utterances per sub-launch)
  return mb > 0.0 && mb < 1.0e9 ? (size_t)(mb * 1048576.0) : (size_t)2 << 30;
}

// bytes of one sub-launch's workspace: utterances [u0, u1) with `samples` input samples and `frames` frames in all
struct WsLayout { size_t rs_floats, pov_floats, bp_off, bytes; };
WsLayout ws_layout(const MfaPitchHostPlan &h, int n_utt, int64_t samples, int64_t frames) {
  WsLayout l;
  l.rs_floats = (size_t)rs_slot(samples, n_utt, h.rs.phases, h.rs.in_per_unit) + 1;
  l.pov_floats = (size_t)frames * h.n_lags;
  l.bp_off = (l.rs_floats + l.pov_floats) * sizeof(float);
  l.bytes = l.bp_off + (size_t)frames * h.n_states * sizeof(uint16_t);
  return l;
}

PitchParams params_of(mfa_ctx *c) {
  const MfaPitchHostPlan &h = c->pitch;
  PitchParams p;
  p.S = h.n_states; p.L = h.n_lags; p.first_lag = h.first_lag; p.N = h.n_win; p.W = h.n_win + h.last_lag; p.shift = h.shift;
  p.snip = h.o.snip_edges != 0; p.up_max_taps = h.up_max_taps;
  p.O = h.rs.phases; p.I = h.rs.in_per_unit; p.rs_max_taps = h.rs.max_taps;
  p.nccf_ballast = h.o.nccf_ballast;
  const size_t S = h.n_states;
  p.lags = c->d_pitch_f.ptr<float>(); p.sml = p.lags + S; p.pen = p.sml + S; p.up_w = p.pen + S; p.rs_w = p.up_w + S * h.up_max_taps;
  p.up_first = c->d_pitch_i.ptr<int32_t>(); p.up_taps = p.up_first + S; p.rs_first = p.up_taps + S; p.rs_taps = p.rs_first + h.rs.phases;
  p.pov_scale = h.o.pov_scale; p.pov_offset = h.o.pov_offset; p.pitch_scale = h.o.pitch_scale;
  p.norm_ctx = h.o.normalization_context;
  p.add_pov = h.o.add_pov_feature != 0; p.add_norm = h.o.add_normalized_log_pitch != 0; p.add_raw = h.o.add_raw_log_pitch != 0;
  return p;
}

struct PitchDebug { float *rs = nullptr; const int64_t *rs_off = nullptr; float *np = nullptr, *nv = nullptr; int32_t *path = nullptr; };

int track_batch(mfa_ctx *c, const int16_t *d_pcm, const int64_t *d_sample_off, const int64_t *d_frame_off,
                const int64_t *h_sample_off, const int64_t *h_frame_off, int32_t n_utt, float *d_raw, const PitchDebug *dbg) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (!c->pitch_ready) return c->fail("mfa_pitch_configure has not been called");
  if (n_utt < 0) return c->fail("pitch: negative utterance count");
  if (n_utt == 0) return 0;
  if (!d_pcm || !d_sample_off || !d_frame_off || !h_sample_off || !h_frame_off || !d_raw) return c->fail("pitch: NULL argument");
  const MfaPitchHostPlan &h = c->pitch;
  for (int u = 0; u < n_utt; u++) {
    const int64_t n = h_sample_off[u + 1] - h_sample_off[u], T = h_frame_off[u + 1] - h_frame_off[u];
    if (n < 0 || T < 0) return c->fail("pitch: offsets of utterance %d decrease", u);
    if (T != mfa_pitch_host_num_frames(h, n))
      return c->fail("pitch: utterance %d is given %lld frames, its %lld samples have %lld", u, (long long)T, (long long)n,
                     (long long)mfa_pitch_host_num_frames(h, n));
  }
  const PitchParams p = params_of(c);
  const size_t lds = track_lds_bytes(h);
  const size_t budget = dbg ? (size_t)-1 : budget_bytes();
  // sub-launches: always one utterance, then as many more as fit the budget; the workspace is sized once, for the largest
  std::vector<int> cuts(1, 0);
  size_t need = 0;
  for (int u0 = 0; u0 < n_utt;) {
    int u1 = u0 + 1;
    while (u1 < n_utt && u1 - u0 < 65535 &&
           ws_layout(h, u1 + 1 - u0, h_sample_off[u1 + 1] - h_sample_off[u0], h_frame_off[u1 + 1] - h_frame_off[u0]).bytes <= budget)
      u1++;
    need = std::max(need, ws_layout(h, u1 - u0, h_sample_off[u1] - h_sample_off[u0], h_frame_off[u1] - h_frame_off[u0]).bytes);
    cuts.push_back(u1);
    u0 = u1;
  }
  if (c->d_pitch_ws.reserve(c, need, "the pitch workspace")) return -1;
  KernelTimer kt(c, MFA_K_PITCH);
  for (size_t g = 0; g + 1 < cuts.size(); g++) {
    const int u0 = cuts[g], u1 = cuts[g + 1];
    const WsLayout l = ws_layout(h, u1 - u0, h_sample_off[u1] - h_sample_off[u0], h_frame_off[u1] - h_frame_off[u0]);
    int64_t max_rs = 0;
    for (int u = u0; u < u1; u++) max_rs = std::max(max_rs, rs_count(h_sample_off[u + 1] - h_sample_off[u], p.O, p.I));
    float *ws_rs = c->d_pitch_ws.ptr<float>(), *ws_pov = ws_rs + l.rs_floats;
    uint16_t *ws_bp = (uint16_t *)(c->d_pitch_ws.ptr<char>() + l.bp_off);
    const int64_t blocks = (max_rs + kRsPerBlock - 1) / kRsPerBlock;
    if (blocks > 0x7FFFFFFF) return c->fail("pitch: %lld resampled samples in one utterance", (long long)max_rs);
    if (blocks > 0) {
      hipLaunchKernelGGL(pitch_resample_kernel, dim3((unsigned)blocks, (unsigned)(u1 - u0)), dim3(kThreads), 0, c->stream, p, d_pcm,
                         d_sample_off, u0, ws_rs, dbg ? dbg->rs : nullptr, dbg ? dbg->rs_off : nullptr);
      MFA_HIP_CHECK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(pitch_track_kernel, dim3((unsigned)(u1 - u0)), dim3(kThreads), lds, c->stream, p, d_sample_off, d_frame_off, u0,
                       ws_rs, ws_pov, ws_bp, d_raw, dbg ? dbg->np : nullptr, dbg ? dbg->nv : nullptr, dbg ? dbg->path : nullptr);
    MFA_HIP_CHECK(c, hipGetLastError());
    MFA_DEBUG_POINT(c, "pitch kernels, utterances %d .. %d", u0, u1 - 1);
  }
  return 0;
}

void copy_tables(const MfaPitchHostPlan &h, int32_t *h_sizes, float *h_lags, float *h_sml, float *h_pen, int32_t *h_up_first,
                 int32_t *h_up_taps, float *h_up_w) {
  if (h_sizes) {
    const int32_t s[8] = {h.n_states, h.first_lag, h.last_lag, h.up_max_taps, h.n_win, h.shift, h.rs.phases, h.rs.max_taps};
    std::copy(s, s + 8, h_sizes);
  }
  if (h_lags) std::copy(h.lags.begin(), h.lags.end(), h_lags);
  if (h_sml) std::copy(h.sml.begin(), h.sml.end(), h_sml);
  if (h_pen) std::copy(h.pen.begin(), h.pen.end(), h_pen);
  if (h_up_first) std::copy(h.up_first.begin(), h.up_first.end(), h_up_first);
  if (h_up_taps) std::copy(h.up_taps.begin(), h.up_taps.end(), h_up_taps);
  if (h_up_w) std::copy(h.up_w.begin(), h.up_w.end(), h_up_w);
}

}  // namespace

extern "C" {

MFA_API int mfa_pitch_configure(mfa_ctx *c, const mfa_pitch_opts *opts) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  MfaPitchHostPlan h;
  std::string err;
  if (mfa_pitch_host_plan(opts, &h, &err) != 0) return c->fail("%s", err.c_str());
  if (track_lds_bytes(h) > (size_t)(64 << 10) - 2304)   // the static part: 256 doubles and a float
    return c->fail("pitch: %d states, %d lags and a window of %d samples do not fit a workgroup's LDS", h.n_states, h.n_lags,
                   h.n_win + h.last_lag);
  // nothing is recorded before the tables are on the device: a refusal or a failed upload leaves the previous options in force
  std::vector<float> f;
  f.insert(f.end(), h.lags.begin(), h.lags.end());
  f.insert(f.end(), h.sml.begin(), h.sml.end());
  f.insert(f.end(), h.pen.begin(), h.pen.end());
  f.insert(f.end(), h.up_w.begin(), h.up_w.end());
  f.insert(f.end(), h.rs.weights.begin(), h.rs.weights.end());
  std::vector<int32_t> iv;
  iv.insert(iv.end(), h.up_first.begin(), h.up_first.end());
  iv.insert(iv.end(), h.up_taps.begin(), h.up_taps.end());
  iv.insert(iv.end(), h.rs.first.begin(), h.rs.first.end());
  iv.insert(iv.end(), h.rs.taps.begin(), h.rs.taps.end());
  return dev_upload_commit<MfaHipDev>(c, "the pitch tables",
                           {{&c->d_pitch_f, f.data(), f.size() * sizeof(float)}, {&c->d_pitch_i, iv.data(), iv.size() * sizeof(int32_t)}},
                           [&] { c->pitch = std::move(h); c->pitch_ready = true; });
}

MFA_API int32_t mfa_pitch_num_frames(mfa_ctx *c, int64_t num_samples) {
  if (!c->pitch_ready) { c->fail("mfa_pitch_configure has not been called"); return -1; }
  const int64_t t = mfa_pitch_host_num_frames(c->pitch, num_samples);
  if (t > 0x7FFFFFFF) { c->fail("pitch: %lld frames in one utterance", (long long)t); return -1; }
  return (int32_t)t;
}

MFA_API int32_t mfa_pitch_num_states(mfa_ctx *c) {
  if (!c->pitch_ready) { c->fail("mfa_pitch_configure has not been called"); return -1; }
  return c->pitch.n_states;
}

MFA_API int32_t mfa_pitch_num_columns(mfa_ctx *c) {
  if (!c->pitch_ready) { c->fail("mfa_pitch_configure has not been called"); return -1; }
  return c->pitch.n_cols;
}

MFA_API size_t mfa_pitch_workspace_bytes(mfa_ctx *c, int32_t n_utt, int64_t total_samples, int64_t total_frames,
                                         int64_t max_samples, int32_t max_frames) {
  if (!c->pitch_ready || n_utt <= 0 || total_samples < 0 || total_frames < 0 || max_samples < 0 || max_frames < 0) return 0;
  const size_t all = ws_layout(c->pitch, n_utt, total_samples, total_frames).bytes;
  const size_t one = ws_layout(c->pitch, 1, max_samples, max_frames).bytes;
  return std::max(one, std::min(all, budget_bytes()));
}

MFA_API int mfa_pitch_batch(mfa_ctx *c, const int16_t *d_pcm, const int64_t *d_sample_off, const int64_t *d_frame_off,
                            const int64_t *h_sample_off, const int64_t *h_frame_off, int32_t n_utt, int32_t max_frames,
                            float *d_raw) {
  (void)max_frames;
  return track_batch(c, d_pcm, d_sample_off, d_frame_off, h_sample_off, h_frame_off, n_utt, d_raw, nullptr);
}

MFA_API int mfa_pitch_process_batch(mfa_ctx *c, const float *d_raw, const int64_t *d_frame_off, int32_t n_utt, int32_t max_frames,
                                    float *d_out, int32_t out_stride, int32_t out_col0) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (!c->pitch_ready) return c->fail("mfa_pitch_configure has not been called");
  if (n_utt < 0 || max_frames < 0) return c->fail("pitch: negative utterance count or length");
  if (out_col0 < 0 || out_stride < out_col0 + c->pitch.n_cols)
    return c->fail("pitch: %d columns from column %d do not fit rows of %d", c->pitch.n_cols, out_col0, out_stride);
  if (n_utt > 65535) return c->fail("at most 65535 utterances per pitch launch (got %d)", n_utt);
  if (n_utt == 0 || max_frames == 0) return 0;
  if (!d_raw || !d_frame_off || !d_out) return c->fail("pitch: NULL argument");
  const PitchParams p = params_of(c);
  KernelTimer kt(c, MFA_K_PITCH);
  hipLaunchKernelGGL(pitch_process_kernel, dim3((unsigned)((max_frames + kThreads - 1) / kThreads), (unsigned)n_utt), dim3(kThreads), 0,
                     c->stream, p, d_raw, d_frame_off, d_out, out_stride, out_col0);
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "pitch_process_kernel, %d utterances", n_utt);
  return 0;
}

MFA_API int mfa_debug_pitch_stages(mfa_ctx *c, const mfa_pitch_opts *opts, int32_t *h_sizes, float *h_lags, float *h_soft_min_lag,
                                   float *h_penalty, int32_t *h_up_first, int32_t *h_up_taps, float *h_up_weights,
                                   const int16_t *d_pcm, const int64_t *d_sample_off, const int64_t *d_frame_off,
                                   const int64_t *h_sample_off, const int64_t *h_frame_off, int32_t n_utt, int32_t max_frames,
                                   float *d_resampled, const int64_t *d_rs_off, float *d_nccf_pitch, float *d_nccf_pov,
                                   int32_t *d_path, float *d_raw) {
  (void)max_frames;
  if (!c) {
    MfaPitchHostPlan h;
    if (mfa_pitch_host_plan(opts, &h, nullptr) != 0) return -1;
    copy_tables(h, h_sizes, h_lags, h_soft_min_lag, h_penalty, h_up_first, h_up_taps, h_up_weights);
    return 0;
  }
  if (!c->pitch_ready) return c->fail("mfa_pitch_configure has not been called");
  copy_tables(c->pitch, h_sizes, h_lags, h_soft_min_lag, h_penalty, h_up_first, h_up_taps, h_up_weights);
  if (!d_pcm) return 0;
  if ((d_resampled != nullptr) != (d_rs_off != nullptr) || (d_nccf_pitch != nullptr) != (d_nccf_pov != nullptr))
    return c->fail("pitch stages: d_resampled goes with d_rs_off, d_nccf_pitch with d_nccf_pov");
  PitchDebug dbg;
  dbg.rs = d_resampled; dbg.rs_off = d_rs_off; dbg.np = d_nccf_pitch; dbg.nv = d_nccf_pov; dbg.path = d_path;
  return track_batch(c, d_pcm, d_sample_off, d_frame_off, h_sample_off, h_frame_off, n_utt, d_raw, &dbg);
}

}  // extern "C"
