// Batched sample-rate conversion for gfx950, ahead of the MFCC: int16 at the file's rate → int16 at the model's rate.
// The filter is Kaldi's LinearResample (resample_plan.cpp holds the plan: one windowed-sinc filter per output phase).
//
// Arithmetic of one output sample, fixed by the interface: acc = 0.0f; acc = fmaf(w_j, (float)x_j, acc) over the taps in
// ascending order; rint to nearest-even; clamp to int16.  Taps outside the utterance are dropped — here they are staged
// as zeros and a row's padding carries zero weights: fmaf(w, 0, acc) and fmaf(0, x, acc) leave acc as it is, so the loop
// has one trip count for the whole launch — the longest row, rounded up to a multiple of four — and no branch; four taps'
// operands are read from LDS at a time ahead of their four dependent multiply-adds.
//
// Layout: a workgroup takes one utterance and kOutPerBlock consecutive outputs.  Output k sits at input position
// p_k = ⌊k·I/O⌋ (I inputs and O outputs per unit) and its taps lie in [p_k − back, p_k + fwd], two constants of the plan, so
// a run of C outputs from k0 reads the C·I/O + back + fwd inputs from p_k0 − back on: they are staged in LDS as floats
// (every input is read ≈ taps·O/I times; the conversion is paid once) by plain 2-byte loads, which no offset parity can
// misalign.  The block is cut into runs of C ("chunk") outputs when its whole span would not fit the LDS budget — extreme
// rate ratios only; at 48 kHz → 16 kHz the span of 1 024 outputs is 12 KB.
// The phase table (rows of `stride` = taps4 + 1 floats, odd: the 64 lanes of a wavefront read 64 different rows and an odd
// stride spreads them over the banks) is staged in LDS too when it fits beside the span in 64 KB — two workgroups per CU
// stay resident either way — and read from global memory (L2) otherwise: 3 200 phases at 12 345 Hz → 16 kHz.
#include <algorithm>

#include "ctx.hpp"
#include "resample_plan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kOutPerBlock = 1024;          // outputs of one utterance per workgroup (mfa_resample_block_outputs)
constexpr int kMaxSpanFloats = 5120;        // staged inputs of one run: 20 KB (the longest filter the rate limits admit has 4 655 taps)
constexpr size_t kMaxLdsBytes = 64 << 10;   // span + table, per workgroup

struct ResampleParams {
  int phases, in_per_unit;
  int taps4;       // the longest row's taps, rounded up to a multiple of 4: the trip count of every output
  int stride;      // floats per table row: taps4 + 1 (odd)
  int back;        // max over phases of ⌊i·I/O⌋ − lo_i
  int chunk;       // outputs per staged run (≤ kOutPerBlock)
  int span;        // staged inputs per run: ⌈(chunk − 1)·I/O⌉ + back + fwd + 2
  const int32_t *first;   // [phases] lo_i
  const float *w;         // [phases][stride], rows zero padded
};

template <bool kTableInLds>
__global__ __launch_bounds__(kThreads) void resample_kernel(ResampleParams p, const int16_t *__restrict__ in,
                                                             const int64_t *__restrict__ in_off, int16_t *__restrict__ out,
                                                             const int64_t *__restrict__ out_off,
                                                             const int32_t *__restrict__ utt_list) {
  extern __shared__ float s_mem[];
  float *xs = s_mem;                                      // [span]
  int32_t *s_first = (int32_t *)(s_mem + p.span);         // [phases]           (kTableInLds)
  float *s_w = s_mem + p.span + p.phases;                 // [phases][stride]   (kTableInLds)
  const int tid = threadIdx.x;
  const int utt = utt_list[blockIdx.y];
  const int64_t i0 = in_off[utt], n = in_off[utt + 1] - i0;
  const int64_t o0 = out_off[utt], n_out = out_off[utt + 1] - o0;
  const int64_t kb = (int64_t)blockIdx.x * kOutPerBlock;
  if (kb >= n_out) return;                                // whole workgroup: nothing to do (an empty utterance ends here)
  const int64_t kend = min(kb + (int64_t)kOutPerBlock, n_out);
  const int O = p.phases, I = p.in_per_unit;
  if (kTableInLds) {                                      // (the first barrier of the run loop orders these stores too)
    for (int k = tid; k < O; k += kThreads) s_first[k] = p.first[k];
    for (int k = tid; k < O * p.stride; k += kThreads) s_w[k] = p.w[k];
  }
  const int32_t *first = kTableInLds ? s_first : p.first;
  const float *wtab = kTableInLds ? s_w : p.w;
  const int16_t *x = in + i0;
  int16_t *y = out + o0;
  const int step_u = kThreads / O, step_i = kThreads % O;
  for (int64_t kc = kb; kc < kend; kc += p.chunk) {
    const int64_t base = kc * I / O - p.back;             // first staged input (kc·I ≥ 0: the division floors)
    __syncthreads();                                      // the previous run's reads are done
    for (int s = tid; s < p.span; s += kThreads) {
      const int64_t idx = base + s;
      xs[s] = (idx >= 0 && idx < n) ? (float)x[idx] : 0.0f;
    }
    __syncthreads();
    const int cn = (int)min((int64_t)p.chunk, kend - kc);
    if (tid >= cn) continue;
    const int64_t k = kc + tid;
    int64_t u = k / O;
    int i = (int)(k - u * O);
    for (int c = tid; c < cn; c += kThreads) {
      // 0 ≤ pos and pos + taps4 ≤ span: ⌊k·I/O⌋ = u·I + ⌊i·I/O⌋, the definitions of back / fwd / span (mfa_resample_batch)
      const float *xv = xs + ((int)(u * I - base) + first[i]);
      const float *wv = wtab + (size_t)i * p.stride;
      float acc = 0.0f;
      for (int j = 0; j < p.taps4; j += 4) {
        const float w0 = wv[j], w1 = wv[j + 1], w2 = wv[j + 2], w3 = wv[j + 3];
        const float x0 = xv[j], x1 = xv[j + 1], x2 = xv[j + 2], x3 = xv[j + 3];
        acc = fmaf(w0, x0, acc); acc = fmaf(w1, x1, acc); acc = fmaf(w2, x2, acc); acc = fmaf(w3, x3, acc);
      }
      const float r = fminf(fmaxf(__builtin_rintf(acc), -32768.0f), 32767.0f);   // (round to nearest even)
      y[kc + c] = (int16_t)(int)r;
      u += step_u; i += step_i;
      if (i >= O) { i -= O; u += 1; }
    }
  }
}

int plan_for(mfa_ctx *c, int32_t in_hz, int32_t out_hz, MfaResampleDevicePlan **out) {
  for (auto &q : c->resample_plans)
    if (q.in_hz == in_hz && q.out_hz == out_hz) { *out = &q; return 0; }
  MfaResampleHostPlan h;
  mfa_resample_host_plan(in_hz, out_hz, true, &h);
  MfaResampleDevicePlan d;
  d.in_hz = in_hz; d.out_hz = out_hz;
  d.phases = h.phases; d.in_per_unit = h.in_per_unit; d.max_taps = h.max_taps;
  d.taps4 = (h.max_taps + 3) & ~3;
  d.stride = d.taps4 + 1;
  // where the taps of phase i lie around its position ⌊i·I/O⌋; fwd counts the padded row (taps4, not taps_i)
  int back = 0, fwd = 0;
  for (int i = 0; i < h.phases; i++) {
    const int pos = (int)((int64_t)i * h.in_per_unit / h.phases);
    back = std::max(back, pos - h.first[i]);
    fwd = std::max(fwd, h.first[i] + d.taps4 - 1 - pos);
  }
  d.back = back;
  auto span_of = [&](int chunk) {
    return (int64_t)(((int64_t)(chunk - 1) * h.in_per_unit + h.phases - 1) / h.phases) + back + fwd + 2;
  };
  int chunk = kOutPerBlock;
  while (chunk > 1 && span_of(chunk) > kMaxSpanFloats) chunk >>= 1;
  if (span_of(chunk) > kMaxSpanFloats)
    return c->fail("resampler: a filter of %d taps (%d Hz -> %d Hz) does not fit the staging buffer", h.max_taps, in_hz, out_hz);
  d.chunk = chunk; d.span = (int)span_of(chunk);
  const size_t table_floats = (size_t)h.phases * (1 + d.stride);
  d.table_in_lds = ((size_t)d.span + table_floats) * sizeof(float) <= kMaxLdsBytes;
  std::vector<float> rows((size_t)h.phases * d.stride, 0.0f);
  for (int i = 0; i < h.phases; i++)
    std::copy(h.weights.begin() + (size_t)i * h.max_taps, h.weights.begin() + (size_t)(i + 1) * h.max_taps, rows.begin() + (size_t)i * d.stride);
  if (dev_upload_commit<MfaHipDev>(c, "the resampler's phase table",
                        {{&d.d_first, h.first.data(), h.first.size() * sizeof(int32_t)}, {&d.d_w, rows.data(), rows.size() * sizeof(float)}}))
    return -1;
  c->resample_plans.push_back(std::move(d));
  *out = &c->resample_plans.back();
  return 0;
}

}  // namespace

extern "C" {

MFA_API int32_t mfa_resample_block_outputs(void) { return kOutPerBlock; }

MFA_API int mfa_resample_batch(mfa_ctx *c, int32_t in_hz, int32_t out_hz, const int16_t *d_in, const int64_t *d_in_off,
                               int16_t *d_out, const int64_t *d_out_off, const int32_t *d_utt, int32_t n_sel, int64_t max_out) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (!mfa_resample_rates_ok(in_hz, out_hz))
    return c->fail("resampler: rates must lie in %d - %d Hz (got %d Hz -> %d Hz)", kMfaResampleMinHz, kMfaResampleMaxHz, in_hz, out_hz);
  if (in_hz == out_hz) return c->fail("resampler: input and output rate are both %d Hz (copy the samples instead)", in_hz);
  if (n_sel < 0 || max_out < 0) return c->fail("resampler: negative utterance count or length");
  if (n_sel > 65535) return c->fail("at most 65535 utterances per resampler launch (got %d)", n_sel);
  const int64_t blocks = (max_out + kOutPerBlock - 1) / kOutPerBlock;
  if (blocks > 0x7FFFFFFF) return c->fail("resampler: %lld output samples in one utterance", (long long)max_out);
  if (n_sel == 0 || max_out == 0) return 0;
  MfaResampleDevicePlan *d = nullptr;
  if (plan_for(c, in_hz, out_hz, &d) != 0) return -1;
  ResampleParams p;
  p.phases = d->phases; p.in_per_unit = d->in_per_unit; p.taps4 = d->taps4; p.stride = d->stride;
  p.back = d->back; p.chunk = d->chunk; p.span = d->span;
  p.first = d->d_first.ptr<int32_t>(); p.w = d->d_w.ptr<float>();
  dim3 grid((unsigned)blocks, (unsigned)n_sel);
  KernelTimer kt(c, MFA_K_RESAMPLE);
  if (d->table_in_lds) {
    const size_t lds = ((size_t)d->span + (size_t)d->phases * (1 + d->stride)) * sizeof(float);
    hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(kThreads), lds, c->stream, p, d_in, d_in_off, d_out, d_out_off, d_utt);
  } else {
    hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(kThreads), (size_t)d->span * sizeof(float), c->stream, p, d_in, d_in_off,
                       d_out, d_out_off, d_utt);
  }
  MFA_HIP_CHECK(c, hipGetLastError());
  MFA_DEBUG_POINT(c, "resample_kernel %d Hz -> %d Hz, %d utterances", in_hz, out_hz, n_sel);
  return 0;
}

}  // extern "C"
