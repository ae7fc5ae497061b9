// The arithmetic of the feature codec (compress.hip), host and device: kaldi_io.write_compressed_matrix / _read_compressed
// operation for operation.  The kernel and the host restatement behind mfa_debug_compress_host (which the CPU tests hold
// to kaldi_io bit for bit) both run exactly these functions; only how the order statistics are found differs.
// Compiled with -ffp-contract=off; on the device every float32 operation is an _rn intrinsic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define MFA_CODEC_FN __host__ __device__ inline
#if defined(__HIP_DEVICE_COMPILE__)
MFA_CODEC_FN float cadd(float a, float b) { return __fadd_rn(a, b); }
MFA_CODEC_FN float csub(float a, float b) { return __fsub_rn(a, b); }
MFA_CODEC_FN float cmul(float a, float b) { return __fmul_rn(a, b); }
MFA_CODEC_FN float cdiv(float a, float b) { return __fdiv_rn(a, b); }
MFA_CODEC_FN double cmuladd(double a, double b, double c) { return __dadd_rn(__dmul_rn(a, b), c); }
#else
MFA_CODEC_FN float cadd(float a, float b) { return a + b; }
MFA_CODEC_FN float csub(float a, float b) { return a - b; }
MFA_CODEC_FN float cmul(float a, float b) { return a * b; }
MFA_CODEC_FN float cdiv(float a, float b) { return a / b; }
MFA_CODEC_FN double cmuladd(double a, double b, double c) { const double m = a * b; return m + c; }
#endif

// ComputeGlobalHeader from the table's extremes: {min, range}; a constant table gets the range 1 + |min| (in double,
// rounded once, then the float32 difference — as the writer has it)
MFA_CODEC_FN void codec_global(float mn, float mx, float *range) {
  if (mx == mn) mx = (float)((double)mn + (1.0 + (mn < 0.0f ? -(double)mn : (double)mn)));
  *range = csub(mx, mn);
}

// the writer's to_u16: the float32 quotient widened, clamped to [0, 1], scaled and rounded in double
MFA_CODEC_FN int codec_u16(float v, float mn, float rng) {
  double fr = (double)cdiv(csub(v, mn), rng);
  fr = fr > 0.0 ? fr : 0.0;          // (a NaN ends up 0: undefined on the host codec, bounded here)
  fr = fr < 1.0 ? fr : 1.0;
  return (int)cmuladd(fr, 65535.0, 0.499);
}

// astype(int64) then clip(0, span) of the writer's byte stage: truncation toward zero; a value no int64 holds (NaN, ±inf,
// ≥ 2^63: a piece whose two percentile floats coincide divides by zero) converts to INT64_MIN there, so it clips low
MFA_CODEC_FN int codec_q8(float t, int span) {
  if (!(t < 9.2233720368547758e18f)) return 0;
  if (t >= (float)span) return span;
  if (t < 1.0f) return 0;
  return (int)t;
}

struct CodecColumn {
  int code[4];                       // p0, p25, p75, p100
  float w0, w25, w75, dw_lo, dw_mid, dw_hi;   // the writer's percentile floats and their differences
  float r0, r25, r75, dr_lo, dr_mid, dr_hi;   // the reader's
};

// ComputeColHeader from the column's order statistics s = {sorted[0], sorted[a], sorted[b], sorted[rows-1]}, with
// (a, b) = (q, 3q), q = rows / 4, from five rows on and (1, 2), where those rows exist, below (the small-matrix rule)
MFA_CODEC_FN CodecColumn codec_column(const float s[4], int rows, float mn, float rng) {
  CodecColumn h;
  int p0, p25, p75, p100;
  const int u0 = codec_u16(s[0], mn, rng), ua = codec_u16(s[1], mn, rng), ub = codec_u16(s[2], mn, rng),
            u3 = codec_u16(s[3], mn, rng);
  p0 = u0 < 65532 ? u0 : 65532;
  if (rows >= 5) {
    p25 = ua > p0 + 1 ? ua : p0 + 1;    p25 = p25 < 65533 ? p25 : 65533;
    p75 = ub > p25 + 1 ? ub : p25 + 1;  p75 = p75 < 65534 ? p75 : 65534;
    p100 = u3 > p75 + 1 ? u3 : p75 + 1;
  } else {
    p25 = rows > 1 && ua > p0 + 1 ? ua : p0 + 1;     p25 = p25 < 65533 ? p25 : 65533;
    p75 = rows > 2 && ub > p25 + 1 ? ub : p25 + 1;   p75 = p75 < 65534 ? p75 : 65534;
    p100 = rows > 3 && u3 > p75 + 1 ? u3 : p75 + 1;
  }
  h.code[0] = p0; h.code[1] = p25; h.code[2] = p75; h.code[3] = p100;
  // writer: inc = f32(range · f32(1/65535)); reader: inc = f32(double(range) · double(1/65535)) — not the same float
  const float inc_w = cmul(rng, (float)(1.0 / 65535.0));
  const float inc_r = (float)((double)rng * (1.0 / 65535.0));
  const float w100 = cadd(mn, cmul(inc_w, (float)p100)), r100 = cadd(mn, cmul(inc_r, (float)p100));
  h.w0 = cadd(mn, cmul(inc_w, (float)p0)); h.w25 = cadd(mn, cmul(inc_w, (float)p25)); h.w75 = cadd(mn, cmul(inc_w, (float)p75));
  h.r0 = cadd(mn, cmul(inc_r, (float)p0)); h.r25 = cadd(mn, cmul(inc_r, (float)p25)); h.r75 = cadd(mn, cmul(inc_r, (float)p75));
  h.dw_lo = csub(h.w25, h.w0); h.dw_mid = csub(h.w75, h.w25); h.dw_hi = csub(w100, h.w75);
  h.dr_lo = csub(h.r25, h.r0); h.dr_mid = csub(h.r75, h.r25); h.dr_hi = csub(r100, h.r75);
  return h;
}

// FloatToChar as the writer has it: IEEE division, ·64 | ·128 | ·63, + 0.5, truncate, clip; branches on x < f25, x < f75
MFA_CODEC_FN int codec_byte(const CodecColumn &h, float x) {
  if (x < h.w25) return codec_q8(cadd(cmul(cdiv(csub(x, h.w0), h.dw_lo), 64.0f), 0.5f), 64);
  if (x < h.w75) return 64 + codec_q8(cadd(cmul(cdiv(csub(x, h.w25), h.dw_mid), 128.0f), 0.5f), 128);
  return 192 + codec_q8(cadd(cmul(cdiv(csub(x, h.w75), h.dw_hi), 63.0f), 0.5f), 63);
}

// CharToFloat as the reader has it: p + (Δp · v) · k, left to right in float32, k = f32(1/64), f32(1/128), f32(1/63)
MFA_CODEC_FN float codec_value(const CodecColumn &h, int b) {
  const float v = (float)b;
  if (b <= 64) return cadd(h.r0, cmul(cmul(h.dr_lo, v), (float)(1 / 64.0)));
  if (b <= 192) return cadd(h.r25, cmul(cmul(h.dr_mid, csub(v, 64.0f)), (float)(1 / 128.0)));
  return cadd(h.r75, cmul(cmul(h.dr_hi, csub(v, 192.0f)), (float)(1 / 63.0)));
}
