// The model packer: turns a diagonal-GMM (SoA over all Gaussians) into the row layout, the bf16×3 and the column-scaled
// f16×2 operand tables the scoring kernels read (gmm.hip describes the layout; mfa_load_gmm uploads the result), and the
// host helpers that depend on the layout alone: a pdf's slot class, the order of an utterance's pdf list.  Pure host
// arithmetic — nothing here touches the device, so tests/test_gmm_pack_cpu.py checks it without one (mfa_debug_gmm_pack).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "gmm_pack.hpp"

namespace {

constexpr float kPadGconst = -1.0e30f;   // gconst of pad rows: they fall under the log-sum-exp cutoff

int slot_of(int g) { return g <= 1 ? 1 : g <= 4 ? 4 : g <= 8 ? 8 : g <= 16 ? 16 : 32; }
int class_index(int slot) { return slot == 32 ? 0 : slot == 16 ? 1 : slot == 8 ? 2 : slot == 4 ? 3 : 4; }

// bf16×3 split for the bf16 kernels: blocks of [step][piece][half][row] × 8 bf16 (natural k order, zero padded)
void pack_bf16x3(GmmPacked &m) {
  const int dim = m.dim, kpad = m.kpad, rows = m.rows, steps = kpad / 16;
  const std::vector<float> &w = m.w;
  std::vector<uint16_t> &wb = m.wb;
  wb.assign((size_t)m.blocks * steps * 3 * 2 * 32 * 8, 0);
  auto to_bf16 = [](float f) -> uint16_t {   // round to nearest even, as the device's v_cvt_pk_bf16_f32
    uint32_t u; memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  };
  auto from_bf16 = [](uint16_t b) -> float { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; };
  for (int row = 0; row < rows; row++) {
    for (int k = 0; k < 2 * dim; k++) {
      const float v = w[mfa_packed_offset(row, k, kpad)];
      const uint16_t v1 = to_bf16(v);
      const float r1 = v - from_bf16(v1);
      const uint16_t v2 = to_bf16(r1);
      const float r2 = r1 - from_bf16(v2);
      const uint16_t piece[3] = {v1, v2, to_bf16(r2)};
      const int s_ = k >> 4, hh = (k >> 3) & 1, e = k & 7;
      for (int qq = 0; qq < 3; qq++) wb[gmm_split_unit(row, s_, qq, hh, steps, 3) * 8 + e] = piece[qq];
    }
  }
}

// f16×2 split (default scoring path of the 32-row classes without multi-block pdfs).  Column k of the weights is
// multiplied by 2^e_k and column k of x̃ by S·2^-e_k, so every product — and the gconst, stored × S — carries the one
// factor S and nothing is rounded differently.  The exponents balance the two operands inside the f16 range using the
// model's own idea of how large a feature can get (|μ| + 10σ over all Gaussians); features beyond 65000 after scaling
// are caught per tile on the device (see gmm_split_single_kernel).
void pack_f16x2(GmmPacked &pm, const int32_t *h_pdf_offsets, const float *h_means_invvars, const float *h_inv_vars) {
  const int dim = pm.dim, kpad = pm.kpad, rows = pm.rows, num_pdfs = pm.num_pdfs, steps = kpad / 16;
  const std::vector<float> &w = pm.w, &gc = pm.gc;
  std::vector<uint16_t> &wh = pm.wh;
  std::vector<float> &fscale = pm.fscale, &gch = pm.gch;
  std::vector<double> wmax(2 * dim, 0.0), xmax(2 * dim, 0.0);
  for (int p = 0; p < num_pdfs; p++) {
    int g0 = h_pdf_offsets[p], g = h_pdf_offsets[p + 1] - g0;
    for (int i = 0; i < g; i++) {
      const float *mi = h_means_invvars + (size_t)(g0 + i) * dim, *iv = h_inv_vars + (size_t)(g0 + i) * dim;
      for (int k = 0; k < dim; k++) {
        const double v = iv[k], m = mi[k];
        if (std::isfinite(m)) wmax[k] = std::max(wmax[k], std::fabs(m));
        if (std::isfinite(v)) wmax[dim + k] = std::max(wmax[dim + k], 0.5 * std::fabs(v));
        if (std::isfinite(v) && std::isfinite(m) && v > 0) {
          const double reach = std::fabs(m / v) + 10.0 / std::sqrt(v);
          if (std::isfinite(reach)) { xmax[k] = std::max(xmax[k], reach); xmax[dim + k] = std::max(xmax[dim + k], reach * reach); }
        }
      }
    }
  }
  int log_s = 12;
  for (int k = 0; k < 2 * dim; k++)
    if (wmax[k] > 0 && xmax[k] > 0) log_s = std::min(log_s, (int)std::floor(26.0 - std::log2(wmax[k] * xmax[k])));
  log_s = std::max(log_s, -20);
  pm.acc_scale = std::ldexp(1.0f, log_s);
  std::vector<int> e_w(2 * dim, 0);
  for (int k = 0; k < 2 * dim; k++) {
    if (!(wmax[k] > 0)) { fscale[k] = 0.0f; continue; }           // an all-zero weight column: x̃_k is irrelevant
    const double xm = xmax[k] > 0 ? xmax[k] : 1.0;
    int e = (int)std::lround(0.5 * (log_s + std::log2(xm) - std::log2(wmax[k])));
    while (std::ldexp(wmax[k], e) > 32768.0) e--;                 // never let the weights themselves leave the range
    e = std::max(-100, std::min(100, e));
    e_w[k] = e;
    fscale[k] = (float)std::ldexp(1.0, log_s - e);
  }
  wh.assign((size_t)pm.blocks * steps * 2 * 2 * 32 * 8, 0);
  auto f16_bits = [](float f) -> uint16_t { _Float16 hv = (_Float16)f; uint16_t u; memcpy(&u, &hv, 2); return u; };
  for (int row = 0; row < rows; row++) {
    for (int k = 0; k < 2 * dim; k++) {
      const float v = std::ldexp(w[mfa_packed_offset(row, k, kpad)], e_w[k]);
      const _Float16 v1 = (_Float16)v;
      const float r1 = v - (float)v1;
      const uint16_t piece[2] = {f16_bits(v), f16_bits(r1)};
      const int s_ = k >> 4, hh = (k >> 3) & 1, e = k & 7;
      for (int qq = 0; qq < 2; qq++) wh[gmm_split_unit(row, s_, qq, hh, steps, 2) * 8 + e] = piece[qq];
    }
  }
  gch.resize(gc.size());
  for (size_t i = 0; i < gc.size(); i++) gch[i] = gc[i] * pm.acc_scale;
}

}  // namespace

void gmm_pack_rows(int dim, int num_pdfs, const int32_t *h_pdf_offsets, const int32_t *row0, int kpad,
                   const float *h_means_invvars, const float *h_inv_vars, std::vector<float> &w) {
  for (int p = 0; p < num_pdfs; p++) {
    int g0 = h_pdf_offsets[p], g = h_pdf_offsets[p + 1] - g0;
    for (int i = 0; i < g; i++) {
      const float *mi = h_means_invvars + (size_t)(g0 + i) * dim, *iv = h_inv_vars + (size_t)(g0 + i) * dim;
      for (int k = 0; k < 2 * dim; k++)
        w[mfa_packed_offset(row0[p] + i, k, kpad)] = k < dim ? mi[k] : -0.5f * iv[k - dim];
    }
  }
}

int gmm_pack_model(int dim, int num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts, const float *h_means_invvars,
                   const float *h_inv_vars, GmmPacked &m) {
  m = GmmPacked();
  m.dim = dim; m.num_pdfs = num_pdfs;
  // the MFMA kernel is instantiated for rows of exactly 80 or 96 floats; wider models use the naive kernel
  const int kpad = 2 * dim <= 80 ? 80 : (2 * dim <= 96 ? 96 : ((2 * dim + 7) / 8) * 8);
  m.kpad = kpad;
  std::vector<int32_t> &row0 = m.row0, &nblk = m.nblk, &slot = m.slot;
  row0.assign(num_pdfs + 1, 0); nblk.assign(num_pdfs, 0); slot.assign(num_pdfs, 0);
  for (int p = 0; p < num_pdfs; p++) {
    int g = h_pdf_offsets[p + 1] - h_pdf_offsets[p];
    if (g <= 0) return -(p + 1);
    slot[p] = slot_of(g);
    nblk[p] = slot[p] == 32 ? (g + 31) / 32 : 1;
  }
  // rows are handed out class by class (32, 16, 8, 4, 1): every pdf then starts at a multiple of its slot size, so the
  // gconst rows of a 32-row block can be fetched with aligned 16-byte loads
  int rows = 0;
  for (int cls : {32, 16, 8, 4, 1})
    for (int p = 0; p < num_pdfs; p++)
      if (slot[p] == cls) { row0[p] = rows; rows += cls == 32 ? 32 * nblk[p] : cls; }
  rows = (rows + 3) & ~3;
  row0[num_pdfs] = rows;
  m.rows = rows;
  // whole 32-row blocks, plus room for the dummy row `rows` (zero weights, gconst −1e30) that idle lanes address
  const int blocks = (rows + 1 + 31) / 32;
  m.blocks = blocks;
  m.w.assign((size_t)blocks * 32 * kpad, 0.0f);
  m.gc.assign((size_t)blocks * 32, kPadGconst);
  gmm_pack_rows(dim, num_pdfs, h_pdf_offsets, row0.data(), kpad, h_means_invvars, h_inv_vars, m.w);
  for (int p = 0; p < num_pdfs; p++) {
    int g0 = h_pdf_offsets[p], g = h_pdf_offsets[p + 1] - g0;
    for (int i = 0; i < g; i++) m.gc[row0[p] + i] = h_gconsts[g0 + i];
  }
  m.fscale.assign(kpad, 0.0f);
  if (m.split()) {
    pack_bf16x3(m);
    pack_f16x2(m, h_pdf_offsets, h_means_invvars, h_inv_vars);
  }
  m.all_pdfs_32row = true;
  for (int p = 0; p < num_pdfs; p++) {
    if (slot[p] != 32) m.all_pdfs_32row = false;
    if (nblk[p] > 1) m.has_multi_block = true;
    m.max_nblk = std::max(m.max_nblk, nblk[p]);
    if (slot[p] == 32 && nblk[p] == 1) m.has_single32 = true;
    m.has_slot_class[class_index(slot[p])] = true;
  }
  return 0;
}

// Sorts h_pdfs[n] into the scoring kernels' class order; inside a class by ascending key (h_keys, permuted along), or — no
// keys — in the order given: the buckets are filled in list order and the sort is stable.
int gmm_sort_pdf_list(const std::vector<int32_t> &slot, const std::vector<int32_t> &nblk, int32_t *h_pdfs, int32_t *h_keys,
                      int32_t n, int32_t *h_class_counts) {
  std::vector<std::pair<int32_t, int32_t>> bucket[6];  // (key, pdf)
  for (int i = 0; i < n; i++) {
    int p = h_pdfs[i];
    if (p < 0 || p >= (int)slot.size()) return -(i + 1);
    int ci = class_index(slot[p]);
    bucket[ci == 0 ? (nblk[p] == 1 ? 0 : 1) : ci + 1].push_back({h_keys ? h_keys[i] : 0, p});
  }
  int k = 0;
  for (int b = 0; b < 6; b++) {
    std::stable_sort(bucket[b].begin(), bucket[b].end(),
                     [](const std::pair<int32_t, int32_t> &x, const std::pair<int32_t, int32_t> &y) { return x.first < y.first; });
    h_class_counts[b] = (int32_t)bucket[b].size();
    for (auto &e : bucket[b]) { if (h_keys) h_keys[k] = e.first; h_pdfs[k++] = e.second; }
  }
  return 0;
}

static int sort_for_ctx(mfa_ctx *c, int32_t *h_pdfs, int32_t *h_keys, int32_t n, int32_t *h_class_counts) {
  if (!c->gmm_ready) return c->fail("mfa_load_gmm has not been called");
  const int bad = gmm_sort_pdf_list(c->h_slot, c->h_nblk, h_pdfs, h_keys, n, h_class_counts);
  if (bad) return c->fail("pdf id %d out of range [0,%d)", h_pdfs[-bad - 1], c->num_pdfs);
  return 0;
}

extern "C" {

MFA_API int32_t mfa_gmm_slot(mfa_ctx *c, int32_t pdf) {
  if (!c->gmm_ready || pdf < 0 || pdf >= c->num_pdfs) return -1;
  return c->h_slot[pdf];
}

MFA_API int mfa_gmm_sort_pdf_list(mfa_ctx *c, int32_t *h_pdfs, int32_t n, int32_t *h_class_counts) {
  return sort_for_ctx(c, h_pdfs, nullptr, n, h_class_counts);
}

MFA_API int mfa_gmm_sort_pdf_list_keyed(mfa_ctx *c, int32_t *h_pdfs, int32_t *h_first_frame, int32_t n,
                                        int32_t *h_class_counts) {
  return sort_for_ctx(c, h_pdfs, h_first_frame, n, h_class_counts);
}

MFA_API int mfa_debug_gmm_pack(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                               const float *h_means_invvars, const float *h_inv_vars, int32_t *h_info, float *h_acc_scale,
                               int32_t *h_row0, int32_t *h_nblk, int32_t *h_slot, float *h_w, float *h_gc, uint16_t *h_wb,
                               uint16_t *h_wh, float *h_gch, float *h_fscale, int32_t *h_sort_pdfs, int32_t *h_sort_keys,
                               int32_t n_sort, int32_t *h_sort_counts) {
  if (dim <= 0 || num_pdfs <= 0) return -1;
  GmmPacked m;
  if (gmm_pack_model(dim, num_pdfs, h_pdf_offsets, h_gconsts, h_means_invvars, h_inv_vars, m) != 0) return -1;
  const int32_t info[13] = {m.kpad, m.rows, m.blocks, m.split() ? 1 : 0, m.has_slot_class[0], m.has_slot_class[1],
                            m.has_slot_class[2], m.has_slot_class[3], m.has_slot_class[4], m.has_single32, m.has_multi_block,
                            m.max_nblk, m.all_pdfs_32row};
  memcpy(h_info, info, sizeof(info));
  *h_acc_scale = m.acc_scale;
  auto copy = [](auto *dst, const auto &v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
  copy(h_row0, m.row0); copy(h_nblk, m.nblk); copy(h_slot, m.slot); copy(h_w, m.w); copy(h_gc, m.gc);
  copy(h_wb, m.wb); copy(h_wh, m.wh); copy(h_gch, m.gch); copy(h_fscale, m.fscale);
  if (h_sort_pdfs && gmm_sort_pdf_list(m.slot, m.nblk, h_sort_pdfs, h_sort_keys, n_sort, h_sort_counts) != 0) return -2;
  return 0;
}

}  // extern "C"
