// The packed acoustic model as a host value (gmm_pack.cpp): what mfa_load_gmm uploads, what mfa_fmllr_stats_model lays its
// rows out by, and what tests/test_gmm_pack_cpu.py reads through mfa_debug_gmm_pack.  No device types, no HIP call.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIP__) || defined(__HIPCC__)
#define MFA_HOST_DEVICE __host__ __device__
#else
#define MFA_HOST_DEVICE
#endif

// Packed model layout (built by gmm_pack_model, read by gmm.hip, gmm_band.hip and fmllr.hip).  Rows (Gaussians) are grouped
// in blocks of 32; a block is stored operand-major: for every group m of 8 k-values and half h, the 32 rows' 4-float pieces
// lie side by side —  float offset of (row, logical k = 8m + 2c + h):
//     (row >> 5) · 32·kpad  +  ((2m + h) · 32 + (row & 31)) · 4  +  c
// so the 16-byte A-operand loads of the 32 lanes of a half-wavefront (one row each) read 512 contiguous bytes.
MFA_HOST_DEVICE inline size_t mfa_packed_offset(int row, int k, int kpad) {
  const int m = k >> 3, o = k & 7, h = o & 1, c = o >> 1;
  return (size_t)(row >> 5) * 32 * kpad + (size_t)(((2 * m + h) * 32 + (row & 31)) * 4 + c);
}

struct GmmPacked {
  int dim = 0, kpad = 0, num_pdfs = 0;
  int rows = 0, blocks = 0;                  // rows handed out (a multiple of 4; `rows` itself is the dummy row); 32-row blocks
  std::vector<int32_t> row0, nblk, slot;     // [num_pdfs + 1] first row (last entry: rows); [num_pdfs] blocks; [num_pdfs] slot rows
  std::vector<float> w, gc;                  // [blocks·32·kpad] weights (mfa_packed_offset); [blocks·32] gconsts, pads −1e30
  // split operands of the 16-bit matrix pipe, only for rows of 80 or 96 floats (empty otherwise): 32-row blocks of
  // [step][piece][half][row] 16-byte units
  std::vector<uint16_t> wb, wh;              // bf16×3 pieces; f16×2 pieces of the column-scaled weights
  std::vector<float> gch, fscale;            // gc × acc_scale; [kpad] feature column scales S·2^-e_k
  float acc_scale = 1.0f;                    // S
  bool has_slot_class[5] = {false, false, false, false, false};
  bool has_single32 = false, has_multi_block = false, all_pdfs_32row = false;
  int max_nblk = 1;
  bool split() const { return kpad == 80 || kpad == 96; }
};

// 16-byte unit of (row, 16-k step, piece, k-half) in the split-operand tables
inline size_t gmm_split_unit(int row, int step, int piece, int half, int steps, int pieces) {
  return (size_t)(row >> 5) * steps * pieces * 2 * 32 + (size_t)((step * pieces + piece) * 2 + half) * 32 + (row & 31);
}

// w[(row0[p] + i, k)] = means·inv_vars | −½ inv_vars of Gaussian i of pdf p; w must hold whole blocks and is not cleared
void gmm_pack_rows(int dim, int num_pdfs, const int32_t *pdf_offsets, const int32_t *row0, int kpad,
                   const float *means_invvars, const float *inv_vars, std::vector<float> &w);

// 0, or −(p + 1) when pdf p has no Gaussians
int gmm_pack_model(int dim, int num_pdfs, const int32_t *pdf_offsets, const float *gconsts, const float *means_invvars,
                   const float *inv_vars, GmmPacked &m);

// Sorts h_pdfs[n] into the scoring kernels' order (mfa_gmm_sort_pdf_list[_keyed]; h_keys may be NULL); 0, or −(i + 1) when
// h_pdfs[i] is not a pdf of the model
int gmm_sort_pdf_list(const std::vector<int32_t> &slot, const std::vector<int32_t> &nblk, int32_t *h_pdfs, int32_t *h_keys,
                      int32_t n, int32_t *h_class_counts);
