// What the tree statistics (tree_acc.hip) and their host twin (tree_acc_host.cpp) share: the contract of include/mfa_hip.h
// ("Tree statistics") for the event key, the participation rule and the arithmetic of one addition.  Both sides run exactly
// these functions, so the keys, the frames that take part and the order of the events are the same by construction; what may
// differ is the order of the double additions.  Compiled with -ffp-contract=off.  Plain C++: no HIP type, so the twin's
// translation unit also builds with a host compiler alone (tests/native/tree_acc_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define MFA_TREE_FN __host__ __device__ inline
#else
#define MFA_TREE_FN inline
#endif

constexpr int kTreeMaxDim = 48;                  // the GMM statistics' limit: those run next (mfa_tree_acc_max_dim)
constexpr int kTreeChunk = 512;                  // frames of an event per chunk (mfa_tree_acc_chunk_frames)
constexpr int32_t kTreeMaxPhones = 1 << 16;      // the left phone has bits 48..63 of the key
constexpr int32_t kTreeMaxClasses = 256;         // the pdf-class has bits 0..7
constexpr uint64_t kTreeNoKey = ~(uint64_t)0;    // a frame that takes no part

// The frame's transition-id can be looked up at all.
MFA_TREE_FN bool tree_tid_ok(int32_t tid, int32_t n_tids) { return tid > 0 && tid < n_tids; }

// Phone and pdf-class of a looked-up transition-id are inside what the key holds and what the phone table covers.
MFA_TREE_FN bool tree_entry_ok(int32_t phone, int32_t pdf_class, int32_t n_phones) {
  return phone > 0 && phone <= n_phones && pdf_class >= 0 && pdf_class < kTreeMaxClasses;
}

// The per transition-id flags of d_tid_flags.
constexpr int32_t kTreeFinal = 1, kTreeSelfLoop = 2;

// Segments of a reordered alignment (the graphs of this project put a state's self-loops after its forward arc, as Kaldi's
// reorder option does): a frame is in the tail of its segment when its transition-id is final, or a self-loop that follows
// a tail frame; the segment ends at the tail frame that no self-loop follows.
MFA_TREE_FN bool tree_tail(int32_t flags, bool prev_tail) { return (flags & kTreeFinal) || ((flags & kTreeSelfLoop) && prev_tail); }
MFA_TREE_FN bool tree_segment_end(bool tail, int32_t next_flags) { return tail && !(next_flags & kTreeSelfLoop); }

// key = l << 48 | c << 28 | r << 8 | pc; a context-independent centre has l = r = 0.
MFA_TREE_FN uint64_t tree_event_key(int32_t l, int32_t c, int32_t r, int32_t pc, bool ci) {
  if (ci) { l = 0; r = 0; }
  return (uint64_t)(uint32_t)l << 48 | (uint64_t)(uint32_t)c << 28 | (uint64_t)(uint32_t)r << 8 | (uint64_t)(uint32_t)pc;
}

// The same order on fewer bits, for the sort: the fields packed at `b` bits a phone (b = tree_phone_bits(n_phones)); a frame
// that takes no part sorts after every event.
MFA_TREE_FN int tree_phone_bits(int32_t n_phones) {
  int b = 1;
  while (((int64_t)1 << b) <= (int64_t)n_phones) b++;
  return b;
}
MFA_TREE_FN uint64_t tree_sort_key(uint64_t key, int b) {
  if (key == kTreeNoKey) return (uint64_t)1 << (3 * b + 8);
  const uint64_t l = key >> 48, c = (key >> 28) & 0xFFFFF, r = (key >> 8) & 0xFFFFF, pc = key & 0xFF;
  return ((l << b | c) << b | r) << 8 | pc;
}
MFA_TREE_FN uint64_t tree_key_of_sort_key(uint64_t sk, int b) {
  if (sk >> (3 * b + 8)) return kTreeNoKey;
  const uint64_t m = ((uint64_t)1 << b) - 1;
  return (sk >> (2 * b + 8)) << 48 | ((sk >> (b + 8)) & m) << 28 | ((sk >> 8) & m) << 8 | (sk & 0xFF);
}

// sum += (double)x; sumsq += (double)x·(double)x: the product is exact in double (24 + 24 bits), so each step rounds once.
MFA_TREE_FN void tree_acc_add(float x, double &sum, double &sumsq) {
  const double d = (double)x;
  sum += d;
  sumsq += d * d;
}
