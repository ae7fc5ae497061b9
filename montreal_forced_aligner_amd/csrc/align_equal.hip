// Equal alignment on gfx950: the first alignment of flat-start training (the reference's gmm_align_equal, Kaldi
// EqualAlign restated).  Contract: include/mfa_hip.h "Equal alignment"; the shared arithmetic: align_equal_math.hpp; the
// host twin: align_equal_host.cpp.
//
// One wavefront per utterance, kWaves of them per workgroup.  Lane 0 walks the graph (sequential by nature) and leaves the
// path in the utterance's piece of the workspace; the whole wavefront then spreads the loops: a prefix sum over the path,
// 64 positions at a time, and every position's run written by all lanes, so d_ali is written in consecutive addresses.
// Nothing here is arithmetic-bound.
#include "ctx.hpp"
#include "align_equal_math.hpp"

namespace {

constexpr int kWaves = 4;

struct EqualParams {
  mfa_graph_batch g;
  const int64_t *frame_off;
  const uint32_t *key;
  uint32_t seed;
  int32_t *path;       // per utterance two arrays of mfa_ae_path_capacity(T_u, S_u) entries: loops' ids, outgoing labels
  int64_t positions;   // path positions the workspace holds, and the frames d_ali holds: an utterance whose offsets do not
  int64_t total_frames;   // fit them (the caller's totals were not the arrays') fails without touching either
  int32_t *ali;
  int32_t *status;
};

__global__ __launch_bounds__(64 * kWaves) void align_equal_kernel(EqualParams p) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (u >= p.g.n_utt) return;                      // the same for the whole wavefront
  const int64_t f0 = p.frame_off[u], T = p.frame_off[u + 1] - f0;
  const int64_t s0 = p.g.d_state_off[u], S = p.g.d_state_off[u + 1] - s0;
  const int64_t a0 = p.g.d_arc_base[u], A = p.g.d_arc_base[u + 1] - a0;
  // positions before this utterance's: Σ_{v<u} (2 (T_v + S_v) + 1), two arrays of them each
  const int64_t before = 2 * ((f0 - p.frame_off[0]) + (s0 - p.g.d_state_off[0])) + u;
  const bool fits = T >= 0 && S > 0 && S <= INT32_MAX && A >= 0 && A <= INT32_MAX && before >= 0 && f0 >= 0 &&
                    f0 + T <= p.total_frames && before + mfa_ae_path_capacity(T, S) <= p.positions;
  const int64_t cap = fits ? mfa_ae_path_capacity(T, S) : 0;
  int32_t *loop_tid = p.path + 2 * before, *out_tid = loop_tid + cap;
  int32_t st = 2, n_pos = 0, n_labels = 0, n_loopable = 0;
  if (lane == 0 && fits) {
    MfaAeGraph g{(int32_t)S, (int32_t)A, p.g.d_start[u], p.g.d_arc_off + s0 + u, p.g.d_arc_next + a0, p.g.d_arc_ilabel + a0,
                 p.g.d_final + s0};
    st = mfa_ae_walk(g, T, p.seed, p.key[u], loop_tid, out_tid, &n_pos, &n_labels, &n_loopable);
  }
  __threadfence_block();                           // lane 0's path, before the other lanes read it
  st = __shfl(st, 0); n_pos = __shfl(n_pos, 0); n_labels = __shfl(n_labels, 0); n_loopable = __shfl(n_loopable, 0);
  const int32_t extra = (int32_t)T - n_labels;
  if (st == 0 && n_loopable == 0 && extra > 0) st = 2;
  if (lane == 0) p.status[u] = st;
  int32_t *ali = p.ali + f0;
  if (st != 0) {
    if (fits)
      for (int64_t t = lane; t < T; t += 64) ali[t] = 0;
    return;
  }
  const int32_t Ti = (int32_t)T;
  int32_t rank0 = 0, at0 = 0;                      // loopable positions and frames before this round's 64 positions
  for (int32_t base = 0; base < n_pos; base += 64) {
    const int32_t i = base + lane;
    const int32_t lt = i < n_pos ? loop_tid[i] : 0, ot = i < n_pos ? out_tid[i] : 0;
    const unsigned long long can = __ballot(lt != 0);
    const int32_t rank = rank0 + __popcll(can & (((unsigned long long)1 << lane) - 1));
    const int32_t loops = lt != 0 ? mfa_ae_loops(extra, n_loopable, rank) : 0;
    const int32_t len = loops + (ot != 0 ? 1 : 0);
    int32_t incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    const int32_t at = at0 + incl - len;
    const int32_t n_here = min(64, n_pos - base);
    for (int j = 0; j < n_here; j++) {
      const int32_t lj = __shfl(len, j);
      if (lj == 0) continue;                       // the same for the whole wavefront
      const int32_t aj = __shfl(at, j), loops_j = __shfl(loops, j), lt_j = __shfl(lt, j), ot_j = __shfl(ot, j);
      for (int32_t f = lane; f < lj; f += 64)
        if (aj + f < Ti) ali[aj + f] = f < loops_j ? lt_j : ot_j;
    }
    rank0 += __popcll(can);
    at0 += __shfl(incl, 63);
  }
}

}  // namespace

extern "C" {

MFA_API int mfa_align_equal_batch(mfa_ctx *c, const mfa_graph_batch *graphs, const int64_t *d_frame_off, int64_t total_frames,
                                  int64_t total_states, const uint32_t *d_utt_key, uint32_t seed, int32_t *d_ali,
                                  int32_t *d_status) {
  MFA_HIP_CHECK(c, hipSetDevice(c->device));
  if (!graphs) return c->fail("equal alignment: no graph batch");
  const int n = graphs->n_utt;
  if (n < 0) return c->fail("equal alignment: %d utterances", n);
  if (n == 0) return 0;
  if (!graphs->d_state_off || !graphs->d_arc_base || !graphs->d_start || !graphs->d_arc_off || !graphs->d_final ||
      !graphs->d_arc_next || !graphs->d_arc_ilabel)
    return c->fail("equal alignment: a graph array is NULL (state_off, arc_base, start, arc_off, final, arc_next and arc_ilabel are read)");
  if (!d_frame_off || !d_utt_key || !d_status) return c->fail("equal alignment: frame offsets, utterance keys or status is NULL");
  if (total_frames < 0 || total_states < 0) return c->fail("equal alignment: negative totals");
  if (total_frames >= ((int64_t)1 << 31)) return c->fail("equal alignment: %lld frames in one call (at most 2^31 - 1)", (long long)total_frames);
  if (total_frames > 0 && !d_ali) return c->fail("equal alignment: d_ali is NULL");
  const size_t positions = 2 * ((size_t)total_frames + (size_t)total_states) + (size_t)n;
  if (c->d_ws.reserve(c, positions * 2 * sizeof(int32_t), "the equal alignment's paths")) return -1;
  EqualParams p{*graphs, d_frame_off, d_utt_key, seed, c->d_ws.ptr<int32_t>(), (int64_t)positions, total_frames, d_ali, d_status};
  {
    KernelTimer kt(c, MFA_K_EQUAL_ALIGN);
    hipLaunchKernelGGL(align_equal_kernel, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, c->stream, p);
    MFA_HIP_CHECK(c, hipGetLastError());
  }
  return 0;
}

}  // extern "C"
