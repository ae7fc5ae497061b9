// The host twins of the speech-activity stage (csrc/vad_host.cpp over csrc/vad_math.hpp) as a stand-alone program for the
// host sanitizers: tests/test_vad_cpu.py builds it with -fsanitize=address,undefined and runs it once.  Every array is sized
// exactly, so an index past an end is a report.  Inputs: empty batches, utterances of 0 and 1 frames, lengths around the sum
// chunk and the CMVN tile, contexts and windows larger than the utterance, every subsample factor against short
// utterances, runs that touch both ends, a capacity that is too small, the refusals.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mfa_hip.h"

static int failures = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main() {
  uint32_t seed = 7;
  const std::vector<int64_t> lens = {0, 1, 2, 63, 64, 65, 0, 300, 2047, 2048, 2049, 4100, 1};
  std::vector<int64_t> fo{0};
  for (int64_t n : lens) fo.push_back(fo.back() + n);
  const int32_t n_utt = (int32_t)lens.size();
  const int64_t total = fo.back();

  for (int stride : {1, 3}) {
    std::vector<float> x((size_t)total * stride);
    for (auto &v : x) v = (float)((int)(lcg(seed) >> 20) % 160 - 40) / 8.0f;
    // ---- VAD: contexts up to far beyond the utterances
    for (int ctx : {0, 1, 2, 40, 1 << 30}) {
      mfa_vad_opts o{5.5f, 0.5f, 0.6f, ctx};
      std::vector<float> vad((size_t)total, -1.0f), thr(n_utt, -1.0f);
      std::vector<int32_t> voiced(n_utt, -1);
      CHECK(mfa_debug_vad_host(x.data(), stride, fo.data(), n_utt, &o, vad.data(), thr.data(), voiced.data()) == 0);
      for (int u = 0; u < n_utt; u++) {
        int32_t c = 0;
        for (int64_t f = fo[u]; f < fo[u + 1]; f++) { CHECK(vad[f] == 0.0f || vad[f] == 1.0f); c += vad[f] != 0.0f; }
        CHECK(c == voiced[u]);
      }
      CHECK(thr[0] == 5.5f);                         // no frames: the plain threshold
      // ---- runs, with room for all and with room for one
      std::vector<int64_t> ro(n_utt + 1, -1), ro1(n_utt + 1, -1);
      const int64_t cap = (total + 1) / 2 + n_utt;
      std::vector<int32_t> rb((size_t)cap, -1), re((size_t)cap, -1), rb1(1, -1), re1(1, -1);
      CHECK(mfa_debug_vad_runs_host(vad.data(), fo.data(), n_utt, cap, rb.data(), re.data(), ro.data()) == 0);
      CHECK(mfa_debug_vad_runs_host(vad.data(), fo.data(), n_utt, 1, rb1.data(), re1.data(), ro1.data()) == 0);
      CHECK(ro == ro1 && ro[0] == 0 && ro[n_utt] <= cap);
      for (int u = 0; u < n_utt; u++) {
        int32_t covered = 0;
        for (int64_t r = ro[u]; r < ro[u + 1]; r++) {
          CHECK(rb[r] >= 0 && rb[r] < re[r] && re[r] <= fo[u + 1] - fo[u]);
          if (r > ro[u]) CHECK(rb[r] > re[r - 1]);
          covered += re[r] - rb[r];
        }
        CHECK(covered == voiced[u]);
      }
      // ---- selection
      for (int n : {1, 2, 3, 7}) {
        std::vector<int32_t> src((size_t)total, -1);
        std::vector<int64_t> oo(n_utt + 1, -1);
        CHECK(mfa_debug_select_frames_host(vad.data(), fo.data(), n_utt, n, src.data(), oo.data()) == 0);
        for (int u = 0; u < n_utt; u++) {
          CHECK(oo[u + 1] - oo[u] == (voiced[u] + n - 1) / n);
          for (int64_t r = oo[u]; r < oo[u + 1]; r++) CHECK(src[r] >= fo[u] && src[r] < fo[u + 1] && vad[src[r]] != 0.0f);
        }
        CHECK(mfa_debug_select_frames_host(nullptr, fo.data(), n_utt, n, src.data(), oo.data()) == 0);
        CHECK(oo[n_utt] >= total / n);
      }
      // ---- scan of the decisions
      std::vector<int32_t> flags((size_t)total), scan((size_t)total, -1), totals(n_utt, -1);
      for (int64_t f = 0; f < total; f++) flags[f] = vad[f] != 0.0f;
      CHECK(mfa_debug_vad_scan_host(flags.data(), fo.data(), n_utt, scan.data(), totals.data()) == 0);
      for (int u = 0; u < n_utt; u++) CHECK(totals[u] == voiced[u]);
    }
  }

  // ---- sliding CMVN: widths with and without pad columns, windows below / at / above the lengths
  for (int dim : {1, 13}) {
    const int stride = dim + 2;
    std::vector<float> x((size_t)total * stride), out((size_t)total * stride, -99.0f);
    for (auto &v : x) v = (float)((int)(lcg(seed) >> 20) % 400 - 200) / 8.0f;
    for (int window : {1, 2, 64, 300, 600, 5000})
      for (int center : {0, 1})
        for (int norm : {0, 1}) {
          mfa_sliding_cmvn_opts o{window, 100, center, norm};
          CHECK(mfa_debug_sliding_cmvn_host(x.data(), fo.data(), n_utt, dim, stride, &o, out.data()) == 0);
          for (int64_t f = 0; f < total; f++)
            for (int c = dim; c < stride; c++) CHECK(out[f * stride + c] == x[f * stride + c]);
          CHECK(out[(size_t)fo[1] * stride] == 0.0f);      // an utterance of one frame: x − x
        }
  }

  // ---- empty batches and refusals
  {
    mfa_vad_opts vo{5.0f, 0.5f, 0.6f, 0};
    mfa_sliding_cmvn_opts co{300, 100, 1, 0};
    int64_t zero[2] = {0, 0}, bad[2] = {1, 4}, one_off[1] = {-5};
    float thr = -1.0f, v = 1.0f, y = 0.0f;
    int32_t i = 0;
    CHECK(mfa_debug_vad_host(nullptr, 13, nullptr, 0, &vo, nullptr, nullptr, nullptr) == 0);
    CHECK(mfa_debug_vad_host(nullptr, 13, zero, 1, &vo, nullptr, &thr, nullptr) == 0 && thr == 5.0f);
    CHECK(mfa_debug_vad_host(nullptr, 13, zero, 1, nullptr, nullptr, &thr, nullptr) != 0);
    CHECK(mfa_debug_vad_host(&v, 0, zero, 1, &vo, &y, &thr, nullptr) != 0);
    CHECK(mfa_debug_vad_host(&v, 1, bad, 1, &vo, &y, &thr, nullptr) != 0);
    vo.frames_context = -1;
    CHECK(mfa_debug_vad_host(&v, 1, zero, 1, &vo, &y, &thr, nullptr) != 0);
    CHECK(mfa_debug_sliding_cmvn_host(nullptr, zero, 1, 13, 13, &co, nullptr) == 0);
    CHECK(mfa_debug_sliding_cmvn_host(&v, zero, 1, 13, 12, &co, &y) != 0);
    CHECK(mfa_debug_sliding_cmvn_host(&v, zero, 1, 0, 12, &co, &y) != 0);
    co.cmn_window = 0;
    CHECK(mfa_debug_sliding_cmvn_host(&v, zero, 1, 1, 1, &co, &y) != 0);
    CHECK(mfa_debug_select_frames_host(nullptr, zero, 1, 0, &i, one_off) != 0);
    CHECK(mfa_debug_select_frames_host(nullptr, zero, 1, -2, &i, one_off) != 0);
    CHECK(mfa_debug_select_frames_host(nullptr, nullptr, 0, 1, nullptr, one_off) == 0 && one_off[0] == 0);
    one_off[0] = -5;
    CHECK(mfa_debug_vad_runs_host(nullptr, nullptr, 0, 0, nullptr, nullptr, one_off) == 0 && one_off[0] == 0);
    CHECK(mfa_debug_vad_runs_host(nullptr, zero, 1, -1, nullptr, nullptr, one_off) != 0);
    CHECK(mfa_debug_vad_scan_host(nullptr, nullptr, 0, nullptr, nullptr) == 0);
    CHECK(mfa_debug_vad_scan_host(nullptr, bad, 1, nullptr, nullptr) != 0);
  }
  if (failures == 0) printf("vad_check: ok\n");
  return failures ? 1 : 0;
}
