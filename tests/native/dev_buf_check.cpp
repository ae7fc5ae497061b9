// Host check of csrc/dev_buf.hpp: the buffer type and the table-set upload over a fake device that counts what is live,
// records the order of its calls and fails the n-th allocation or copy on request.  Built and run by
// tests/test_dev_buf_cpu.py with the address and undefined-behaviour sanitizers; exit status 0 means every check held.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../montreal_forced_aligner_amd/csrc/dev_buf.hpp"

namespace {

struct Fake {
  static int live, allocs, copies, fail_alloc_at, fail_copy_at;   // fail_*_at: 1-based count of the call to fail, 0: none
  static size_t live_bytes;
  static std::string log;   // 's' sync, 'f' free, 'a' alloc, 'c' copy
  struct Block { size_t bytes; };
  static int alloc(void **p, size_t bytes) {
    log += 'a';
    if (++allocs == fail_alloc_at) { *p = (void *)0x1; return 2; }   // a failed call may leave garbage behind
    Block *b = (Block *)malloc(sizeof(Block) + bytes);
    b->bytes = bytes;
    live++; live_bytes += bytes;
    *p = b + 1;
    return 0;
  }
  static void free(void *p) {
    log += 'f';
    Block *b = (Block *)p - 1;
    live--; live_bytes -= b->bytes;
    ::free(b);
  }
  static int copy_h2d(void *dst, const void *src, size_t bytes) {
    log += 'c';
    if (++copies == fail_copy_at) return 3;
    memcpy(dst, src, bytes);
    return 0;
  }
  static int sync(int) { log += 's'; return 0; }
  static const char *describe(int code) { return code == 2 ? "out of memory" : "copy failed"; }
  static void reset_counts() { allocs = copies = fail_alloc_at = fail_copy_at = 0; log.clear(); }
};
int Fake::live = 0, Fake::allocs = 0, Fake::copies = 0, Fake::fail_alloc_at = 0, Fake::fail_copy_at = 0;
size_t Fake::live_bytes = 0;
std::string Fake::log;

struct Ctx {
  int stream = 0;
  std::string err;
  int fail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return -1;
  }
};

using Buf = DevBuf<Fake>;

int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

void check_reserve() {
  Ctx c;
  Buf b;
  CHECK(!b && b.ptr() == nullptr && b.bytes() == 0);
  Fake::reset_counts();
  CHECK(b.reserve(&c, 0, "x") == 0 && Fake::log.empty() && !b);   // nothing asked of an empty buffer
  CHECK(b.reserve(&c, 100, "x") == 0);
  CHECK(Fake::log == "a");                                         // an empty buffer grows without sync or free
  CHECK(b && b.bytes() == 100 && Fake::live == 1 && Fake::live_bytes == 100);
  Fake::reset_counts();
  void *p = b.ptr();
  CHECK(b.reserve(&c, 100, "x") == 0 && b.reserve(&c, 1, "x") == 0);
  CHECK(Fake::log.empty() && b.ptr() == p && b.bytes() == 100);    // below capacity: no call at all
  CHECK(b.reserve(&c, 101, "x") == 0);
  CHECK(Fake::log == "sfa");                                       // a non-empty one: sync, free, alloc — exactly what was asked
  CHECK(b.bytes() == 101 && Fake::live == 1 && Fake::live_bytes == 101);
  Fake::reset_counts();
  Fake::fail_alloc_at = 1;
  CHECK(b.reserve(&c, 5000, "the test buffer") != 0);
  CHECK(Fake::log == "sfa" && !b && b.ptr() == nullptr && b.bytes() == 0 && Fake::live == 0);
  CHECK(c.err.find("the test buffer") != std::string::npos && c.err.find("5000") != std::string::npos);
  CHECK(b.reserve(&c, 5000, "the test buffer") == 0);             // the next call tries again
  CHECK(b && b.bytes() == 5000 && Fake::live == 1);
}

void check_move() {
  Ctx c;
  Buf a;
  CHECK(a.reserve(&c, 64, "a") == 0);
  void *p = a.ptr();
  Fake::reset_counts();
  Buf b(std::move(a));
  CHECK(!a && a.bytes() == 0 && b.ptr() == p && b.bytes() == 64 && Fake::log.empty() && Fake::live == 1);
  Buf d;
  d = std::move(b);
  CHECK(!b && d.ptr() == p && Fake::log.empty() && Fake::live == 1);
  Buf e;
  CHECK(e.reserve(&c, 8, "e") == 0 && Fake::live == 2);
  Fake::reset_counts();
  e = std::move(d);                                                // what the target held is freed, what moves is not
  CHECK(Fake::log == "f" && e.ptr() == p && Fake::live == 1);
  std::vector<Buf> v(3);
  v[1] = std::move(e);
  v.resize(40);                                                    // a growing vector moves its buffers
  CHECK(v[1].ptr() == p && Fake::live == 1);
}

// six tables and the scalar block that describes them, as mfa_mfcc_configure keeps them
struct Scalars { int win, shift, nfft, n; bool ready; };
struct Set { Buf t[6]; Scalars s{0, 0, 0, 0, false}; };

int upload(Ctx *c, Set &set, const std::vector<std::vector<float>> &h, const Scalars &s) {
  return dev_upload_commit<Fake>(c, "the tables",
                                 {{&set.t[0], h[0].data(), h[0].size() * 4}, {&set.t[1], h[1].data(), h[1].size() * 4},
                                  {&set.t[2], h[2].data(), h[2].size() * 4}, {&set.t[3], h[3].data(), h[3].size() * 4},
                                  {&set.t[4], h[4].data(), h[4].size() * 4}, {&set.t[5], h[5].data(), h[5].size() * 4}},
                                 [&] { set.s = s; });
}

void check_table_set() {
  Ctx c;
  std::vector<std::vector<float>> h1(6), h2(6);
  for (int i = 0; i < 6; i++) { h1[i].assign(3 + i, 1.0f + i); h2[i].assign(9 - i, -2.0f - i); }
  {
    Set set;
    Fake::reset_counts();
    CHECK(upload(&c, set, h1, {400, 160, 512, 7, true}) == 0);
    CHECK(Fake::log == "acacacacacac");                           // nothing to wait for or to free the first time
    CHECK(Fake::live == 6 && set.s.ready);
    for (int i = 0; i < 6; i++) CHECK(set.t[i].bytes() == h1[i].size() * 4 && memcmp(set.t[i].ptr(), h1[i].data(), h1[i].size() * 4) == 0);
    void *before[6];
    for (int i = 0; i < 6; i++) before[i] = set.t[i].ptr();
    const Scalars s_before = set.s;
    const int live_before = Fake::live;
    const size_t bytes_before = Fake::live_bytes;
    for (int step = 0; step < 12; step++) {                        // fail each allocation and each copy in turn
      Fake::reset_counts();
      if (step % 2 == 0) Fake::fail_alloc_at = step / 2 + 1; else Fake::fail_copy_at = step / 2 + 1;
      c.err.clear();
      CHECK(upload(&c, set, h2, {640, 320, 1024, 9, true}) != 0);
      CHECK(!c.err.empty());
      CHECK(Fake::log.find('s') == std::string::npos);            // nobody waited: nothing of the old set was touched
      for (int i = 0; i < 6; i++) {
        CHECK(set.t[i].ptr() == before[i] && set.t[i].bytes() == h1[i].size() * 4);
        CHECK(memcmp(set.t[i].ptr(), h1[i].data(), h1[i].size() * 4) == 0);
      }
      CHECK(memcmp(&set.s, &s_before, sizeof(Scalars)) == 0);
      CHECK(Fake::live == live_before && Fake::live_bytes == bytes_before);
    }
    Fake::reset_counts();
    CHECK(upload(&c, set, h2, {640, 320, 1024, 9, true}) == 0);
    CHECK(Fake::log == "acacacacacacsffffff");                    // the old set goes after the uploads and exactly one sync
    CHECK(Fake::live == 6 && set.s.win == 640 && set.s.n == 9);
    for (int i = 0; i < 6; i++) CHECK(set.t[i].bytes() == h2[i].size() * 4 && memcmp(set.t[i].ptr(), h2[i].data(), h2[i].size() * 4) == 0);
    // a table of no bytes empties its buffer (how a model without split operands, or a dropped statistics model, is stored)
    h2[4].clear();
    Fake::reset_counts();
    CHECK(upload(&c, set, h2, {640, 320, 1024, 10, true}) == 0);
    CHECK(Fake::log == "acacacacacsffffff" && Fake::live == 5 && !set.t[4] && set.t[5]);
  }
  CHECK(Fake::live == 0 && Fake::live_bytes == 0);                 // destructors free
}

}  // namespace

int main() {
  check_reserve();
  CHECK(Fake::live == 0);
  check_move();
  CHECK(Fake::live == 0);
  check_table_set();
  CHECK(Fake::live == 0 && Fake::live_bytes == 0);
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  puts("dev_buf: all checks passed");
  return 0;
}
