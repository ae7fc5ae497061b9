// Owned device memory of a context: one growable buffer type, and "upload a set of tables, then commit".
//
// Nothing here names HIP.  The four device operations come from a trait,
//   static int alloc(void **p, size_t bytes);                        0, or an error code
//   static void free(void *p);
//   static int copy_h2d(void *dst, const void *src, size_t bytes);   synchronous; 0, or an error code
//   static int sync(Stream s);                                       wait for the stream; 0, or an error code
//   static const char *describe(int code);
// which ctx.hpp fills in with the HIP calls (MfaBuf) and tests/native/dev_buf_check.cpp with a fake that counts.
// The context type needs a `stream` member and `int fail(const char *fmt, ...)` (stores the message, returns non-zero).
#pragma once
#include <cstddef>
#include <initializer_list>
#include <utility>
#include <vector>

template <class Dev>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { release(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
    return *this;
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }

  template <class T = void> T *ptr() const { return static_cast<T *>(p_); }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

  // Frees at once.  The caller knows that nothing enqueued still uses the memory.
  void release() {
    if (p_) Dev::free(p_);
    p_ = nullptr; bytes_ = 0;
  }

  // At least `bytes` of device memory; the contents are not kept.  With enough capacity this is no device call at all.
  // Otherwise: wait for ctx->stream (work in flight may use the old memory; an empty buffer has none), free, allocate
  // exactly `bytes`.  A failed allocation leaves the buffer empty and the context usable: the next call tries again.
  // (A failed wait frees nothing: the buffer stays as it was.)
  template <class Ctx>
  int reserve(Ctx *ctx, size_t bytes, const char *what) {
    if (bytes <= bytes_) return 0;
    if (p_) {
      if (int e = Dev::sync(ctx->stream)) return ctx->fail("waiting for the stream before %s grows failed: %s", what, Dev::describe(e));
      release();
    }
    if (int e = Dev::alloc(&p_, bytes)) {
      p_ = nullptr;
      return ctx->fail("allocation of %s (%zu bytes) failed: %s", what, bytes, Dev::describe(e));
    }
    bytes_ = bytes;
    return 0;
  }

 private:
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

// One table of a set: `bytes` at `host` replace what `dst` holds.  No bytes: `dst` ends up empty.
template <class Dev>
struct DevUpload {
  DevBuf<Dev> *dst;
  const void *host;
  size_t bytes;
};

struct DevNoCommit { void operator()() const {} };

// Replaces a set of tables as a whole.  Every table is uploaded into a fresh buffer first; a failure on the way frees
// those, runs no `commit` and leaves every `dst` — so the previous set — as it was.  Only then are the new buffers moved
// into place and `commit()` run (the scalar fields and the ready flag that describe the set; it cannot fail), and the
// previous buffers freed, after one wait for ctx->stream when there were any.
template <class Dev, class Ctx, class Commit = DevNoCommit>
int dev_upload_commit(Ctx *ctx, const char *what, std::initializer_list<DevUpload<Dev>> set, Commit commit = Commit()) {
  std::vector<DevBuf<Dev>> fresh(set.size());
  size_t i = 0;
  bool had_any = false;
  for (const DevUpload<Dev> &u : set) {
    DevBuf<Dev> &b = fresh[i++];
    had_any = had_any || *u.dst;
    if (u.bytes == 0) continue;
    if (b.reserve(ctx, u.bytes, what)) return -1;
    if (int e = Dev::copy_h2d(b.ptr(), u.host, u.bytes)) return ctx->fail("upload of %s (%zu bytes) failed: %s", what, u.bytes, Dev::describe(e));
  }
  if (had_any)
    if (int e = Dev::sync(ctx->stream)) return ctx->fail("waiting for the stream before %s are replaced failed: %s", what, Dev::describe(e));
  i = 0;
  for (const DevUpload<Dev> &u : set) std::swap(*u.dst, fresh[i++]);
  commit();
  return 0;   // `fresh` now holds the previous set and frees it
}
