// lslam_buf.hpp -- the library's grow-only buffers (host side only): device memory (DevBuf) and page-locked host memory
// (PinBuf).  A buffer belongs to the object it is a member of and is released by its destructor: a context, a map, an odometry
// node frees what it allocated when it is destroyed -- once nothing enqueued on its streams can still touch the memory (the
// owner waits for them first).  One growth rule for every buffer: n + n / 4 + 256 elements.
// reserve(n) is for what grows and applies that rule; alloc(n) is for what is sized once, when its owner is made (a map's rings,
// a pose graph's arrays, hash tables): exactly n elements, so a container the user sized keeps the footprint they asked for.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace lslam {

inline size_t buf_grown(size_t n) { return n + n / 4 + 256; }

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t cap = 0;
  bool borrowed = false;  // p points into another allocation (adopt): never freed here, dropped by the next reserve
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed) { o.forget(); }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p; cap = o.cap; borrowed = o.borrowed;
      o.forget();
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void adopt(T *ptr, size_t n) {
    release();
    p = ptr;
    cap = n;
    borrowed = true;
  }
  // exactly max(n, 1) elements, whatever was held before
  hipError_t alloc(size_t n) {
    release();
    const size_t want = n ? n : 1;
    hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    else p = nullptr;
    return e;
  }
  // room for n elements; the contents are lost when the buffer grows
  hipError_t reserve(size_t n) { return n <= cap ? hipSuccess : alloc(buf_grown(n)); }
  // grow, keeping the first `keep` elements (copied on `s`, waited for)
  hipError_t grow(size_t n, size_t keep, hipStream_t s) {
    if (n <= cap) return hipSuccess;
    DevBuf q;
    hipError_t e = q.reserve(n);
    if (e != hipSuccess) return e;
    if (keep && p) {
      e = hipMemcpyAsync(q.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    *this = static_cast<DevBuf &&>(q);
    return e;
  }
  void release() {
    if (p && !borrowed) (void)hipFree(p);
    forget();
  }

 private:
  void forget() {
    p = nullptr;
    cap = 0;
    borrowed = false;
  }
};

// a pinned host block that lives as long as its owner: asynchronous copies to and from it need no wait to keep their host side
// alive (a std::vector local does), and they run at the link's rate instead of through the runtime's staging
template <typename T>
struct PinBuf {
  T *p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf &) = delete;
  PinBuf &operator=(const PinBuf &) = delete;
  PinBuf(PinBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  PinBuf &operator=(PinBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p; cap = o.cap;
      o.p = nullptr; o.cap = 0;
    }
    return *this;
  }
  ~PinBuf() { release(); }
  hipError_t alloc(size_t n) {
    release();
    const size_t want = n ? n : 1;
    hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    else p = nullptr;
    return e;
  }
  hipError_t reserve(size_t n) { return n <= cap ? hipSuccess : alloc(buf_grown(n)); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace lslam
