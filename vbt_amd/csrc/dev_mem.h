// Owners of device and pinned host memory (host code only): a buffer is freed when its owner goes out of scope, so an entry point that
// leaves early - VBT_HIP_CHECK returns - frees what it had allocated.  hipFree waits for the device: a scope that ends after its last
// blocking copy or synchronisation frees exactly where a hand-written hipFree stood.  Nothing else lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace vbt {

template <class T, bool PINNED>
class OwnedBuf {   // move-only
 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  ~OwnedBuf() { reset(); }
  // room for `count` elements; what the buffer held before is freed first.  After a failure the buffer is empty.
  hipError_t alloc(size_t count) { return alloc_impl(count, hipHostMallocDefault); }
  // pinned memory only: hipHostMalloc's flags (mapped, coherent, ...)
  hipError_t alloc(size_t count, unsigned flags) {
    static_assert(PINNED, "device memory takes no allocation flags");
    return alloc_impl(count, flags);
  }
  void reset() {
    if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
  }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  hipError_t alloc_impl(size_t count, unsigned flags) {
    reset();
    void* p = nullptr;
    const hipError_t e = PINNED ? hipHostMalloc(&p, sizeof(T) * count, flags) : hipMalloc(&p, sizeof(T) * count);
    if (e == hipSuccess) p_ = (T*)p;
    return e;
  }
  T* p_ = nullptr;
};
template <class T> using DevBuf = OwnedBuf<T, false>;    // hipMalloc / hipFree
template <class T> using PinnedBuf = OwnedBuf<T, true>;  // hipHostMalloc / hipHostFree

// A device block and its pinned host copy: a pack kernel fills dev(), fetch() brings it to host() with one stream-ordered copy and
// one synchronisation of that stream.
class Mirror {
 public:
  Mirror() = default;
  Mirror(const Mirror&) = delete;   // (neither copied nor moved: it lives in its handle)
  // room for `bytes` in both; grows, never shrinks.  After a failure bytes() is 0 and a later reserve starts afresh; dev() tells
  // which half failed (null: the device block, else the pinned one).
  hipError_t reserve(size_t bytes) {
    if (bytes <= bytes_) return hipSuccess;
    reset();
    hipError_t e = dev_.alloc(bytes);
    if (e == hipSuccess) e = host_.alloc(bytes);
    if (e == hipSuccess) bytes_ = bytes;
    return e;
  }
  hipError_t fetch(size_t bytes, hipStream_t st) {
    const hipError_t e = hipMemcpyAsync(host_.get(), dev_.get(), bytes, hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
  }
  void reset() { dev_.reset(); host_.reset(); bytes_ = 0; }
  unsigned char* dev() const { return dev_.get(); }
  unsigned char* host() const { return host_.get(); }
  size_t bytes() const { return bytes_; }

 private:
  DevBuf<unsigned char> dev_;
  PinnedBuf<unsigned char> host_;
  size_t bytes_ = 0;
};

}  // namespace vbt
