// Owners of HIP events and streams (host code only), the siblings of dev_mem.h's buffers: a handle is destroyed when its owner goes out
// of scope, so an entry point that leaves early - VBT_HIP_CHECK returns - destroys what it had created.  Nothing else lives here.
#pragma once
#include <hip/hip_runtime.h>

namespace vbt {

template <class H, hipError_t (*CREATE)(H*, unsigned), hipError_t (*DESTROY)(H)>
class OwnedHandle {   // move-only
 public:
  OwnedHandle() = default;
  OwnedHandle(OwnedHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  OwnedHandle& operator=(OwnedHandle&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  ~OwnedHandle() { reset(); }
  // what the owner held before is destroyed first.  After a failure the owner is empty.
  hipError_t create(unsigned flags) {
    reset();
    H h = nullptr;
    const hipError_t e = CREATE(&h, flags);
    if (e == hipSuccess) h_ = h;
    return e;
  }
  void reset() {
    if (h_) (void)DESTROY(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }

 private:
  H h_ = nullptr;
};
using Event = OwnedHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;      // create(hipEventDefault) = hipEventCreate
using Stream = OwnedHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

}  // namespace vbt
