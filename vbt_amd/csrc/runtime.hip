// Library-wide plumbing of libvbt_hip.so, used by every unit: the per-thread error text, the device check, the per-device opt-in for more
// than 64 KB of dynamic LDS, and the streams and the memory the library hands to its callers.  (roctx ranges: frames.hip.)
#include <chrono>

#include "common.h"

namespace vbt {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int use_device(const char* fn, int device, bool set_current) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    set_error("%s: HIP device %d not available (%d visible) - no CPU fallback", fn, device, ndev);
    return VBT_ERR_HIP;
  }
  if (set_current) VBT_HIP_CHECK(hipSetDevice(device));
  return VBT_OK;
}

bool lds_opt_in(const void* fn, LdsOptIn* state) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_error("lds_opt_in: no current HIP device"); return false; }
  if (state->dev[dev] > 0) return true;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("device %d refuses more than 64 KB of dynamic LDS for a kernel that needs it: %s", dev, hipGetErrorString(e));
    return false;
  }
  state->dev[dev] = 1;
  return true;
}

}  // namespace vbt

using namespace vbt;

extern "C" {

const char* vbt_last_error(void) { return vbt::g_err; }

int vbt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// A HIP stream gets its hardware queue at its FIRST command, round-robin over GPU_MAX_HW_QUEUES (rocprofv3 Queue_Id).  Streams
// drawn from a framework's pool may have been used before, so a pipeline's streams can land on one queue and serialise
// (measured: 89 k -> 58 k frames/s).  Streams created here run one empty launch at once: streams created back to back sit on
// consecutive queues.
__global__ void stream_touch_kernel() {}
int vbt_stream_create(int device, void** stream_out) {
  if (!stream_out) { set_error("vbt_stream_create: NULL argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(device));
  hipStream_t st = nullptr;
  VBT_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  stream_touch_kernel<<<1, 64, 0, st>>>();
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipStreamDestroy(st); set_error("vbt_stream_create: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  *stream_out = (void*)st;
  return VBT_OK;
}
// Do two streams share a hardware queue?  A single-wave kernel that spins for `us` microseconds on each: side by side they
// take `us`, on one in-order queue 2 x `us`.  (The queue of a stream cannot be queried; GPU otherwise idle when called.)
__global__ void stream_spin_kernel(long ticks) {
  const long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
int vbt_streams_share_queue(void* a, void* b, int us, int* shared) {
  if (!a || !b || !shared || us < 20 || us > 100000) { set_error("vbt_streams_share_queue: bad argument"); return VBT_ERR_ARG; }
  const long ticks = (long)us * 100;   // wall_clock64: 100 MHz
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)a));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)b));
  auto t0 = std::chrono::steady_clock::now();
  stream_spin_kernel<<<1, 64, 0, (hipStream_t)a>>>(ticks);
  stream_spin_kernel<<<1, 64, 0, (hipStream_t)b>>>(ticks);
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)a));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)b));
  const double el = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  *shared = el > 1.6 * us ? 1 : 0;
  return VBT_OK;
}
int vbt_stream_destroy(void* stream) {
  if (!stream) return VBT_OK;
  VBT_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
  return VBT_OK;
}

// Memory and synchronisation for callers without a framework.  What vbt_host_alloc and vbt_device_alloc give belongs to the caller until
// it hands it back: no owner of dev_mem.h can hold it.
int vbt_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) { set_error("vbt_host_alloc: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return VBT_OK;
}
int vbt_host_free(void* ptr) {
  if (ptr) VBT_HIP_CHECK(hipHostFree(ptr));
  return VBT_OK;
}
int vbt_device_alloc(int device, size_t bytes, void** out) {
  if (!out || bytes == 0) { set_error("vbt_device_alloc: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(device));
  VBT_HIP_CHECK(hipMalloc(out, bytes));
  return VBT_OK;
}
int vbt_device_free(void* ptr) {
  if (ptr) VBT_HIP_CHECK(hipFree(ptr));
  return VBT_OK;
}
int vbt_memcpy(void* dst, const void* src, size_t bytes, int kind) {
  if (!dst || !src || kind < 0 || kind > 1) { set_error("vbt_memcpy: bad argument"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipMemcpy(dst, src, bytes, kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
  return VBT_OK;
}
int vbt_stream_synchronize(void* stream) {
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return VBT_OK;
}
int vbt_device_synchronize(int device) {
  VBT_HIP_CHECK(hipSetDevice(device));
  VBT_HIP_CHECK(hipDeviceSynchronize());
  return VBT_OK;
}

}  // extern "C"
