// Frame plumbing in front of the detector (gfx950): assembling a detector batch from frames that live in different
// places of device memory (HBM-bound byte moves: 16 bytes per lane, consecutive lanes on consecutive addresses), and the two
// entries of preprocess_image: the bilinear resize of RGB frames and its YUV twins (yuv_kernels.h: NV12 / I420 -> RGB fused
// into the same resize; packed 4:2:2, P010 and the BT.709 / full-range descriptions through one template per layout).
#include <dlfcn.h>

#include "common.h"
#include "dev_mem.h"
#include "yuv_kernels.h"

namespace vbt {

constexpr int GATHER_FRAMES = 64;
struct GatherMeta {
  const uint8_t* src[GATHER_FRAMES];
};

// grid = (chunks, frames): workgroup (x, y) copies 256 x 16-byte pieces x `per` of frame y
__global__ __launch_bounds__(256) void gather_frames_kernel(uint4* __restrict__ dst, GatherMeta meta, size_t frame_vec, int per) {
  const uint4* __restrict__ s = (const uint4*)meta.src[blockIdx.y];
  uint4* __restrict__ d = dst + (size_t)blockIdx.y * frame_vec;
  size_t i = ((size_t)blockIdx.x * per) * 256 + threadIdx.x;
#pragma unroll 4
  for (int k = 0; k < per; k++, i += 256)
    if (i < frame_vec) d[i] = s[i];
}

// ------------------------------------------------------------------------------------------
// preprocess_image (reference odt.py:10-19): tf.image.resize bilinear with half-pixel centres
// [EXTERNAL TF2 ResizeBilinear: in = (out+0.5)*scale-0.5, lower = max(floor(in),0),
// upper = min(ceil(in), size-1), lerp = in - floor(in); top + (bottom-top)*ly], float32,
// then tf.cast(..., uint8) = truncation.  Optional BGR->RGB swap (reference track.py:171).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              long total, int H, int W, int h, int w, float sy, float sx,
                                                              int swap_rb, int compact) {
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  int ox = (int)(idx % w);
  long t = idx / w;
  int oy = (int)(t % h);
  long b = t / h;
  float iy = ((float)oy + 0.5f) * sy - 0.5f, ix = ((float)ox + 0.5f) * sx - 0.5f;
  float fy = floorf(iy), fx = floorf(ix);
  int y0 = max((int)fy, 0), y1 = min((int)ceilf(iy), H - 1);
  int x0 = max((int)fx, 0), x1 = min((int)ceilf(ix), W - 1);
  float ly = iy - fy, lx = ix - fx;
  // compact: the source holds only the row pairs the resize reads, [B][2h][W][3]: pair oy = source rows p, p + 1 with p = min(y0, H - 2)
  // (the host-fed pipeline uploads nothing else: the compact layout, upload_plan.h); y0 and y1 then become rows 2 oy + (y - p)
  const uint8_t* s = src + b * (long)(compact ? 2 * h : H) * W * 3;
  if (compact) {
    const int p = min(y0, H - 2);
    y0 = 2 * oy + (y0 - p);
    y1 = 2 * oy + (y1 - p);
  }
  uint8_t* d = dst + ((b * h + oy) * (long)w + ox) * 3;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float tl = (float)s[((long)y0 * W + x0) * 3 + c], tr = (float)s[((long)y0 * W + x1) * 3 + c];
    float bl = (float)s[((long)y1 * W + x0) * 3 + c], br = (float)s[((long)y1 * W + x1) * 3 + c];
    float top = tl + (tr - tl) * lx;
    float bot = bl + (br - bl) * lx;
    float v = top + (bot - top) * ly;
    d[swap_rb ? 2 - c : c] = (uint8_t)(int)v;
  }
}

int resize_frames_dev(const uint8_t* src_dev, int B, int H, int W, uint8_t* dst_dev, int h, int w, int swap_rb, int compact, hipStream_t st) {
  if (compact && H < 2) { set_error("resize: compact rows need a source of at least two rows"); return VBT_ERR_ARG; }
  const long total = (long)B * h * w;
  const float sy = (float)H / (float)h, sx = (float)W / (float)w;
  resize_bilinear_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(src_dev, dst_dev, total, H, W, h, w, sy, sx, swap_rb, compact);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

int resize_frames_yuv_dev(const uint8_t* src_dev, int B, int H, int W, int pix_fmt, size_t frame_stride, size_t chroma_off, int compact,
                          uint8_t* dst_dev, int h, int w, hipStream_t st) {
  if (!pix_fmt_is_yuv(pix_fmt) || H < 2 || W < 2 || (H & 1) || (W & 1)) { set_error("resize: YUV 4:2:0 needs NV12 / I420 and even H, W >= 2"); return VBT_ERR_ARG; }
  const long total = (long)B * h * w;
  const float sy = (float)H / (float)h, sx = (float)W / (float)w;
  yuv_resize_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(src_dev, dst_dev, total, H, W, h, w, sy, sx, pix_fmt, (long)frame_stride,
                                                                           (long)chroma_off, compact);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

bool yuv_colour(int pix_fmt, int matrix, int range, YuvColour* c) {
  if (!pix_fmt_is_source_yuv(pix_fmt) || (matrix != VBT_CS_BT601 && matrix != VBT_CS_BT709) || (range != VBT_RANGE_LIMITED && range != VBT_RANGE_FULL))
    return false;
  // [matrix][depth][range] = CY, CRV, CGU, CGV, CBU (include/vbt_hip.h; tests/test_pixfmt_host.py re-derives the rows)
  static const int tab[2][2][2][5] = {
      {{{1220542, 1673527, 409993, 852492, 2116026}, {1048576, 1470104, 360853, 748826, 1858077}},
       {{305236, 418389, 102698, 213115, 528805}, {261375, 366448, 89949, 186658, 463157}}},
      {{{1220945, 1879825, 223607, 558796, 2215014}, {1048576, 1651297, 196424, 490864, 1945738}},
       {{305236, 469956, 55902, 139699, 553753}, {261375, 411614, 48962, 122356, 485008}}}};
  const int deep = pix_fmt == VBT_PIX_P010;
  const int* t = tab[matrix][deep][range];
  *c = YuvColour{t[0], t[1], t[2], t[3], t[4], range == VBT_RANGE_FULL ? 0 : (deep ? 64 : 16), deep ? 512 : 128};
  return true;
}

int resize_frames_pix_dev(const uint8_t* src_dev, int B, int H, int W, int pix_fmt, int matrix, int range, size_t frame_stride, size_t chroma_off,
                          int compact, uint8_t* dst_dev, int h, int w, hipStream_t st) {
  YuvColour cc;
  if (!yuv_colour(pix_fmt, matrix, range, &cc) || !pix_layout(pix_fmt, H, W).ok || (compact && H < 2)) {
    set_error("resize: pixel format %d, matrix %d, range %d does not take %d x %d frames", pix_fmt, matrix, range, H, W);
    return VBT_ERR_ARG;
  }
  if (pix_fmt_is_yuv(pix_fmt) && matrix == VBT_CS_BT601 && range == VBT_RANGE_LIMITED)
    return resize_frames_yuv_dev(src_dev, B, H, W, pix_fmt, frame_stride, chroma_off, compact, dst_dev, h, w, st);
  if (!pix_fmt_is_yuv(pix_fmt) && (((uintptr_t)src_dev | frame_stride | chroma_off) & 3)) {
    set_error("resize: a source of pixel format %d must be 4-byte aligned", pix_fmt);
    return VBT_ERR_ARG;
  }
  const long total = (long)B * h * w;
  const float sy = (float)H / (float)h, sx = (float)W / (float)w;
  const dim3 grid((unsigned)((total + 255) / 256));
#define VBT_PIX_LAUNCH(FMT) \
  pix_resize_kernel<FMT><<<grid, 256, 0, st>>>(src_dev, dst_dev, total, H, W, h, w, sy, sx, cc, (long)frame_stride, (long)chroma_off, compact)
  switch (pix_fmt) {
    case VBT_PIX_NV12: VBT_PIX_LAUNCH(VBT_PIX_NV12); break;
    case VBT_PIX_I420: VBT_PIX_LAUNCH(VBT_PIX_I420); break;
    case VBT_PIX_YUYV422: VBT_PIX_LAUNCH(VBT_PIX_YUYV422); break;
    case VBT_PIX_UYVY422: VBT_PIX_LAUNCH(VBT_PIX_UYVY422); break;
    default: VBT_PIX_LAUNCH(VBT_PIX_P010); break;
  }
#undef VBT_PIX_LAUNCH
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

// ---- roctx ranges (common.h): resolved lazily with dlopen, so that the library has no link-time dependency on the profiler SDK ----
static int (*g_roctx_push)(const char*) = nullptr;
static int (*g_roctx_pop)() = nullptr;
static int g_roctx_state = 0;   // 0 = not tried, 1 = on, -1 = off
static bool roctx_ready() {
  if (g_roctx_state == 0) {
    g_roctx_state = -1;
    const char* e = getenv("VBT_ROCTX");
    if (e && e[0] == '1') {
      void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
      if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
      if (h) {
        g_roctx_push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        g_roctx_pop = (int (*)())dlsym(h, "roctxRangePop");
        if (g_roctx_push && g_roctx_pop) g_roctx_state = 1;
      }
    }
  }
  return g_roctx_state == 1;
}
RoctxRange::RoctxRange(const char* name) : on(roctx_ready()) { if (on) g_roctx_push(name); }
RoctxRange::~RoctxRange() { if (on) g_roctx_pop(); }

}  // namespace vbt

using namespace vbt;

extern "C" int vbt_gather_frames(uint8_t* dst_dev, const uint8_t* const* src_frames_host, int n_frames, size_t frame_bytes, void* stream) {
  if (!dst_dev || !src_frames_host || n_frames < 1 || frame_bytes < 16 || (frame_bytes & 15) != 0 || ((uintptr_t)dst_dev & 15) != 0) {
    set_error("vbt_gather_frames: bad argument (frame_bytes must be a positive multiple of 16, pointers 16-byte aligned)");
    return VBT_ERR_ARG;
  }
  for (int i = 0; i < n_frames; i++)
    if (!src_frames_host[i] || ((uintptr_t)src_frames_host[i] & 15) != 0) { set_error("vbt_gather_frames: source %d is NULL or misaligned", i); return VBT_ERR_ARG; }
  const size_t vec = frame_bytes / 16;
  const int per = 4;
  const unsigned chunks = (unsigned)((vec + 256 * per - 1) / (256 * per));
  for (int f0 = 0; f0 < n_frames; f0 += GATHER_FRAMES) {
    const int nb = std::min(GATHER_FRAMES, n_frames - f0);
    GatherMeta meta;
    for (int i = 0; i < nb; i++) meta.src[i] = src_frames_host[f0 + i];
    for (int i = nb; i < GATHER_FRAMES; i++) meta.src[i] = nullptr;
    gather_frames_kernel<<<dim3(chunks, (unsigned)nb), 256, 0, (hipStream_t)stream>>>((uint4*)(dst_dev + (size_t)f0 * frame_bytes), meta, vec, per);
  }
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

extern "C" int vbt_resize_frames(const uint8_t* src, int B, int H, int W, int src_on_device, uint8_t* dst, int h, int w, int dst_on_device,
                                 int swap_rb, int device, void* stream) {
  if (!src || !dst || B < 1 || H < 1 || W < 1 || h < 1 || w < 1) { set_error("vbt_resize_frames: bad argument"); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_resize_frames", device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  size_t sb = (size_t)B * H * W * 3, db = (size_t)B * h * w * 3;
  DevBuf<uint8_t> ds, dd;   // freed when the function returns: after the stream synchronisation, or - on an error - by a hipFree that waits
  const uint8_t* sp = src;
  uint8_t* dp = dst;
  if (!src_on_device) {
    VBT_HIP_CHECK(ds.alloc(sb));
    VBT_HIP_CHECK(hipMemcpyAsync(ds.get(), src, sb, hipMemcpyHostToDevice, st));
    sp = ds.get();
  }
  if (!dst_on_device) {
    VBT_HIP_CHECK(dd.alloc(db));
    dp = dd.get();
  }
  hipError_t e = resize_frames_dev(sp, B, H, W, dp, h, w, swap_rb, 0, st) == VBT_OK ? hipSuccess : hipErrorLaunchFailure;
  if (e == hipSuccess && !dst_on_device) e = hipMemcpyAsync(dst, dd.get(), db, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && (ds || dd)) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { set_error("vbt_resize_frames failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  return VBT_OK;
}

extern "C" int vbt_resize_frames_yuv(const uint8_t* src, int B, int H, int W, int pix_fmt, int src_on_device, uint8_t* dst, int h, int w, int dst_on_device,
                          int device, void* stream) {
  if (!src || !dst || B < 1 || H < 1 || W < 1 || h < 1 || w < 1) { set_error("vbt_resize_frames_yuv: bad argument"); return VBT_ERR_ARG; }
  if (pix_fmt == VBT_PIX_RGB24) { set_error("vbt_resize_frames_yuv: VBT_PIX_RGB24 frames go through vbt_resize_frames"); return VBT_ERR_ARG; }
  if (!pix_fmt_is_yuv(pix_fmt)) { set_error("vbt_resize_frames_yuv: unknown pixel format %d", pix_fmt); return VBT_ERR_ARG; }
  if ((H & 1) || (W & 1)) { set_error("vbt_resize_frames_yuv: YUV 4:2:0 frames have even H and W, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_resize_frames_yuv", device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t fb = (size_t)H * W * 3 / 2, sb = (size_t)B * fb, db = (size_t)B * h * w * 3;
  // every failure below goes through the one clean-up; rc keeps the error a callee already described
  DevBuf<uint8_t> ds, dd;
  hipError_t e = hipSuccess;
  int rc = VBT_OK;
  if (!src_on_device) {
    e = ds.alloc(sb);
    if (e == hipSuccess) e = hipMemcpyAsync(ds.get(), src, sb, hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess && !dst_on_device) e = dd.alloc(db);
  if (e == hipSuccess) rc = resize_frames_yuv_dev(ds ? ds.get() : src, B, H, W, pix_fmt, fb, (size_t)H * W, 0, dd ? dd.get() : dst, h, w, st);
  if (e == hipSuccess && rc == VBT_OK && !dst_on_device) e = hipMemcpyAsync(dst, dd.get(), db, hipMemcpyDeviceToHost, st);
  if (ds || dd) {   // (also after a failure: a copy may still be in flight on the buffers freed when the function returns)
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
  }
  if (e != hipSuccess) { set_error("vbt_resize_frames_yuv failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  return rc;
}

extern "C" size_t vbt_pix_frame_bytes(int H, int W, int pix_fmt) {
  return pix_fmt_takes(pix_fmt, H, W) ? pix_layout(pix_fmt, H, W).frame_bytes : 0;
}

extern "C" int vbt_resize_frames_pix(const void* src, int B, int H, int W, int pix_fmt, int matrix, int range, int src_on_device, uint8_t* dst, int h,
                                     int w, int dst_on_device, int device, void* stream) {
  if (!src || !dst || B < 1 || h < 1 || w < 1) { set_error("vbt_resize_frames_pix: bad argument (src, dst, B, h or w)"); return VBT_ERR_ARG; }
  if (pix_fmt == VBT_PIX_RGB24) { set_error("vbt_resize_frames_pix: pix_fmt VBT_PIX_RGB24 frames go through vbt_resize_frames"); return VBT_ERR_ARG; }
  if (!pix_fmt_is_source_yuv(pix_fmt)) { set_error("vbt_resize_frames_pix: unknown pix_fmt %d", pix_fmt); return VBT_ERR_ARG; }
  if (matrix != VBT_CS_BT601 && matrix != VBT_CS_BT709) { set_error("vbt_resize_frames_pix: unknown matrix %d", matrix); return VBT_ERR_ARG; }
  if (range != VBT_RANGE_LIMITED && range != VBT_RANGE_FULL) { set_error("vbt_resize_frames_pix: unknown range %d", range); return VBT_ERR_ARG; }
  const PixLayout l = pix_layout(pix_fmt, H, W);
  if (!l.ok || H > 16384 || W > 16384) {   // (this entry point takes no side above 16384 in any format)
    set_error("vbt_resize_frames_pix: pix_fmt %d does not take a size of %d x %d (H x W; 4:2:0 and P010: both even, 4:2:2: W even; 1..16384)", pix_fmt, H, W);
    return VBT_ERR_ARG;
  }
  if (src_on_device && !pix_fmt_is_yuv(pix_fmt) && ((uintptr_t)src & 3)) {
    set_error("vbt_resize_frames_pix: a device src of pix_fmt %d must be 4-byte aligned", pix_fmt);
    return VBT_ERR_ARG;
  }
  if (int rc = use_device("vbt_resize_frames_pix", device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t fb = l.frame_bytes, sb = (size_t)B * fb, db = (size_t)B * h * w * 3;
  // every failure below goes through the one clean-up; rc keeps the error a callee already described
  DevBuf<uint8_t> ds, dd;
  hipError_t e = hipSuccess;
  int rc = VBT_OK;
  if (!src_on_device) {
    e = ds.alloc(sb);
    if (e == hipSuccess) e = hipMemcpyAsync(ds.get(), src, sb, hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess && !dst_on_device) e = dd.alloc(db);
  if (e == hipSuccess)
    rc = resize_frames_pix_dev(ds ? ds.get() : (const uint8_t*)src, B, H, W, pix_fmt, matrix, range, fb, l.chroma_plane ? (size_t)H * l.row : 0, 0,
                               dd ? dd.get() : dst, h, w, st);
  if (e == hipSuccess && rc == VBT_OK && !dst_on_device) e = hipMemcpyAsync(dst, dd.get(), db, hipMemcpyDeviceToHost, st);
  if (ds || dd) {   // (also after a failure: a copy may still be in flight on the buffers freed when the function returns)
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
  }
  if (e != hipSuccess) { set_error("vbt_resize_frames_pix failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  return rc;
}
