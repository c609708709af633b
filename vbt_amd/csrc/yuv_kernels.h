// YUV 4:2:0 ingest: colour conversion fused into preprocess_image (include/vbt_hip.h, "pixel formats").
//
// A decoder emits NV12 or I420, not packed RGB (the reference's cv2.VideoCapture converts inside the decoder, track.py:135,160).  The
// kernel below reads the four source pixels of the bilinear resize straight from the planes, converts each to uint8 RGB with the
// integer BT.601 limited-range formula (20-bit fixed point, int32), and lerps them in float32 exactly as resize_bilinear_kernel
// (frames.hip) does - a full-resolution RGB frame is never written.  The result is, bit for bit,
// preprocess_image(rgb_from_yuv(frame)).  Packed 4:2:2 (YUYV / UYVY), 10-bit P010 and the other colour descriptions (BT.709, full
// range) run the template at the end of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.h"

namespace vbt {

struct Rgb8 { int r, g, b; };

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// R = clip8((1220542 Y' + 1673527 v + 2^19) >> 20) etc. with Y' = max(0, Y - 16), u = U - 128, v = V - 128; >> is arithmetic
__device__ __forceinline__ Rgb8 yuv_to_rgb8(int Y, int U, int V) {
  const int y = 1220542 * max(0, Y - 16) + (1 << 19), u = U - 128, v = V - 128;
  Rgb8 o;
  o.r = clip8((y + 1673527 * v) >> 20);
  o.g = clip8((y - 409993 * u - 852492 * v) >> 20);
  o.b = clip8((y + 2116026 * u) >> 20);
  return o;
}

// One thread per output pixel, consecutive lanes = consecutive output columns: a wave reads one luma row segment per source row
// (lanes W / w bytes apart, neighbouring lanes within the same cache lines) and the chroma row under it.
// Source frame b starts at src + b * frame_stride.  Whole frame (compact == 0): luma row y at y * W.  Compact (the host-fed upload,
// upload_plan.h): luma holds only the row pairs the resize reads, pair oy = source rows p, p + 1 (p = min(y0, H - 2)) at row 2 oy.
// Either way the chroma plane(s) start at chroma_off, whole, in the layout of the format: NV12 [H/2][W] interleaved U,V;
// I420 [H/2][W/2] U then [H/2][W/2] V.  The chroma sample of source pixel (y, x) is the one at (y >> 1, x >> 1), taken nearest.
__global__ __launch_bounds__(256) void yuv_resize_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long total, int H, int W,
                                                         int h, int w, float sy, float sx, int pix_fmt, long frame_stride, long chroma_off,
                                                         int compact) {
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
  const uint8_t* s = src + b * frame_stride;
  const uint8_t* cp = s + chroma_off;
  int ly0 = y0, ly1 = y1;   // luma rows as the source buffer holds them
  if (compact) {
    const int p = min(y0, H - 2);
    ly0 = 2 * oy + (y0 - p);
    ly1 = 2 * oy + (y1 - p);
  }
  const int ys[2] = {y0, y1}, lys[2] = {ly0, ly1}, xs[2] = {x0, x1};
  Rgb8 px[2][2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int Y = s[(long)lys[j] * W + xs[i]];
      int U, V;
      if (pix_fmt == VBT_PIX_NV12) {
        const uint8_t* c = cp + (long)(ys[j] >> 1) * W + (xs[i] & ~1);
        U = c[0];
        V = c[1];
      } else {
        const long ci = (long)(ys[j] >> 1) * (W >> 1) + (xs[i] >> 1);
        U = cp[ci];
        V = cp[(long)(H >> 1) * (W >> 1) + ci];
      }
      px[j][i] = yuv_to_rgb8(Y, U, V);
    }
  }
  uint8_t* d = dst + ((b * h + oy) * (long)w + ox) * 3;
  const int tlc[3] = {px[0][0].r, px[0][0].g, px[0][0].b}, trc[3] = {px[0][1].r, px[0][1].g, px[0][1].b};
  const int blc[3] = {px[1][0].r, px[1][0].g, px[1][0].b}, brc[3] = {px[1][1].r, px[1][1].g, px[1][1].b};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float tl = (float)tlc[c], tr = (float)trc[c];
    float bl = (float)blc[c], br = (float)brc[c];
    float top = tl + (tr - tl) * lx;
    float bot = bl + (br - bl) * lx;
    float v = top + (bot - top) * ly;
    d[c] = (uint8_t)(int)v;
  }
}

// ---- every YUV format under a colour description (include/vbt_hip.h, "more source formats") ----
// The kernel above is what NV12 / I420 run under (BT.601, limited); everything else runs the template below: the layout is a template
// argument, the colour description a by-value struct - uniform across the launch, so its seven words stay in scalar registers.
__device__ __forceinline__ Rgb8 yuv_to_rgb8(int Y, int U, int V, const YuvColour& cc) {
  const int y = cc.cy * max(0, Y - cc.yoff) + (1 << 19), u = U - cc.coff, v = V - cc.coff;
  Rgb8 o;
  o.r = clip8((y + cc.crv * v) >> 20);
  o.g = clip8((y - cc.cgu * u - cc.cgv * v) >> 20);
  o.b = clip8((y + cc.cbu * u) >> 20);
  return o;
}

// Source pixel (y, x) of a frame at s; ly: the row of the buffer that holds luma row y (ly == y in a whole frame); cp: the chroma plane(s).
//   YUYV / UYVY: rows of 2W bytes; ONE aligned dword holds the pixel pair, Y0 U Y1 V or U Y0 V Y1 - luma and both chroma samples.
//   P010: rows of W 16-bit words; a 16-bit luma load and one dword for the U,V pair at (y >> 1, x >> 1); the sample is word >> 6.
//   NV12 / I420: as the kernel above.
template <int FMT>
__device__ __forceinline__ Rgb8 load_pixel(const uint8_t* __restrict__ s, const uint8_t* __restrict__ cp, int y, int ly, int x, int H, int W,
                                           const YuvColour& cc) {
  int Y, U, V;
  if constexpr (FMT == VBT_PIX_YUYV422 || FMT == VBT_PIX_UYVY422) {
    const uint32_t q = *(const uint32_t*)(s + (long)ly * 2 * W + (long)(x >> 1) * 4);
    const int odd = x & 1;
    if constexpr (FMT == VBT_PIX_YUYV422) {
      Y = (q >> (odd ? 16 : 0)) & 255;
      U = (q >> 8) & 255;
      V = q >> 24;
    } else {
      Y = (q >> (odd ? 24 : 8)) & 255;
      U = q & 255;
      V = (q >> 16) & 255;
    }
  } else if constexpr (FMT == VBT_PIX_P010) {
    Y = *(const uint16_t*)(s + ((long)ly * W + x) * 2) >> 6;
    const uint32_t q = *(const uint32_t*)(cp + ((long)(y >> 1) * W + (x & ~1)) * 2);
    U = (q & 0xffff) >> 6;
    V = q >> 22;
  } else if constexpr (FMT == VBT_PIX_NV12) {
    Y = s[(long)ly * W + x];
    const uint8_t* c = cp + (long)(y >> 1) * W + (x & ~1);
    U = c[0];
    V = c[1];
  } else {
    static_assert(FMT == VBT_PIX_I420, "unknown layout");
    Y = s[(long)ly * W + x];
    const long ci = (long)(y >> 1) * (W >> 1) + (x >> 1);
    U = cp[ci];
    V = cp[(long)(H >> 1) * (W >> 1) + ci];
  }
  return yuv_to_rgb8(Y, U, V, cc);
}

// One thread per output pixel, the geometry and the float32 arithmetic of yuv_resize_kernel.  compact: rows y0, y1 of the frame sit at
// rows 2 oy + (y - p) of the buffer, p = min(y0, H - 2) - for the formats with a chroma plane in the luma part only, as above; for
// 4:2:2 the buffer is [2h] packed rows and nothing else (every row carries its own chroma).
template <int FMT>
__global__ __launch_bounds__(256) void pix_resize_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long total, int H, int W, int h,
                                                         int w, float sy, float sx, YuvColour cc, long frame_stride, long chroma_off, int compact) {
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
  const uint8_t* s = src + b * frame_stride;
  const uint8_t* cp = s + chroma_off;
  int ly0 = y0, ly1 = y1;
  if (compact) {
    const int p = min(y0, H - 2);
    ly0 = 2 * oy + (y0 - p);
    ly1 = 2 * oy + (y1 - p);
  }
  const Rgb8 tl = load_pixel<FMT>(s, cp, y0, ly0, x0, H, W, cc), tr = load_pixel<FMT>(s, cp, y0, ly0, x1, H, W, cc);
  const Rgb8 bl = load_pixel<FMT>(s, cp, y1, ly1, x0, H, W, cc), br = load_pixel<FMT>(s, cp, y1, ly1, x1, H, W, cc);
  uint8_t* d = dst + ((b * h + oy) * (long)w + ox) * 3;
  const int tlc[3] = {tl.r, tl.g, tl.b}, trc[3] = {tr.r, tr.g, tr.b}, blc[3] = {bl.r, bl.g, bl.b}, brc[3] = {br.r, br.g, br.b};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float ftl = (float)tlc[c], ftr = (float)trc[c];
    float fbl = (float)blc[c], fbr = (float)brc[c];
    float top = ftl + (ftr - ftl) * lx;
    float bot = fbl + (fbr - fbl) * lx;
    float v = top + (bot - top) * ly;
    d[c] = (uint8_t)(int)v;
  }
}

}  // namespace vbt
