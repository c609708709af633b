// How a source frame lies in memory, how it lies in a staging buffer - whole or compact - and the copies that bring a batch of host
// frames there.  Plain C++ (no HIP, no common.h): also built host-only by tests/test_upload_plan_host.py, which executes the plans with
// memcpy.  pipeline_ingest.hip issues the copies; the resize kernels (resize_bilinear_kernel in frames.hip, yuv_resize_kernel and
// pix_resize_kernel in yuv_kernels.h) read what they leave.
//
// The compact layout.  The bilinear resize to h rows (tf.image.resize without antialias, reference odt.py:15-16) reads two source rows
// per output row d: p(d) and p(d) + 1, p(d) = min(max(floor(src_y(d)), 0), H - 2).  A host-fed source with more than twice the network's
// rows uploads only those.  With `row` the bytes of a packed row or of a luma row:
//  - packed rows (RGB24, 4:2:2): the staged frame is [2h][row], pair d at row 2d;
//  - formats with a chroma plane (NV12, I420, P010): the pairs 0 .. h-2, [2 (h - 1)][row], then the source frame from luma row p(h - 1)
//    to its end as it is - the last pair, the luma rows below it (none or a few) and the whole chroma plane(s).  That tail is one
//    contiguous piece of the source, so the chroma costs no copy call of its own, and the kernels find source row p(h - 1) + r at staged
//    row 2 (h - 1) + r.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/vbt_hip.h"

namespace vbt {

inline bool pix_fmt_is_yuv(int pix_fmt) { return pix_fmt == VBT_PIX_NV12 || pix_fmt == VBT_PIX_I420; }
// Every YUV format the ingest takes (include/vbt_hip.h, "more source formats"); pix_fmt_is_yuv above stays the 4:2:0 pair that the
// export handles (overlay, scaler, mjpeg) know.
inline bool pix_fmt_is_422(int pix_fmt) { return pix_fmt == VBT_PIX_YUYV422 || pix_fmt == VBT_PIX_UYVY422; }
inline bool pix_fmt_is_source_yuv(int pix_fmt) { return pix_fmt_is_yuv(pix_fmt) || pix_fmt_is_422(pix_fmt) || pix_fmt == VBT_PIX_P010; }
// The one place that knows how a source frame of H x W pixels lies in memory: H rows of `row` bytes (packed pixels, or the luma plane),
// then - chroma_plane - H/2 rows of chroma in as many bytes per row.  ok: the layout is defined - the format is known, H and W are
// positive and as even as the format's chroma needs.  It says nothing about an upper limit: that is pix_fmt_takes below.
struct PixLayout {
  bool ok, chroma_plane;
  size_t row, frame_bytes;
};
inline PixLayout pix_layout(int pix_fmt, int H, int W) {
  PixLayout l{false, false, 0, 0};
  if (H < 1 || W < 1) return l;
  const bool even = !(H & 1) && !(W & 1);
  switch (pix_fmt) {
    case VBT_PIX_RGB24: l.ok = true; l.row = (size_t)W * 3; break;
    case VBT_PIX_NV12:
    case VBT_PIX_I420: l.ok = even; l.chroma_plane = true; l.row = (size_t)W; break;
    case VBT_PIX_YUYV422:
    case VBT_PIX_UYVY422: l.ok = !(W & 1); l.row = (size_t)W * 2; break;
    case VBT_PIX_P010: l.ok = even; l.chroma_plane = true; l.row = (size_t)W * 2; break;
    default: return l;
  }
  l.frame_bytes = l.chroma_plane ? (size_t)H * l.row * 3 / 2 : (size_t)H * l.row;
  return l;
}
// Does the format take frames of this size?  The layout must be defined; the 4:2:2 formats and P010 take no side above 16384.  RGB24,
// NV12 and I420 sources of the pipeline have never had an upper limit and keep none.
inline bool pix_fmt_takes(int pix_fmt, int H, int W) {
  const bool limited = pix_fmt_is_422(pix_fmt) || pix_fmt == VBT_PIX_P010;
  return pix_layout(pix_fmt, H, W).ok && (!limited || (H <= 16384 && W <= 16384));
}

// p(d), d = 0 .. h-1: first source row of the pair output row d reads, in the resize kernels' own float32 arithmetic
inline void row_table(int H, int h, std::vector<int>& tab) {
  tab.resize((size_t)h);
  const float sy = (float)H / (float)h;
  for (int d = 0; d < h; d++) {
    const float iy = ((float)d + 0.5f) * sy - 0.5f;
    const int y0 = std::max((int)floorf(iy), 0);
    tab[d] = std::min(y0, H - 2);
  }
}

// A frame of H rows of `row` bytes (+ chroma_plane: H/2 rows of chroma behind them) in a staging buffer, whole or - compact, tab =
// the row table of (H, h) - in the compact layout: the distance between two frames and where a frame's chroma starts (0: it has no
// plane).  These are the two numbers resize_frames_pix_dev takes.
struct StagedLayout {
  size_t frame_bytes, chroma_off;
};
inline StagedLayout staged_layout(size_t row, bool chroma_plane, int H, int h, bool compact, const std::vector<int>& tab) {
  if (!compact) return {chroma_plane ? (size_t)H * row * 3 / 2 : (size_t)H * row, chroma_plane ? (size_t)H * row : 0};
  if (!chroma_plane) return {(size_t)2 * h * row, 0};
  const size_t head = (size_t)2 * (h - 1) * row, luma_tail = (size_t)(H - tab[(size_t)h - 1]) * row;
  return {head + luma_tail + (size_t)H * row / 2, head + luma_tail};
}

// One host-to-device copy of a plan, offsets in bytes from the staging buffer / from the first host frame.  flat: `width` contiguous
// bytes (height 1, no pitch); else `height` rows of `width` bytes at the two pitches.
struct UploadCopy {
  size_t dst_off, dst_pitch, src_off, src_pitch, width, height;
  bool flat;
};

// The copies that bring nf consecutive host frames to frame slots slot0 .. slot0 + nf - 1 of a staging buffer, in the order they are
// issued; the sum of width * height is nf * staged_layout().frame_bytes.  The fewest calls the layout allows:
//  - whole frames: one flat copy;
//  - compact, pairs at one source pitch (`uniform`): packed rows at an integer scale (step * h == H) continue at that pitch from frame
//    to frame - ONE strided copy of nf * h rows; else one strided copy per frame - with a chroma plane (which breaks the pitch between
//    frames) only while that is fewer copies than one per pair;
//  - compact, otherwise: pair d of every frame in one strided copy (pitch = one source frame / one staged frame);
//  - chroma plane: the tails of all frames in one more strided copy.
inline void upload_plan(size_t row, bool chroma_plane, int H, int h, bool compact, const std::vector<int>& tab, int slot0, int nf,
                        std::vector<UploadCopy>& plan) {
  plan.clear();
  const size_t fb = chroma_plane ? (size_t)H * row * 3 / 2 : (size_t)H * row;   // source frame
  if (!compact) {
    plan.push_back({(size_t)slot0 * fb, 0, 0, 0, (size_t)nf * fb, 1, true});
    return;
  }
  const size_t sb = staged_layout(row, chroma_plane, H, h, true, tab).frame_bytes, dst = (size_t)slot0 * sb;
  const int np = chroma_plane ? h - 1 : h;   // pairs that travel as pairs (the last one of a chroma-plane format is in the tail)
  const int step = h > 1 ? tab[1] - tab[0] : 0;
  bool uniform = np > 1;
  for (int d = 1; d < np && uniform; d++) uniform = tab[d] - tab[d - 1] == step;
  if (uniform && !chroma_plane && (long)step * h == H) {
    plan.push_back({dst, 2 * row, (size_t)tab[0] * row, (size_t)step * row, 2 * row, (size_t)nf * h, false});
  } else if (uniform && (!chroma_plane || nf < np)) {
    for (int b = 0; b < nf; b++)
      plan.push_back({dst + (size_t)b * sb, 2 * row, (size_t)b * fb + (size_t)tab[0] * row, (size_t)step * row, 2 * row, (size_t)np, false});
  } else {
    for (int d = 0; d < np; d++) plan.push_back({dst + (size_t)d * 2 * row, sb, (size_t)tab[d] * row, fb, 2 * row, (size_t)nf, false});
  }
  if (chroma_plane) {
    const size_t tail_src = (size_t)tab[(size_t)h - 1] * row;
    plan.push_back({dst + (size_t)2 * (h - 1) * row, sb, tail_src, fb, fb - tail_src, (size_t)nf, false});
  }
}

}  // namespace vbt
