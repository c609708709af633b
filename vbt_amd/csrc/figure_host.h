// Host side of a figure handle (figure.hip, curve_figure.hip): the refusals every figure's create, render and table share, the one
// device allocation carved into regions, and the part of the handle the shared calls work on.  `who` is the entry point's name as the
// error texts give it.
#pragma once
#include "carver.h"
#include "common.h"
#include "dev_mem.h"

namespace vbt {

using FigCarver = Carver<64>;   // the regions of a figure's blob begin on 64-byte boundaries
inline size_t align64(size_t v) { return FigCarver::align(v); }

inline int check_canvas(const char* who, int width, int height, int scale, int thickness) {
  if (width < 1 || width > 16384 || height < 1 || height > 16384) { set_error("%s: figures of 1..16384 pixels a side, got %d x %d", who, width, height); return VBT_ERR_ARG; }
  if (scale < 1 || scale > 64) { set_error("%s: scale %d outside 1..64", who, scale); return VBT_ERR_ARG; }
  if (thickness < 1 || thickness > 64) { set_error("%s: thickness %d outside 1..64", who, thickness); return VBT_ERR_ARG; }
  return VBT_OK;
}

// G: the figure's geometry (W, H, s and the plot rectangle's PW x PH)
template <class Geom>
int check_plot_rect(const char* who, const Geom& G, int min_plot) {
  if (G.PW >= min_plot && G.PH >= min_plot) return VBT_OK;
  set_error("%s: a %d x %d figure at scale %d leaves a plot rectangle of %d x %d, below %d x %d", who, G.W, G.H, G.s, G.PW, G.PH, min_plot, min_plot);
  return VBT_ERR_ARG;
}

// What the shared calls need of a handle.  blob is the one allocation, its head the upload of the last set.
struct FigureHandle {
  int device = 0;
  DevBuf<uint8_t> blob;
  int rec_cap = 0;
  int n = 0;                           // figures set
  hipStream_t last = nullptr;          // the stream of the last set or render: table waits for it
  int32_t *d_recs = nullptr, *d_nrec = nullptr;

  // the tail of set: e is what the upload and the prepare launch on st gave; synchronises (the caller frees its upload buffer) and reports
  int finish_set(const char* who, hipStream_t st, hipError_t e) {
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { set_error("%s failed: %s", who, hipGetErrorString(e)); return VBT_ERR_HIP; }
    last = st;
    return VBT_OK;
  }
  ~FigureHandle() {
    if (blob) (void)hipSetDevice(device);   // (the blob goes after this: its free waits for the launches still using it)
  }
};

// the refusals of render; set_name: the entry point that sets figures
inline int check_render_args(const char* who, const char* set_name, const FigureHandle* h, const void* frames, int fig0, int n) {
  if (!h || !frames) { set_error("%s: NULL argument (handle %p, frames %p)", who, (const void*)h, frames); return VBT_ERR_ARG; }
  if (h->n == 0) { set_error("%s: no figures are set (%s)", who, set_name); return VBT_ERR_STATE; }
  if (fig0 < 0 || n < 0 || (long)fig0 + n > h->n) { set_error("%s: figures %d .. %ld outside the %d that are set", who, fig0, (long)fig0 + n - 1, h->n); return VBT_ERR_ARG; }
  return VBT_OK;
}

// table, once its pointers are checked: its refusals, then the wait for the handle's last stream and the figure's record count
inline int table_begin(const char* who, const char* set_name, const FigureHandle* h, int fig, int32_t* nrec) {
  if (h->n == 0) { set_error("%s: no figures are set (%s)", who, set_name); return VBT_ERR_STATE; }
  if (fig < 0 || fig >= h->n) { set_error("%s: figure %d outside the %d that are set", who, fig, h->n); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(h->device));
  VBT_HIP_CHECK(hipStreamSynchronize(h->last));
  VBT_HIP_CHECK(hipMemcpy(nrec, h->d_nrec + fig, 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

}  // namespace vbt
