// Raster tile (device only): what the render kernels of figure.hip and curve_figure.hip share besides raster_core.h - the frame
// rectangle of a workgroup's tile, the staging of the records that touch it, and the RGB24 store of four adjacent pixels.  The tile's
// height and the way points are staged are each kernel's own.
#pragma once
#include "raster_core.h"

namespace vbt {

constexpr int RASTER_THREADS = 256;
constexpr int RASTER_TILE_W = 256;      // a lane decides four adjacent pixels: a wavefront stores 768 contiguous bytes of one pixel row at a time

struct TileBox { int x_lo, y_lo, x_hi, y_hi; };

// tile blockIdx.x of a W x H frame cut into tiles of RASTER_TILE_W x TILE_H, tiles_x to a row of tiles
template <int TILE_H>
__device__ __forceinline__ TileBox tile_box(int tiles_x, int W, int H) {
  const int x_lo = (int)(blockIdx.x % tiles_x) * RASTER_TILE_W, y_lo = (int)(blockIdx.x / tiles_x) * TILE_H;
  return {x_lo, y_lo, (x_lo + RASTER_TILE_W < W ? x_lo + RASTER_TILE_W : W) - 1, (y_lo + TILE_H < H ? y_lo + TILE_H : H) - 1};
}

// The records of gr[nrec][REC] that touch the tile and can be seen, copied to s_recs in any order: the first `cap` of them.  *s_found
// (LDS, zero before the workgroup came here) counts all of them; the caller synchronises, and above cap reads gr.
template <int REC>
__device__ __forceinline__ void stage_tile_records(const int32_t* gr, int nrec, const TileBox& box, int32_t* s_recs, int cap, int* s_found) {
  for (int r = threadIdx.x; r < nrec; r += RASTER_THREADS) {
    const int32_t* q = gr + (size_t)r * REC;
    if (q[REC_X0] > box.x_hi || q[REC_X1] < box.x_lo || q[REC_Y0] > box.y_hi || q[REC_Y1] < box.y_lo) continue;
    if (q[REC_X0] > q[REC_X1] || q[REC_Y0] > q[REC_Y1]) continue;
    const int k = atomicAdd(s_found, 1);
    if (k < cap)
      for (int e = 0; e < REC; e++) s_recs[k * REC + e] = q[e];
  }
}

// pixels e < n_valid of rgb[4] (r | g << 8 | b << 16 each) to the 3 bytes at p + 3 e.  words: n_valid == 4 and p is 4-aligned - three
// 32-bit stores
__device__ __forceinline__ void store_rgb24x4(uint8_t* p, const uint32_t (&rgb)[4], int n_valid, int words) {
  if (words) {
    uint32_t* w = (uint32_t*)p;
    w[0] = rgb[0] | (rgb[1] & 0xffu) << 24;
    w[1] = rgb[1] >> 8 | (rgb[2] & 0xffffu) << 16;
    w[2] = rgb[2] >> 16 | rgb[3] << 8;
  } else {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (e >= n_valid) break;
      p[3 * e] = (uint8_t)rgb[e]; p[3 * e + 1] = (uint8_t)(rgb[e] >> 8); p[3 * e + 2] = (uint8_t)(rgb[e] >> 16);
    }
  }
}

}  // namespace vbt
