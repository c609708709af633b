// Halo bookkeeping of the fused tile kernels' expand stage (fused_block.h).  Plain C++: the kernel and the host test share it.
//
// A tile's input halo is HWx x HWy pixels with its origin at image pixel (iy0, ix0); halo pixel p = hy * HWx + hx.  The expand stage walks
// the NPh = HWx * HWy pixels in groups of 16 (lane r of group pg holds pixel 16 pg + r; wave w takes the groups w, w + 4, ...), and must
// know two things about a pixel: whether it exists (the last group is part-filled unless NPh % 16 == 0) and whether it lies outside the
// image (the depthwise pads ITS input, so such a pixel of the expanded tile is forced to the expand's zero point).
#pragma once

// the halo reaches past the image on some side: false <=> no halo pixel of the tile is out of the image, and the expand stage needs
// neither the masks below nor the select they feed (most tiles of the large maps)
constexpr bool halo_border(int iy0, int ix0, int HWx, int HWy, int H, int W) { return iy0 < 0 || ix0 < 0 || iy0 + HWy > H || ix0 + HWx > W; }
// image pixel (iy, ix) is out of an H x W image: two unsigned compares (a negative coordinate wraps past every H, W > 0)
constexpr bool halo_outside(int iy, int ix, int H, int W) { return (unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W; }
constexpr int halo_groups(int NPh) { return (NPh + 15) >> 4; }
// groups wave w of four walks
constexpr int halo_wave_groups(int NPh, int wave) { return (halo_groups(NPh) - wave + 3) >> 2; }
// lanes r < halo_group_lanes hold a pixel of the halo (p < NPh): 16 on every group but the last
constexpr int halo_group_lanes(int NPh, int pg) { return NPh - 16 * pg < 16 ? NPh - 16 * pg : 16; }
// lane r's out-of-image bits of a border tile, bit i <-> group wave + 4 i.  A lane past the halo's end (p >= NPh) takes the bit of the last
// pixel: it loads that pixel's row and stores nothing.  row_of(p) = p / HWx (the kernel divides through a reciprocal).
template <class RowOf>
constexpr unsigned halo_oob_mask(int wave, int r, int NPh, int HWx, int iy0, int ix0, int H, int W, RowOf row_of) {
  unsigned mask = 0;
  for (int i = 0, pg = wave; pg < halo_groups(NPh); pg += 4, i++) {
    const int p = pg * 16 + r, pc = p < NPh - 1 ? p : NPh - 1;
    const int hy = row_of(pc), hx = pc - hy * HWx;
    if (halo_outside(iy0 + hy, ix0 + hx, H, W)) mask |= 1u << i;
  }
  return mask;
}
