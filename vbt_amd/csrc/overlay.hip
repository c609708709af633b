// Tracking overlay on the device (gfx950): box, id label, marker and bar path of the tracked plates drawn into frames that are
// already in device memory (include/vbt_hip.h, "tracking overlay"; reference track.py:28-62,201-224).  Four kernels:
//   overlay_prepare_kernel, once per vbt_overlay_set_rows: one thread per row - frame number, the six pixel coordinates, trail length;
//   overlay_draw_kernel, once per vbt_overlay_draw: grid (row slot x chunk, frame of the batch).  A frame's rows come from the dense
//     index frame number -> rows (the host builds it while it validates the rows; it sizes the grid from it; follow mode: from the
//     links of overlay_follow_kernel, with a grid of as many row slots as a frame can hold).  Chunk 0 of a row is its
//     box outline (a few thousand pixels), chunk 1 its marker and label, chunk 2 + j the 16 trail segments 16 j .. 16 j + 15, one per
//     16-lane group: a segment is a few dozen candidate pixels, so a wavefront takes four of them and a workgroup sixteen.
//   overlay_follow_kernel, once per vbt_overlay_follow_update (follow mode: the rows are a log in device memory that its writer
//     extends): one wavefront takes the new rows 64 at a time - geometry, the previous row of the id, the 16th one before it, the
//     frame's row list, the id table.  The draw kernel then finds a frame's rows and a row's trail through those links.
//   overlay_hud_kernel, once more per vbt_overlay_draw when vbt_overlay_set_hud set a rep panel: grid (tile of the panel, frame of the
//     batch), one thread per 2 x 2 pixel quad - the chroma sample and its four lumas have one owner, and so has every RGB24 byte.
//     The panel is a gather in two colours: every pixel of its rectangle is tested against the contract and written once.
//   overlay_hud_follow_kernel, once per vbt_overlay_hud_follow_update (the panel follows the live rep analysis of a tracker's clip):
//     one wavefront forms the panel's table from the leader's phase list in the live tables - the records vbt_overlay_set_hud
//     forms on the host, by the same statements (overlay_core.h) - and leaves the phase count in device memory for the panel kernel.
// Nothing reads a pixel and nothing passes over a frame: a workgroup walks its primitive clipped to the frame, or its tile of the
// panel (overlay_core.h).
#include <algorithm>

#include "carver.h"
#include "common.h"
#include "dev_mem.h"
#include "hip_handles.h"
#include "overlay_core.h"
#include "tracker_host.h"

namespace vbt {

constexpr int OV_THREADS = 256;
constexpr int OV_SEG_LANES = 16;                                  // lanes per trail segment
constexpr int OV_SEGS_PER_BLOCK = OV_THREADS / OV_SEG_LANES;
constexpr int OV_HUD_TILE_X = 32, OV_HUD_TILE_Y = OV_THREADS / OV_HUD_TILE_X;   // quads of a workgroup: a row of a wavefront's stores is contiguous
constexpr int OV_HUD_MAX_PHASES = 65536;

struct OverlayDrawArgs {
  const int32_t* geom;     // [n][OV_GEOM]
  const int64_t* ids;      // row i's id at ids[8 i] (the rows as uploaded)
  const int32_t* fstart;   // [fmax + 2]: rows of frame f are frow[fstart[f] .. fstart[f + 1])
  const int32_t* frow;     // [n] row numbers ordered by frame
  const int32_t* link;     // follow mode (else NULL): [rows_cap][OV_LINK], and
  const int32_t* findex;   //   [fmax + 1][2] newest row of the frame, its rows
  uint8_t* frames;
  size_t frame_bytes;
  int frame0, frame_step, fmax, chunks;
  int H, W, fmt, t, R, s, label, box;
  uint8_t c0, c1, c2;
};

struct OverlayHudArgs {
  const int32_t* tab;      // [P][OV_HUD_REC]
  const int32_t* P_dev;    // a panel that follows the live analysis (else NULL): P is read here
  uint8_t* frames;
  size_t frame_bytes;
  int P, frame0, frame_step, tiles_x;
  int H, W, fmt, X, Y, s, full_scale_cm;
  int pairs;               // YUV: the frames start at an even address, so two lumas (and NV12's U, V) go out as one 2-byte store
  uint8_t fg[3], bg[3];    // r, g, b or Y, U, V
};

__global__ __launch_bounds__(OV_THREADS) void overlay_prepare_kernel(const OverlayRow* __restrict__ rows, int n, double fps, int H, int W, int trail,
                                                                       int32_t* __restrict__ geom) {
  const int i = blockIdx.x * OV_THREADS + threadIdx.x;
  if (i >= n) return;
  int32_t g[OV_GEOM];
  ov_row_geometry(rows[i], fps, H, W, g);
  // rows are sorted by (id, time): the rows of the same id before row i are a contiguous slice ending at i
  const int64_t id = rows[i].id;
  int lo = 0, hi = trail - 1 < i ? trail - 1 : i;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[i - mid].id == id) lo = mid; else hi = mid - 1;
  }
  g[OV_TRAIL] = lo + 1;
#pragma unroll
  for (int k = 0; k < OV_GEOM; k++) geom[(size_t)i * OV_GEOM + k] = g[k];
}

__global__ __launch_bounds__(OV_THREADS) void overlay_draw_kernel(OverlayDrawArgs A) {
  const long f = (long)A.frame0 + (long)blockIdx.y * A.frame_step;
  if (f < 1 || f > A.fmax) return;
  const int slot = blockIdx.x / A.chunks, chunk = blockIdx.x % A.chunks;
  int row;
  if (A.link) {
    if (slot >= A.findex[2 * (size_t)f + 1]) return;
    row = ov_follow_frame_row(A.findex, A.link, f, slot);
    if (row < 0) return;
  } else {
    const int r0 = A.fstart[f], r1 = A.fstart[f + 1];
    if (slot >= r1 - r0) return;
    row = A.frow[r0 + slot];
  }
  const int32_t* g = A.geom + (size_t)row * OV_GEOM;
  Painter P{A.frames + (size_t)blockIdx.y * A.frame_bytes, A.H, A.W, A.fmt, A.c0, A.c1, A.c2};
  const int lane = threadIdx.x;
  if (chunk == 0) {
    if (A.box) ov_draw_box(P, g, A.t, lane, OV_THREADS);
  } else if (chunk == 1) {
    ov_draw_marker(P, g, A.R, lane, OV_THREADS);
    if (A.label) {                                                // (uniform over the workgroup, like `chunk`)
      __shared__ uint8_t chars[OV_MAX_CHARS];
      __shared__ int nchars;
      if (lane == 0) nchars = ov_label_chars(A.ids[(size_t)row * 8], chars);
      __syncthreads();
      ov_draw_label(P, g, chars, nchars, A.s, lane, OV_THREADS);
    }
  } else {
    // trail point k (0 = oldest) of this row is the centre of row (row - (trail length - 1) + k); segment s joins points s, s + 1
    const int nseg = g[OV_TRAIL] - 1;
    const int seg = (chunk - 2) * OV_SEGS_PER_BLOCK + lane / OV_SEG_LANES;
    if (seg >= nseg) return;
    if (A.link) {                                                 // segments counted from the newest: at most chunks - 3 skip links, then 15 rows back
      int older, newer;
      ov_follow_segment(A.link, row, seg, &older, &newer);
      if (older < 0) return;
      const int32_t *q0 = A.geom + (size_t)older * OV_GEOM, *q1 = A.geom + (size_t)newer * OV_GEOM;
      ov_draw_segment(P, q0[OV_CX], q0[OV_CY], q1[OV_CX], q1[OV_CY], A.t, lane % OV_SEG_LANES, OV_SEG_LANES);
      return;
    }
    const int32_t* p0 = A.geom + (size_t)(row - nseg + seg) * OV_GEOM;
    ov_draw_segment(P, p0[OV_CX], p0[OV_CY], p0[OV_GEOM + OV_CX], p0[OV_GEOM + OV_CY], A.t, lane % OV_SEG_LANES, OV_SEG_LANES);
  }
}

// Follow mode: rows [cursor, min(*nrows_dev, rows_cap)) of the log, 64 at a time, lane j taking row base + j.  The rows of a group
// are taken as if every one that can stand on its own were accepted: its place among the group's rows of its id and of its frame
// comes from a walk over the lanes, what came before the group from the tables.  If under that assumption no row is out of order and
// no frame overfull, the assumption holds (row by row, each sees exactly the state assumed) and the group is stored side by side.
// Otherwise lane 0 takes the group row by row through ov_follow_row - the statement both paths implement.  The fences order one
// lane's stores before another lane's loads of them: within a group (new ids, links) and from one group to the next.
__global__ __launch_bounds__(64) void overlay_follow_kernel(OvFollow F, const int32_t* __restrict__ nrows_dev) {
  const int lane = threadIdx.x;
  const int cur = F.state[OV_STATE_CURSOR];
  int n = *nrows_dev;
  n = n > F.rows_cap ? F.rows_cap : n;
  if (n < cur) {
    if (lane == 0) F.state[OV_STATE_FLAGS] |= VBT_OVERLAY_FOLLOW_REWOUND;
    return;
  }
  int flags = 0;
  for (int base = cur; base < n; base += 64) {
    const int i = base + lane;
    const bool in = i < n;
    OverlayRow r{};
    int32_t g[OV_GEOM];
    if (in) r = F.rows[i];
    const int own = in ? ov_follow_static(r, F.fps, F.H, F.W, F.max_frame, g) : 0;
    const bool ok = in && own == 0;
    const long long id = ok ? (long long)r.id : -1;
    const int f = ok ? g[OV_FRAME] : -1;
    int pj = -1, rank = 0, qj = -1, frank = 0;                    // the lane before this one with its id / its frame, and how many there are
    bool later_id = false, later_f = false;
    for (int j = 0; j < 64; j++) {
      const long long idj = __shfl(id, j);
      const int fj = __shfl(f, j);
      if (ok && idj == id) { if (j < lane) { pj = j; rank++; } else if (j > lane) later_id = true; }
      if (ok && fj == f) { if (j < lane) { qj = j; frank++; } else if (j > lane) later_f = true; }
    }
    int slot = ok ? ov_follow_find(F.table, F.table_mask, r.id, false) : -1;
    unsigned long long need = __ballot(ok && slot < 0 && pj < 0);   // new ids, one lane each: they take their slots one after the other
    while (need) {
      const int j = __ffsll((long long)need) - 1;
      need &= need - 1;
      if (lane == j) slot = ov_follow_find(F.table, F.table_mask, r.id, true);
      __threadfence();
    }
    if (ok && slot < 0) slot = ov_follow_find(F.table, F.table_mask, r.id, false);
    const bool lost = ok && slot < 0;                             // (never: the table is larger than the log)
    const int tprev = ok && !lost ? F.table[slot].last : -1;
    const int prev = pj >= 0 ? base + pj : tprev;
    double ptime = __shfl(r.time, pj >= 0 ? pj : 0);
    if (pj < 0 && tprev >= 0) ptime = F.rows[tprev].time;
    const int cnt0 = ok ? F.findex[2 * (size_t)f + 1] : 0;
    const int head0 = ok ? F.findex[2 * (size_t)f] : -1;
    const bool order = ok && prev >= 0 && r.time < ptime, full = ok && cnt0 + frank >= F.max_rows_per_frame;
    if (__ballot(lost || order || full)) {
      if (lane == 0) {
        const int end = base + 64 < n ? base + 64 : n;
        for (int k = base; k < end; k++) flags |= ov_follow_row(F, k);
      }
      __threadfence();
      continue;
    }
    flags |= own;
    const int depth = ok ? (tprev >= 0 ? F.link[(size_t)tprev * OV_LINK + OV_LINK_DEPTH] : 0) + rank + 1 : 0;
    if (in) {
      g[OV_TRAIL] = depth < F.trail ? depth : F.trail;
      ov_follow_store(F, i, g, ok ? prev : -1, -1, depth, !ok ? -1 : (qj >= 0 ? base + qj : (cnt0 > 0 ? head0 : -1)));
    }
    if (ok && !later_id) F.table[slot].last = i;
    if (ok && !later_f) { F.findex[2 * (size_t)f] = i; F.findex[2 * (size_t)f + 1] = cnt0 + frank + 1; }
    __threadfence();
    if (ok && depth > OV_SKIP_HOPS) F.link[(size_t)i * OV_LINK + OV_LINK_SKIP] = ov_follow_skip(F.link, prev, depth);
    __threadfence();
  }
  int all = 0;
  for (int bit = 1; bit < VBT_OVERLAY_FOLLOW_REWOUND; bit <<= 1)
    if (__ballot(flags & bit)) all |= bit;
  if (lane == 0) {
    F.state[OV_STATE_CURSOR] = n;
    if (all) F.state[OV_STATE_FLAGS] |= all;
  }
}

// What a panel that follows the live analysis owns (vbt_overlay_hud_follow), all in one allocation
struct OvHudFollow {
  int32_t* tab;      // [cap][OV_HUD_REC]
  int32_t* state;    // [OV_HUD_STATE]
  double* view;      // [cap][6]: the leader's phase list as the update sees it (the flush view appends to it)
  double fps;
  int cap, clip;     // cap = the tracker's phase_cap
};

// The panel's table from the live tables: the leader of the clip, its entry, its phase list (live_view: the poll's statements, into the
// handle's own scratch), then one lane per phase in strides of 64 - the record of ov_hud_follow_table, whose running concentric
// count is a prefix sum over the lanes carried from stride to stride.  A flag leaves P = 0: records already stored are never read.
__global__ __launch_bounds__(64) void overlay_hud_follow_kernel(OvHudFollow F, LiveBufs b, LiveCfg c, int flush) {
  __shared__ int s_e, s_n, s_flags;
  const int lane = threadIdx.x, clip = F.clip;
  const LiveClip& L = b.clips[clip];
  const LiveEntry* E = b.ents + (size_t)clip * LIVE_ENTRIES;
  const long long ld = L.leader;
  if (lane == 0) { s_e = -1; s_flags = L.flags; s_n = 0; }
  __syncthreads();
  if (ld >= 0 && E[lane].id == ld) s_e = lane;
  if (lane == 0 && ld >= 0 && E[64].id == ld) s_e = 64;
  __syncthreads();
  const int e = s_e;
  int n = 0;
  if (e >= 0) n = live_view(E[e], b, c, clip, e, flush != 0, F.view, &s_n, &s_flags, lane);
  else if (lane == 0 && ld >= 0) s_flags |= LIVE_ROWS_LOST;   // the leader's rows are not in the log
  __syncthreads();
  int flags = s_flags ? VBT_OVERLAY_HUD_FOLLOW_FLAGGED : 0;
  if (flags) n = 0;                                             // (the poll reports no phases then)
  if (n > F.cap) { flags |= VBT_OVERLAY_HUD_FOLLOW_CAPACITY; n = 0; }
  int carry = 0;
  bool bad = false;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool in = i < n;
    int32_t t[OV_HUD_REC] = {0, 0, 0, 0, 0, 0};
    bool ok = false;
    if (in) {
      const double* r = F.view + (size_t)i * 6;
      ok = ov_hud_phase_check(r, i > 0 ? r - 6 : nullptr) == OV_HUD_PHASE_OK && ov_hud_phase_record(r, F.fps, t) == OV_HUD_PHASE_OK;
    }
    const unsigned long long conc = __ballot(ok && t[OV_HUD_TYPE] == 0);
    t[OV_HUD_COUNT] = carry + __popcll(conc & ((2ull << lane) - 1ull));     // concentric phases among phases 0 .. i
    carry += __popcll(conc);
    if (ok) {
#pragma unroll
      for (int k = 0; k < OV_HUD_REC; k++) F.tab[(size_t)i * OV_HUD_REC + k] = t[k];
    }
    bad = bad || (in && !ok);
  }
  if (__ballot(bad)) { flags |= VBT_OVERLAY_HUD_FOLLOW_BAD_PHASE; n = 0; }
  if (lane == 0) {
    F.state[OV_HUD_STATE_P] = n;
    if (flags) F.state[OV_HUD_STATE_FLAGS] |= flags;
    *(long long*)(F.state + OV_HUD_STATE_LEADER) = ld;
  }
}

// The panel lies wholly inside the frame (vbt_overlay_set_hud refuses any other, and the handle's H and W never change) and, for the
// YUV formats, starts at even coordinates: no store here needs a test against the frame, and a quad is exactly one chroma sample.
__global__ __launch_bounds__(OV_THREADS) void overlay_hud_kernel(OverlayHudArgs A) {
  __shared__ OvHudState st;
  const int64_t f = (int64_t)A.frame0 + (int64_t)blockIdx.y * A.frame_step;
  if (threadIdx.x < OV_HUD_PARTS) ov_hud_state_part(A.tab, A.P_dev ? *A.P_dev : A.P, f, A.frame_step, A.s, A.full_scale_cm, (int)threadIdx.x, st);
  __syncthreads();
  const int qx = (int)(blockIdx.x % A.tiles_x) * OV_HUD_TILE_X + (int)threadIdx.x % OV_HUD_TILE_X;
  const int qy = (int)(blockIdx.x / A.tiles_x) * OV_HUD_TILE_Y + (int)threadIdx.x / OV_HUD_TILE_X;
  if (qx >= OV_HUD_CELLS_X / 2 * A.s || qy >= OV_HUD_CELLS_Y / 2 * A.s) return;
  const int rx = 2 * qx, ry = 2 * qy;
  bool on[2][2];
#pragma unroll
  for (int dy = 0; dy < 2; dy++)
#pragma unroll
    for (int dx = 0; dx < 2; dx++) on[dy][dx] = ov_hud_covers(st, A.tab, rx + dx, ry + dy, A.s, f, A.frame_step);
  uint8_t* frame = A.frames + (size_t)blockIdx.y * A.frame_bytes;
  const int px = A.X + rx, py = A.Y + ry;
  if (A.fmt == VBT_PIX_RGB24) {                                    // (X may be odd and a pixel is 3 bytes: no alignment to store wider by)
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
      uint8_t* p = frame + ((size_t)(py + dy) * A.W + px) * 3;
#pragma unroll
      for (int dx = 0; dx < 2; dx++)
#pragma unroll
        for (int c = 0; c < 3; c++) p[3 * dx + c] = on[dy][dx] ? A.fg[c] : A.bg[c];
    }
    return;
  }
#pragma unroll
  for (int dy = 0; dy < 2; dy++) {
    uint8_t* p = frame + (size_t)(py + dy) * A.W + px;
    const uint8_t y0 = on[dy][0] ? A.fg[0] : A.bg[0], y1 = on[dy][1] ? A.fg[0] : A.bg[0];
    if (A.pairs) *(uint16_t*)p = (uint16_t)(y0 | (y1 << 8));
    else { p[0] = y0; p[1] = y1; }
  }
  const bool any = on[0][0] || on[0][1] || on[1][0] || on[1][1];
  const uint8_t u = any ? A.fg[1] : A.bg[1], v = any ? A.fg[2] : A.bg[2];
  uint8_t* chroma = frame + (size_t)A.H * A.W;
  if (A.fmt == VBT_PIX_NV12) {
    uint8_t* p = chroma + (size_t)(py >> 1) * A.W + (size_t)(px >> 1) * 2;
    if (A.pairs) *(uint16_t*)p = (uint16_t)(u | (v << 8));
    else { p[0] = u; p[1] = v; }
  } else {
    const size_t i = (size_t)(py >> 1) * (A.W >> 1) + (px >> 1);
    chroma[i] = u;
    chroma[(size_t)(A.H >> 1) * (A.W >> 1) + i] = v;
  }
}

}  // namespace vbt

using namespace vbt;

struct vbt_overlay {
  int device = 0, H = 0, W = 0, fmt = 0;
  vbt_overlay_params prm{};
  uint8_t c0 = 0, c1 = 0, c2 = 0;        // the colour in the frames' format
  size_t frame_bytes = 0;
  int chunks = 2;                        // workgroups per row: box, marker + label, ceil((trail - 1) / 16) of trail segments
  int n = 0, fmax = 0;
  DevBuf<uint8_t> blob;                  // rows | frow | fstart | geom in one allocation
  const OverlayRow* d_rows = nullptr;
  const int32_t *d_frow = nullptr, *d_fstart = nullptr;
  int32_t* d_geom = nullptr;
  std::vector<int32_t> fstart;           // the host's copy of the index: sizes the grid of a draw
  bool follow = false;                   // follow mode (vbt_overlay_follow): the rows are F.rows, everything else of F in follow_blob
  OvFollow F{};
  const int32_t* nrows_dev = nullptr;
  DevBuf<uint8_t> follow_blob;           // geom | link | table | findex | state in one allocation
  bool hud = false;                      // a rep panel is set (vbt_overlay_set_hud)
  vbt_overlay_hud_params hud_prm{};
  uint8_t b0 = 0, b1 = 0, b2 = 0;        // the panel's background in the frames' format
  int hud_P = 0;
  DevBuf<int32_t> hud_tab;               // the table of vbt_overlay_set_hud
  const int32_t* d_hud = nullptr;        // [hud_P][OV_HUD_REC], what a draw reads: hud_tab, or (hud_follow) HF.tab inside hud_follow_blob
  bool hud_follow = false;               // the panel follows the live analysis (vbt_overlay_hud_follow): hud is set too
  OvHudFollow HF{};
  vbt_tracker* hud_trk = nullptr;        // the followed tracker (borrowed)
  DevBuf<uint8_t> hud_follow_blob;       // table | state | view in one allocation
  int hud_flush = 0;                     // flush_view of the updates vbt_pipeline_overlay_draw makes
  Event ev_hud_drawn;                    // behind the last draw vbt_pipeline_overlay_draw enqueued: its next update waits for it
  bool hud_drawn = false;
};

namespace {

// the refusals of vbt_overlay_set_rows that need no handle and no device
int check_rows(const OverlayRow* rows, int n, double fps) {
  if (n < 0 || (n > 0 && !rows)) { set_error("vbt_overlay_set_rows: bad argument (n %d, rows %p)", n, (const void*)rows); return VBT_ERR_ARG; }
  if (!(fps > 0) || !std::isfinite(fps)) { set_error("vbt_overlay_set_rows: fps must be positive and finite, got %g", fps); return VBT_ERR_ARG; }
  for (int i = 0; i < n; i++) {
    const OverlayRow& r = rows[i];
    const double v[7] = {r.time, r.x, r.y, r.dx, r.dy, r.h, r.w};
    for (double d : v)
      if (!std::isfinite(d)) { set_error("vbt_overlay_set_rows: row %d holds a non-finite value", i); return VBT_ERR_ARG; }
    if (r.id < 0) { set_error("vbt_overlay_set_rows: row %d has a negative id %lld", i, (long long)r.id); return VBT_ERR_ARG; }
    if (r.w < 0 || r.h < 0) { set_error("vbt_overlay_set_rows: row %d has a negative plate width or height", i); return VBT_ERR_ARG; }
    if (i > 0 && (rows[i - 1].id > r.id || (rows[i - 1].id == r.id && rows[i - 1].time > r.time))) {
      set_error("vbt_overlay_set_rows: rows are not sorted by (id, time) at row %d", i);
      return VBT_ERR_ARG;
    }
  }
  return VBT_OK;
}

// the colour of the frames' format: r, g, b or the contract's Y, U, V
void overlay_colour(int fmt, const uint8_t* rgb, uint8_t* c) {
  const int r = rgb[0], g = rgb[1], b = rgb[2];
  if (fmt == VBT_PIX_RGB24) { c[0] = rgb[0]; c[1] = rgb[1]; c[2] = rgb[2]; return; }
  c[0] = (uint8_t)(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16);
  c[1] = (uint8_t)(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128);
  c[2] = (uint8_t)(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128);
}

// the refusals on a panel's parameters alone (`who`: vbt_overlay_set_hud or vbt_overlay_hud_follow)
int check_hud_panel(const char* who, const vbt_overlay_hud_params* prm) {
  if (prm->scale < 1 || prm->scale > 64) { set_error("%s: scale %d outside 1..64", who, prm->scale); return VBT_ERR_ARG; }
  if (prm->full_scale_cm < 1 || prm->full_scale_cm > 100000) { set_error("%s: full_scale_cm %d outside 1..100000", who, prm->full_scale_cm); return VBT_ERR_ARG; }
  if (prm->x < 0 || prm->y < 0) { set_error("%s: negative panel origin (%d, %d)", who, prm->x, prm->y); return VBT_ERR_ARG; }
  return VBT_OK;
}

// ... and on the panel's place in the handle's frames
int check_hud_geometry(const char* who, const vbt_overlay* o, const vbt_overlay_hud_params* params) {
  const bool yuv = o->fmt != VBT_PIX_RGB24;
  if (yuv && ((params->x | params->y) & 1)) {
    set_error("%s: a YUV 4:2:0 panel starts at even coordinates, got (%d, %d)", who, params->x, params->y);
    return VBT_ERR_ARG;
  }
  if ((long)params->x + OV_HUD_CELLS_X * params->scale > o->W || (long)params->y + OV_HUD_CELLS_Y * params->scale > o->H) {
    set_error("%s: the %d x %d panel at (%d, %d) does not lie inside the %d x %d frame", who, OV_HUD_CELLS_X * params->scale,
              OV_HUD_CELLS_Y * params->scale, params->x, params->y, o->W, o->H);
    return VBT_ERR_ARG;
  }
  return VBT_OK;
}

// the refusals of vbt_overlay_set_hud that need no handle and no device; on VBT_OK `tab` is the table to upload.  The tests on a
// phase and its record are overlay_core.h's, shared with overlay_hud_follow_kernel.
int check_hud(const vbt_overlay_hud_params* prm, const double* ph, int P, double fps, std::vector<int32_t>& tab) {
  if (P < 0 || (P > 0 && (!ph || !prm))) {
    set_error("vbt_overlay_set_hud: bad argument (P %d, phases %p, params %p)", P, (const void*)ph, (const void*)prm);
    return VBT_ERR_ARG;
  }
  if (!(fps > 0) || !std::isfinite(fps)) { set_error("vbt_overlay_set_hud: fps must be positive and finite, got %g", fps); return VBT_ERR_ARG; }
  for (int i = 0; i < P; i++) {
    const double* r = ph + (size_t)i * 6;
    switch (ov_hud_phase_check(r, i > 0 ? r - 6 : nullptr)) {
      case OV_HUD_PHASE_NONFINITE: set_error("vbt_overlay_set_hud: phase %d holds a non-finite value", i); return VBT_ERR_ARG;
      case OV_HUD_PHASE_TYPE: set_error("vbt_overlay_set_hud: phase %d has type %g, not 0, 1 or 2", i, r[5]); return VBT_ERR_ARG;
      case OV_HUD_PHASE_ENDS_BEFORE: set_error("vbt_overlay_set_hud: phase %d ends before it starts (time_end < time_start)", i); return VBT_ERR_ARG;
      case OV_HUD_PHASE_ORDER: set_error("vbt_overlay_set_hud: phases are not ordered in time at phase %d", i); return VBT_ERR_ARG;
      default: break;
    }
  }
  if (int rc = check_hud_panel("vbt_overlay_set_hud", prm)) return rc;
  if (P > OV_HUD_MAX_PHASES) { set_error("vbt_overlay_set_hud: %d phases, above %d", P, OV_HUD_MAX_PHASES); return VBT_ERR_CAPACITY; }
  tab.assign((size_t)P * OV_HUD_REC, 0);
  int count = 0;
  for (int i = 0; i < P; i++) {
    const double* r = ph + (size_t)i * 6;
    int32_t* t = tab.data() + (size_t)i * OV_HUD_REC;
    if (ov_hud_phase_record(r, fps, t)) { set_error("vbt_overlay_set_hud: phase %d ends at frame %d, above %d", i, t[OV_HUD_FE], (int)OV_MAX_FRAME); return VBT_ERR_CAPACITY; }
    count += t[OV_HUD_TYPE] == 0;
    t[OV_HUD_COUNT] = count;
  }
  return VBT_OK;
}

// the launches of the row primitives (rules 1-4) for a handle with rows
void overlay_launch_rows(vbt_overlay* o, uint8_t* frames_dev, int B, int frame0, int frame_step, int MAX_Y, hipStream_t stream) {
  OverlayDrawArgs A{};
  A.geom = o->d_geom; A.ids = (const int64_t*)o->d_rows; A.fstart = o->d_fstart; A.frow = o->d_frow;
  if (o->follow) { A.geom = o->F.geom; A.ids = (const int64_t*)o->F.rows; A.link = o->F.link; A.findex = o->F.findex; }
  A.frame_bytes = o->frame_bytes; A.frame_step = frame_step; A.fmax = o->fmax; A.chunks = o->chunks;
  A.H = o->H; A.W = o->W; A.fmt = o->fmt; A.t = o->prm.thickness; A.R = o->prm.radius; A.s = o->prm.label_scale;
  A.label = o->prm.label; A.box = o->prm.box; A.c0 = o->c0; A.c1 = o->c1; A.c2 = o->c2;
  for (int b0 = 0; b0 < B; b0 += MAX_Y) {
    const int nb = std::min(MAX_Y, B - b0);
    int most = o->follow ? o->F.max_rows_per_frame : 0;           // rows of the fullest frame of this launch (follow mode: as many as a frame can hold)
    for (int i = 0; i < nb && !o->follow; i++) {
      const long f = (long)frame0 + (long)(b0 + i) * frame_step;
      if (f > o->fmax) break;
      most = std::max(most, o->fstart[f + 1] - o->fstart[f]);
    }
    if (most == 0) continue;
    A.frames = frames_dev + (size_t)b0 * o->frame_bytes;
    A.frame0 = (int)((long)frame0 + (long)b0 * frame_step);
    overlay_draw_kernel<<<dim3((unsigned)most * (unsigned)o->chunks, (unsigned)nb), OV_THREADS, 0, stream>>>(A);
  }
}

void overlay_free_hud(vbt_overlay* o) {
  o->hud_tab.reset(); o->hud_follow_blob.reset();   // (each waits for the updates and draws still using it)
  o->ev_hud_drawn.reset(); o->hud_drawn = false;
  o->hud_follow = false; o->HF = OvHudFollow{}; o->hud_trk = nullptr; o->hud_flush = 0;
  o->d_hud = nullptr; o->hud_P = 0; o->hud = false;
}

void overlay_free_rows(vbt_overlay* o) {
  o->blob.reset();   // (waits for the draws still reading it)
  o->d_rows = nullptr; o->d_frow = o->d_fstart = nullptr; o->d_geom = nullptr;
  o->n = 0; o->fmax = 0; o->fstart.clear();
  o->follow_blob.reset();
  o->follow = false; o->F = OvFollow{}; o->nrows_dev = nullptr;
}

}  // namespace

extern "C" {

void vbt_overlay_default_params(vbt_overlay_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->trail = 120; p->thickness = 2; p->radius = 10; p->label_scale = 3;
  p->rgb[0] = p->rgb[1] = p->rgb[2] = 255;
  p->label = 1; p->box = 1;
}

int vbt_overlay_create(int device, int H, int W, int pix_fmt, const vbt_overlay_params* params, vbt_overlay** out) {
  if (!out) { set_error("vbt_overlay_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  vbt_overlay_params p;
  vbt_overlay_default_params(&p);
  if (params) p = *params;
  if (pix_fmt != VBT_PIX_RGB24 && !pix_fmt_is_yuv(pix_fmt)) { set_error("vbt_overlay_create: unknown pixel format %d", pix_fmt); return VBT_ERR_ARG; }
  if (H < 1 || W < 1 || H > 16384 || W > 16384) { set_error("vbt_overlay_create: frames of 1..16384 pixels a side, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (pix_fmt_is_yuv(pix_fmt) && ((H & 1) || (W & 1))) { set_error("vbt_overlay_create: YUV 4:2:0 frames have even H and W, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (p.trail < 1 || p.trail > 65536) { set_error("vbt_overlay_create: trail %d outside 1..65536", p.trail); return VBT_ERR_ARG; }
  if (p.thickness < 0 || p.thickness > 1024) { set_error("vbt_overlay_create: thickness %d outside 0..1024", p.thickness); return VBT_ERR_ARG; }
  if (p.radius < 0 || p.radius > 16384) { set_error("vbt_overlay_create: radius %d outside 0..16384", p.radius); return VBT_ERR_ARG; }
  if (p.label_scale < 1 || p.label_scale > 64) { set_error("vbt_overlay_create: label_scale %d outside 1..64", p.label_scale); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_overlay_create", device, /*set_current=*/false)) return rc;
  vbt_overlay* o = new vbt_overlay();
  o->device = device; o->H = H; o->W = W; o->fmt = pix_fmt; o->prm = p;
  uint8_t c[3];
  overlay_colour(pix_fmt, p.rgb, c);
  o->c0 = c[0]; o->c1 = c[1]; o->c2 = c[2];
  o->frame_bytes = pix_fmt == VBT_PIX_RGB24 ? (size_t)H * W * 3 : (size_t)H * W * 3 / 2;
  o->chunks = 2 + (p.trail - 1 + OV_SEGS_PER_BLOCK - 1) / OV_SEGS_PER_BLOCK;
  *out = o;
  return VBT_OK;
}

void vbt_overlay_destroy(vbt_overlay* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  delete o;
}

int vbt_overlay_set_rows(vbt_overlay* o, const void* rows_host, int n, double fps, void* stream) {
  const OverlayRow* rows = (const OverlayRow*)rows_host;
  if (int rc = check_rows(rows, n, fps)) return rc;
  if (!o) { set_error("vbt_overlay_set_rows: handle is NULL"); return VBT_ERR_ARG; }
  // frame numbers, by the statement the prepare kernel runs: the dense index frame -> rows, a counting sort
  std::vector<int32_t> frame((size_t)n);
  int fmax = 0;
  for (int i = 0; i < n; i++) {
    frame[i] = ov_frame_number(rows[i].time, fps);
    if (frame[i] > OV_MAX_FRAME) { set_error("vbt_overlay_set_rows: row %d is frame %d, above %d", i, frame[i], OV_MAX_FRAME); return VBT_ERR_CAPACITY; }
    fmax = std::max(fmax, frame[i]);
  }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  overlay_free_rows(o);
  if (n == 0) return VBT_OK;
  std::vector<int32_t> fstart((size_t)fmax + 2, 0), frow((size_t)n, 0);
  for (int i = 0; i < n; i++)
    if (frame[i] >= 1) fstart[(size_t)frame[i] + 1]++;           // rows of frames < 1 are never drawn; they still feed trails
  for (int f = 1; f <= fmax + 1; f++) fstart[f] += fstart[f - 1];
  {
    std::vector<int32_t> next(fstart.begin(), fstart.end() - 1);
    for (int i = 0; i < n; i++)
      if (frame[i] >= 1) frow[next[frame[i]]++] = i;
  }
  const size_t rows_b = (size_t)n * sizeof(OverlayRow), frow_b = (size_t)n * 4, fstart_b = fstart.size() * 4;
  const size_t up_b = (rows_b + frow_b + fstart_b + 31) & ~(size_t)31, geom_b = (size_t)n * OV_GEOM * 4;
  std::vector<uint8_t> up(up_b, 0);
  memcpy(up.data(), rows, rows_b);
  memcpy(up.data() + rows_b, frow.data(), frow_b);
  memcpy(up.data() + rows_b + frow_b, fstart.data(), fstart_b);
  VBT_HIP_CHECK(o->blob.alloc(up_b + geom_b));
  uint8_t* const blob = o->blob.get();
  o->d_rows = (const OverlayRow*)blob;
  o->d_frow = (const int32_t*)(blob + rows_b);
  o->d_fstart = (const int32_t*)(blob + rows_b + frow_b);
  o->d_geom = (int32_t*)(blob + up_b);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(blob, up.data(), up_b, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    overlay_prepare_kernel<<<dim3((unsigned)((n + OV_THREADS - 1) / OV_THREADS)), OV_THREADS, 0, st>>>(o->d_rows, n, fps, o->H, o->W, o->prm.trail, o->d_geom);
    e = hipGetLastError();
  }
  const hipError_t es = hipStreamSynchronize(st);                 // (`up` leaves scope: the copy must have read it)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    overlay_free_rows(o);
    set_error("vbt_overlay_set_rows failed: %s", hipGetErrorString(e));
    return VBT_ERR_HIP;
  }
  o->n = n; o->fmax = fmax; o->fstart = std::move(fstart);
  return VBT_OK;
}

int vbt_overlay_draw(vbt_overlay* o, uint8_t* frames_dev, int B, int frame0, int frame_step, void* stream) {
  if (!o || !frames_dev || B < 0 || frame0 < 1 || frame_step < 1 || (long)frame0 + (long)(B - 1) * frame_step > INT32_MAX) {
    set_error("vbt_overlay_draw: bad argument (B >= 0, frame0 >= 1, frame_step >= 1, frame numbers inside int32)");
    return VBT_ERR_ARG;
  }
  if (B == 0 || (o->n == 0 && !o->follow && !o->hud)) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(o->device));
  constexpr int MAX_Y = 32768;                                    // frames per launch (grid.y)
  if (o->n > 0 || o->follow) overlay_launch_rows(o, frames_dev, B, frame0, frame_step, MAX_Y, (hipStream_t)stream);
  if (o->hud) {                                                   // after the rows, on the same stream: the panel wins
    const vbt_overlay_hud_params& hp = o->hud_prm;
    OverlayHudArgs G{};
    G.tab = o->d_hud; G.P_dev = o->hud_follow ? o->HF.state + OV_HUD_STATE_P : nullptr; G.frame_bytes = o->frame_bytes; G.P = o->hud_P; G.frame_step = frame_step;
    G.H = o->H; G.W = o->W; G.fmt = o->fmt; G.X = hp.x; G.Y = hp.y; G.s = hp.scale; G.full_scale_cm = hp.full_scale_cm;
    G.fg[0] = o->c0; G.fg[1] = o->c1; G.fg[2] = o->c2; G.bg[0] = o->b0; G.bg[1] = o->b1; G.bg[2] = o->b2;
    G.pairs = o->fmt != VBT_PIX_RGB24 && ((uintptr_t)frames_dev & 1) == 0;        // (a YUV frame has an even number of bytes)
    G.tiles_x = (OV_HUD_CELLS_X / 2 * hp.scale + OV_HUD_TILE_X - 1) / OV_HUD_TILE_X;
    const int tiles_y = (OV_HUD_CELLS_Y / 2 * hp.scale + OV_HUD_TILE_Y - 1) / OV_HUD_TILE_Y;
    for (int b0 = 0; b0 < B; b0 += MAX_Y) {
      G.frames = frames_dev + (size_t)b0 * o->frame_bytes;
      G.frame0 = (int)((long)frame0 + (long)b0 * frame_step);
      overlay_hud_kernel<<<dim3((unsigned)(G.tiles_x * tiles_y), (unsigned)std::min(MAX_Y, B - b0)), OV_THREADS, 0, (hipStream_t)stream>>>(G);
    }
  }
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

int vbt_overlay_follow(vbt_overlay* o, const void* rows_dev, const int32_t* nrows_dev, int rows_cap, int max_frame, int max_rows_per_frame,
                       double fps) {
  if (!rows_dev || !nrows_dev) { set_error("vbt_overlay_follow: NULL argument (rows %p, row count %p)", rows_dev, (const void*)nrows_dev); return VBT_ERR_ARG; }
  if (rows_cap < 1) { set_error("vbt_overlay_follow: rows_cap %d < 1", rows_cap); return VBT_ERR_ARG; }
  if (max_frame < 1 || max_frame > OV_MAX_FRAME) { set_error("vbt_overlay_follow: max_frame %d outside 1..%d", max_frame, OV_MAX_FRAME); return VBT_ERR_ARG; }
  if (max_rows_per_frame < 1 || max_rows_per_frame > 64) { set_error("vbt_overlay_follow: max_rows_per_frame %d outside 1..64", max_rows_per_frame); return VBT_ERR_ARG; }
  if (!(fps > 0) || !std::isfinite(fps)) { set_error("vbt_overlay_follow: fps must be positive and finite, got %g", fps); return VBT_ERR_ARG; }
  if (!o) { set_error("vbt_overlay_follow: handle is NULL"); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  overlay_free_rows(o);
  size_t slots = 64;
  while (slots < 2 * (size_t)rows_cap) slots <<= 1;
  Carver<8> C;   // geom | link | table | findex | state: every region's size is a multiple of 8, they lie back to back
  const auto geom = C.add<int32_t>((size_t)rows_cap * OV_GEOM), link = C.add<int32_t>((size_t)rows_cap * OV_LINK);
  const auto table = C.add<OvIdSlot>(slots);
  const auto findex = C.add<int32_t>(((size_t)max_frame + 1) * 2), state = C.add<int32_t>(OV_STATE);
  DevBuf<uint8_t> owner;
  VBT_HIP_CHECK(owner.alloc(C.bytes()));
  uint8_t* const blob = owner.get();
  hipError_t e = hipMemsetAsync(blob, 0xff, findex.at, nullptr);   // every slot free (id -1), every link "none"
  if (e == hipSuccess) e = hipMemsetAsync(blob + findex.at, 0, C.bytes() - findex.at, nullptr);
  const hipError_t es = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    set_error("vbt_overlay_follow failed: %s", hipGetErrorString(e));
    return VBT_ERR_HIP;
  }
  OvFollow& F = o->F;
  F.rows = (const OverlayRow*)rows_dev;
  F.geom = C.ptr(blob, geom); F.link = C.ptr(blob, link); F.table = C.ptr(blob, table);
  F.findex = C.ptr(blob, findex); F.state = C.ptr(blob, state);
  F.fps = fps; F.rows_cap = rows_cap; F.max_frame = max_frame; F.max_rows_per_frame = max_rows_per_frame; F.table_mask = (int)(slots - 1);
  F.H = o->H; F.W = o->W; F.trail = o->prm.trail;
  o->follow_blob = std::move(owner); o->nrows_dev = nrows_dev; o->follow = true; o->fmax = max_frame;
  return VBT_OK;
}

int vbt_overlay_follow_update(vbt_overlay* o, void* stream) {
  if (!o) { set_error("vbt_overlay_follow_update: handle is NULL"); return VBT_ERR_ARG; }
  if (!o->follow) { set_error("vbt_overlay_follow_update: the handle follows no row log (vbt_overlay_follow)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  overlay_follow_kernel<<<1, 64, 0, (hipStream_t)stream>>>(o->F, o->nrows_dev);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

int vbt_overlay_follow_status(vbt_overlay* o, int32_t* rows_consumed, int32_t* flags, void* stream) {
  if (!o || !rows_consumed || !flags) { set_error("vbt_overlay_follow_status: NULL argument"); return VBT_ERR_ARG; }
  if (!o->follow) { set_error("vbt_overlay_follow_status: the handle follows no row log (vbt_overlay_follow)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  int32_t st[OV_STATE];
  VBT_HIP_CHECK(hipMemcpyAsync(st, o->F.state, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *rows_consumed = st[OV_STATE_CURSOR];
  *flags = st[OV_STATE_FLAGS];
  return VBT_OK;
}

void vbt_overlay_hud_default_params(vbt_overlay_hud_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->x = 16; p->y = 16; p->scale = 3; p->full_scale_cm = 200;
}

int vbt_overlay_set_hud(vbt_overlay* o, const vbt_overlay_hud_params* params, const double* phases6_host, int P, double fps, void* stream) {
  if (!params && P == 0) {                                          // the panel off
    if (!o) { set_error("vbt_overlay_set_hud: handle is NULL"); return VBT_ERR_ARG; }
    VBT_HIP_CHECK(hipSetDevice(o->device));
    overlay_free_hud(o);
    return VBT_OK;
  }
  std::vector<int32_t> tab;
  if (int rc = check_hud(params, phases6_host, P, fps, tab)) return rc;
  if (!o) { set_error("vbt_overlay_set_hud: handle is NULL"); return VBT_ERR_ARG; }
  if (int rc = check_hud_geometry("vbt_overlay_set_hud", o, params)) return rc;
  VBT_HIP_CHECK(hipSetDevice(o->device));
  DevBuf<int32_t> d;
  if (P > 0) {
    VBT_HIP_CHECK(d.alloc(tab.size()));
    hipError_t e = hipMemcpyAsync(d.get(), tab.data(), tab.size() * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    const hipError_t es = hipStreamSynchronize((hipStream_t)stream);    // (`tab` leaves scope: the copy must have read it)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
      set_error("vbt_overlay_set_hud failed: %s", hipGetErrorString(e));
      return VBT_ERR_HIP;
    }
  }
  overlay_free_hud(o);
  o->hud_tab = std::move(d);
  o->d_hud = o->hud_tab.get(); o->hud_P = P; o->hud = true; o->hud_prm = *params;
  uint8_t c[3];
  overlay_colour(o->fmt, params->bg, c);
  o->b0 = c[0]; o->b1 = c[1]; o->b2 = c[2];
  return VBT_OK;
}

int vbt_overlay_hud_table(vbt_overlay* o, int32_t* out, int cap, int* P) {
  if (!o || !P || cap < 0 || (cap > 0 && !out)) { set_error("vbt_overlay_hud_table: bad argument"); return VBT_ERR_ARG; }
  int n = o->hud_P;
  if (o->hud_follow) {                                              // the count of the last update
    VBT_HIP_CHECK(hipSetDevice(o->device));
    int32_t st[OV_HUD_STATE];
    VBT_HIP_CHECK(hipMemcpy(st, o->HF.state, sizeof(st), hipMemcpyDeviceToHost));
    n = st[OV_HUD_STATE_P];
  }
  *P = n;
  if (cap < n) { set_error("vbt_overlay_hud_table: %d phases, room for %d", n, cap); return VBT_ERR_CAPACITY; }
  if (n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(o->device));
  VBT_HIP_CHECK(hipMemcpy(out, o->d_hud, (size_t)n * OV_HUD_REC * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt_overlay_hud_follow(vbt_overlay* o, const vbt_overlay_hud_params* params, vbt_tracker* t, int clip, double fps) {
  const char* who = "vbt_overlay_hud_follow";
  if (!params) { set_error("%s: params is NULL", who); return VBT_ERR_ARG; }
  if (!(fps > 0) || !std::isfinite(fps)) { set_error("%s: fps must be positive and finite, got %g", who, fps); return VBT_ERR_ARG; }
  if (int rc = check_hud_panel(who, params)) return rc;
  if (!o) { set_error("%s: handle is NULL", who); return VBT_ERR_ARG; }
  if (!t) { set_error("%s: tracker is NULL", who); return VBT_ERR_ARG; }
  const LiveTables lt = live_tables(t);
  if (clip < 0 || clip >= lt.n_clips) { set_error("%s: clip %d outside the tracker's %d clips", who, clip, lt.n_clips); return VBT_ERR_ARG; }
  if (int rc = check_hud_geometry(who, o, params)) return rc;
  if (!lt.on) { set_error("%s: live analysis is not enabled on the tracker (vbt_tracker_live_enable)", who); return VBT_ERR_STATE; }
  if (lt.device != o->device) { set_error("%s: the tracker is on device %d, the handle on device %d", who, lt.device, o->device); return VBT_ERR_ARG; }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  const int cap = lt.c.phase_cap;
  Carver<8> C;   // table | state | view, back to back: the table's and the state's sizes are multiples of 8
  const auto tab = C.add<int32_t>((size_t)cap * OV_HUD_REC), state = C.add<int32_t>(OV_HUD_STATE);
  const auto view = C.add<double>((size_t)cap * 6);
  DevBuf<uint8_t> owner;
  Event ev;
  VBT_HIP_CHECK(owner.alloc(C.bytes()));
  uint8_t* const blob = owner.get();
  hipError_t e = hipMemsetAsync(blob, 0, C.bytes(), nullptr);
  if (e == hipSuccess) e = hipMemsetAsync(C.ptr(blob, state) + OV_HUD_STATE_LEADER, 0xff, 8, nullptr);   // leader -1, P = 0: blank until the first update
  const hipError_t es = hipStreamSynchronize(nullptr);
  if (e == hipSuccess) e = es;
  if (e == hipSuccess) e = ev.create(hipEventDisableTiming);
  if (e != hipSuccess) {
    set_error("%s failed: %s", who, hipGetErrorString(e));
    return VBT_ERR_HIP;
  }
  overlay_free_hud(o);
  o->HF.tab = C.ptr(blob, tab); o->HF.state = C.ptr(blob, state); o->HF.view = C.ptr(blob, view);
  o->HF.fps = fps; o->HF.cap = cap; o->HF.clip = clip;
  o->hud_follow_blob = std::move(owner); o->ev_hud_drawn = std::move(ev); o->hud_drawn = false; o->hud_trk = t; o->hud_flush = 0;
  o->d_hud = o->HF.tab; o->hud_P = 0; o->hud = true; o->hud_follow = true; o->hud_prm = *params;
  uint8_t c[3];
  overlay_colour(o->fmt, params->bg, c);
  o->b0 = c[0]; o->b1 = c[1]; o->b2 = c[2];
  return VBT_OK;
}

int vbt_overlay_hud_follow_update(vbt_overlay* o, int flush_view, void* stream) {
  if (!o) { set_error("vbt_overlay_hud_follow_update: handle is NULL"); return VBT_ERR_ARG; }
  if (!o->hud_follow) { set_error("vbt_overlay_hud_follow_update: the handle's panel follows no live analysis (vbt_overlay_hud_follow)"); return VBT_ERR_STATE; }
  const LiveTables lt = live_tables(o->hud_trk);
  if (!lt.on || lt.c.phase_cap != o->HF.cap) {                     // (live analysis switched off or enabled anew since the panel was bound)
    set_error("vbt_overlay_hud_follow_update: the tracker's live analysis is not the one the panel was bound to");
    return VBT_ERR_STATE;
  }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  overlay_hud_follow_kernel<<<1, 64, 0, (hipStream_t)stream>>>(o->HF, lt.b, lt.c, flush_view != 0);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

int vbt_overlay_hud_follow_status(vbt_overlay* o, int64_t* leader, int32_t* n_phases, int32_t* flags, void* stream) {
  if (!o || !leader || !n_phases || !flags) { set_error("vbt_overlay_hud_follow_status: NULL argument"); return VBT_ERR_ARG; }
  if (!o->hud_follow) { set_error("vbt_overlay_hud_follow_status: the handle's panel follows no live analysis (vbt_overlay_hud_follow)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(o->device));
  int32_t st[OV_HUD_STATE];
  VBT_HIP_CHECK(hipMemcpyAsync(st, o->HF.state, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *n_phases = st[OV_HUD_STATE_P];
  *flags = st[OV_HUD_STATE_FLAGS];
  memcpy(leader, st + OV_HUD_STATE_LEADER, 8);
  return VBT_OK;
}

int vbt_overlay_hud_follow_flush(vbt_overlay* o, int flush_view) {
  if (!o) { set_error("vbt_overlay_hud_follow_flush: handle is NULL"); return VBT_ERR_ARG; }
  if (!o->hud_follow) { set_error("vbt_overlay_hud_follow_flush: the handle's panel follows no live analysis (vbt_overlay_hud_follow)"); return VBT_ERR_STATE; }
  o->hud_flush = flush_view != 0;
  return VBT_OK;
}

int vbt_overlay_geometry(vbt_overlay* o, int32_t* out, int cap, int* n) {
  if (!o || !n || cap < 0 || (cap > 0 && !out)) { set_error("vbt_overlay_geometry: bad argument"); return VBT_ERR_ARG; }
  if (o->follow) {
    VBT_HIP_CHECK(hipSetDevice(o->device));
    int32_t st[OV_STATE];
    VBT_HIP_CHECK(hipMemcpy(st, o->F.state, sizeof(st), hipMemcpyDeviceToHost));
    *n = st[OV_STATE_CURSOR];
    if (cap < *n) { set_error("vbt_overlay_geometry: %d rows, room for %d", *n, cap); return VBT_ERR_CAPACITY; }
    if (*n > 0) VBT_HIP_CHECK(hipMemcpy(out, o->F.geom, (size_t)*n * OV_GEOM * 4, hipMemcpyDeviceToHost));
    return VBT_OK;
  }
  *n = o->n;
  if (cap < o->n) { set_error("vbt_overlay_geometry: %d rows, room for %d", o->n, cap); return VBT_ERR_CAPACITY; }
  if (o->n == 0) return VBT_OK;
  VBT_HIP_CHECK(hipSetDevice(o->device));
  VBT_HIP_CHECK(hipMemcpy(out, o->d_geom, (size_t)o->n * OV_GEOM * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

}  // extern "C"

namespace vbt {

bool overlay_hud_follows(const vbt_overlay* o, const vbt_tracker* t) { return o && o->hud_follow && o->hud_trk == t; }

int overlay_hud_follow_enqueue(vbt_overlay* o, hipStream_t T) {
  if (o->hud_drawn) VBT_HIP_CHECK(hipStreamWaitEvent(T, o->ev_hud_drawn.get(), 0));
  return vbt_overlay_hud_follow_update(o, o->hud_flush, (void*)T);
}

int overlay_hud_follow_drawn(vbt_overlay* o, hipStream_t stream) {
  VBT_HIP_CHECK(hipEventRecord(o->ev_hud_drawn.get(), stream));
  o->hud_drawn = true;
  return VBT_OK;
}

}  // namespace vbt
