// MJPEG import on the device (gfx950): baseline JPEG frames, compressed bytes in host memory -> RGB24 frames in device memory
// (include/vbt_hip.h, "MJPEG import": the bitstream scope and the reconstruction contract; the numpy statement of it is
// tests/mjpeg_dec_ref.py).  The host parses every header (jpeg_parse.h) and packs the descriptors and the entropy-coded segments
// into one pinned buffer: one H2D copy per batch, then four launches, all on the caller's stream:
//   mjpegd_markers_kernel  grid (frame), one workgroup walking the frame's scan 4096 bytes at a time: RSTm count per thread, prefix
//     sum, positions into the frame's ordered interval table; count and m = index mod 8 checked against the descriptor.
//   mjpegd_entropy_kernel  grid (groups of 64 intervals, frame), one lane per restart interval (jpeg_core.h: jpeg_decode_interval);
//     the non-zero levels go, int16 in natural order, into the levels scratch (128 B per block) that a memset cleared.
//   mjpegd_entropy_sync_kernel  in its place (vbt_mjpeg_decoder_set_entropy; AUTO: when a frame's intervals are long): grid (interval,
//     frame), one workgroup per restart interval, 256 lanes on subsequences of the interval that synchronise (jpeg_core.h:
//     jpeg_sync_walk); the same levels and status.
//   mjpegd_idct_kernel     grid (groups of 256 blocks, frame), one thread per block: dequantise + islow IDCT into the component's
//     plane at its own resolution.
//   mjpegd_colour_kernel   grid (groups of 1024 pixels, frame), one thread per 4 pixels: fancy upsampling + YCbCr -> RGB24.
// The decoding statements are those of jpeg_core.h, which the CPU fuzz run walks under ASan / UBSan.
// JPEG stills (include/vbt_hip.h, "JPEG stills": vbt_jpeg_stills) run the same kernels on a batch whose frames differ in size: where a
// frame's blocks, restart positions and output lie is read from a per-frame table (MjdFrame) behind the descriptors; the video
// handle's instantiation of a kernel computes it from the one frame size instead (template <bool TABLE>: one text, two
// instantiations; the sync kernel alone is one plain kernel with a wave-uniform branch between the two).  The grids cover the batch's largest frame and the
// others leave early.  Straight to the network input, the last
// launch is
//   mjpegd_resized_kernel  grid (groups of 256 output pixels, frame), one thread per pixel of [h][w][3]: the four taps of the
//     bilinear resize through jpeg_pixel, lerped in float32 (jpeg_core.h: jpeg_resized_pixel) - no frame at source size is written.
#include <algorithm>

#include "carver.h"
#include "common.h"
#include "dev_mem.h"
#include "hip_handles.h"
#include "jpeg_parse.h"

namespace vbt {

constexpr int MJD_THREADS = 256;
constexpr int MJD_SLICE = 16;                                     // bytes of the scan per thread and chunk of the marker kernel
constexpr int MJD_MAX_BATCH = 1024;
constexpr size_t MJD_MAX_PACKED = (size_t)1 << 30;                // descriptors + entropy-coded bytes of one batch: 1 GiB
constexpr int MJD_SUBSEQ = 1024;                                  // VBT_MJPEG_ENTROPY_SYNC: bytes per subsequence when the caller names none ...
constexpr int MJD_AUTO_MIN_INTERVAL = 13920;                      // ... and VBT_MJPEG_ENTROPY_AUTO: the mean interval length from which a frame takes that path (profiles/mjpeg_decode.md)

// Where one frame of a batch lives in the handle's scratch and in the output: the per-frame table, behind the descriptors in the
// packed buffer, so a batch stays at one H2D copy.  Only the stills handle has one: it fills it frame by frame and its kernels (TABLE)
// read it.  The video handle packs no table; for it the marker, interval, IDCT and colour kernels are instantiated a second time with
// the geometry computed from four kernel arguments, as before the table existed.  Measured (profiles/jpeg_stills.md): with the table
// the interval kernel of a video batch was 2 to 5 % slower and the sync kernel 1 %; the sync kernel as a template was 7 % slower in
// either instantiation (12 bytes of scratch per lane appear), so it is one plain kernel that chooses between arguments and table
// by a wave-uniform branch on A.frame_blocks.
struct MjdFrame {
  uint32_t block_off;        // the frame's first block in levels and planes ...
  uint32_t block_cap;        // ... and how many it may take (a frame whose layout asks for more is not touched)
  uint32_t rst_off;          // the frame's first word in the restart table ...
  uint32_t rst_cap;          // ... and how many it may take
  uint64_t out_off;          // bytes from `out` to the frame's output
  float sy, sx;              // decode_resized: H / h and W / w (jpeg_resize_scale); 0 otherwise
};
static_assert(sizeof(MjdFrame) == 32 && sizeof(JpegDesc) % 8 == 0, "the table sits 8-byte aligned behind [B] JpegDesc");

struct MjdArgs {
  const uint8_t* packed;     // [B] JpegDesc, (TABLE: [B] MjdFrame,) then the frames' scans, each 16-byte aligned (scan_off counts from packed)
  int B, H, W;               // H, W: the video handle's frame size
  uint32_t* rst;             // video: [B][rst_cap], TABLE: per frame from rst_off - byte offset of every RSTm inside its frame's scan, in order
  uint32_t rst_cap;
  uint32_t* rst_count;       // [B]
  int32_t* status;           // [B]
  int16_t* levels;           // video: [B][frame_blocks][64], TABLE: per frame from block_off
  uint8_t* planes;           // likewise, [64] samples per block
  uint32_t frame_blocks;     // video: the batch's largest jpeg_layout().blocks
  uint8_t* out;              // video: [B][H][W][3]; TABLE: per frame from out_off, [H_f][W_f][3] or [h][w][3] of mjpegd_resized_kernel
  int h, w, swap_rb;         // mjpegd_resized_kernel: the target size and channel order
};

__device__ __forceinline__ const JpegDesc& mjd_desc(const MjdArgs& A, int f) { return ((const JpegDesc*)A.packed)[f]; }
__device__ __forceinline__ const MjdFrame& mjd_frame(const MjdArgs& A, int f) { return ((const MjdFrame*)(A.packed + (size_t)A.B * sizeof(JpegDesc)))[f]; }

// frame f's place, by table or by arithmetic
struct MjdWhere {
  size_t block_off, rst_off, out_off;
  uint32_t block_cap, rst_cap;
  float sy, sx;
};
template <bool TABLE>
__device__ __forceinline__ MjdWhere mjd_where(const MjdArgs& A, int f) {
  MjdWhere g;
  if (TABLE) {
    const MjdFrame t = mjd_frame(A, f);
    g.block_off = t.block_off; g.block_cap = t.block_cap; g.rst_off = t.rst_off; g.rst_cap = t.rst_cap; g.out_off = t.out_off; g.sy = t.sy; g.sx = t.sx;
  } else {
    g.block_off = (size_t)f * A.frame_blocks; g.block_cap = A.frame_blocks; g.rst_off = (size_t)f * A.rst_cap; g.rst_cap = A.rst_cap;
    g.out_off = (size_t)f * ((size_t)A.H * A.W) * 3; g.sy = g.sx = 0.f;
  }
  return g;
}

// exclusive prefix sum of v over the workgroup (every thread calls it); *total = the sum.  wsum: 4 ints of LDS
__device__ __forceinline__ int mjd_block_scan(int v, int* total, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();                                                // the readers of the call before are done with wsum
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < MJD_THREADS / 64; k++) {
    const int s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

template <bool TABLE>
__global__ __launch_bounds__(MJD_THREADS) void mjpegd_markers_kernel(MjdArgs A) {
  __shared__ int wsum[MJD_THREADS / 64];
  const int tid = threadIdx.x, f = blockIdx.x;
  const JpegDesc& d = mjd_desc(A, f);
  const uint8_t* scan = A.packed + d.scan_off;
  const MjdWhere g = mjd_where<TABLE>(A, f);
  const uint32_t len = d.scan_len, want = (uint32_t)d.n_int - 1;    // want <= rst_cap (video: n_int <= MCUs <= ceil(W / 8) ceil(H / 8); TABLE: the host gave the frame want words)
  uint32_t* pos = A.rst + g.rst_off;
  uint32_t base = 0;
  for (uint32_t c0 = 0; c0 < len; c0 += MJD_THREADS * MJD_SLICE) {
    const uint32_t i0 = c0 + (uint32_t)tid * MJD_SLICE;
    int cnt = 0;
#pragma unroll 4
    for (int j = 0; j < MJD_SLICE; j++) cnt += jpeg_is_rst(scan, len, i0 + j);
    int total;
    uint32_t k = base + (uint32_t)mjd_block_scan(cnt, &total, wsum);
    if (cnt) {
      for (int j = 0; j < MJD_SLICE; j++) {
        if (!jpeg_is_rst(scan, len, i0 + j)) continue;
        if (k < want && k < g.rst_cap) {
          pos[k] = i0 + j;
          if ((scan[i0 + j + 1] & 7u) != (k & 7u)) atomicMax(&A.status[f], (int)JPEG_ST_RST_ORDER);
        }
        k++;
      }
    }
    base += (uint32_t)total;
  }
  if (tid == 0) {
    A.rst_count[f] = base;
    if (base != want) atomicMax(&A.status[f], (int)JPEG_ST_RST_COUNT);
  }
}

template <bool TABLE>
__global__ __launch_bounds__(64) void mjpegd_entropy_kernel(MjdArgs A) {
  const int f = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
  const JpegDesc& d = mjd_desc(A, f);
  if (k >= d.n_int || A.rst_count[f] != (uint32_t)d.n_int - 1) return;   // (a frame whose marker count is off is not walked at all)
  const MjdWhere g = mjd_where<TABLE>(A, f);
  const uint32_t* pos = A.rst + g.rst_off;
  const uint32_t start = k ? pos[k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[k] : d.scan_len;
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > g.block_cap) return;
  const int st = jpeg_decode_interval(d, L, A.packed + d.scan_off, start, end, k, A.levels + g.block_off * 64);
  if (st) atomicMax(&A.status[f], st);
}

// exclusive prefix sums of the four words of v over the workgroup, wrapping (every thread calls it); tot: the sums.  wsum: 4 x 4 words of LDS
__device__ __forceinline__ void mjd_block_scan4(const uint32_t (&v)[4], uint32_t (&base)[4], uint32_t (&tot)[4], uint32_t (*wsum)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc[j], d, 64);
      if (lane >= d) inc[j] += o;
    }
  }
  __syncthreads();                                                // the readers of the call before are done with wsum
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < 4; j++) wsum[wave][j] = inc[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t b = 0, t = 0;
#pragma unroll
    for (int k = 0; k < MJD_THREADS / 64; k++) {
      const uint32_t s = wsum[k][j];
      if (k < wave) b += s;
      t += s;
    }
    base[j] = b + inc[j] - v[j];
    tot[j] = t;
  }
}

// Subsequences that synchronise (jpeg_core.h): grid (interval, frame), one workgroup per restart interval, its scan cut into
// subsequences of S bytes, MJD_THREADS of them (a chunk) at a time, the chunks in order.  Per chunk: every lane walks from a guess (lane
// 0 from the true state the chunk before left) and then from its left neighbour's exit until no entry changes - at most
// MJD_THREADS + 1 rounds, since lanes 0 .. r - 1 are final after round r; prefix sums of the block counts and DC sums give each
// lane its block number and predictors; a second walk stores the levels.  A chunk in which a lane recorded a status before the
// interval's last block, or in which the bits end before the blocks do, is not stored that way: thread 0 finishes the interval from the
// chunk's entry state with the statements of jpeg_decode_interval (jpeg_decode_rest).  Every loop is bounded before it starts;
// no lane waits for another except at the workgroup's barriers, which every thread reaches.
// info: { most rounds of any chunk, intervals finished by the single lane } of the batch.
__global__ __launch_bounds__(MJD_THREADS) void mjpegd_entropy_sync_kernel(MjdArgs A, int S, int32_t* info) {
  static_assert(sizeof(JpegHuff) % 4 == 0 && offsetof(JpegDesc, ac) == offsetof(JpegDesc, dc) + 2 * sizeof(JpegHuff) && offsetof(JpegDesc, dc) % 4 == 0,
                "the four tables are staged as one run of words");
  __shared__ JpegHuff sHuff[4];
  __shared__ JpegSyncState sExit[MJD_THREADS];
  __shared__ uint32_t sSum[MJD_THREADS / 64][4];
  const int tid = threadIdx.x, f = blockIdx.y, k = blockIdx.x;
  const JpegDesc& d = mjd_desc(A, f);
  if (k >= d.n_int || A.rst_count[f] != (uint32_t)d.n_int - 1) return;   // (per workgroup: every thread returns or none does)
  MjdWhere g;                                                       // no template here (see MjdFrame): a wave-uniform branch, frame_blocks != 0 is the video handle
  if (A.frame_blocks) g = mjd_where<false>(A, f);
  else g = mjd_where<true>(A, f);
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > g.block_cap) return;
  {
    const uint32_t* src = (const uint32_t*)d.dc;
    uint32_t* dst = (uint32_t*)sHuff;
    for (int i = tid; i < (int)(4 * sizeof(JpegHuff) / 4); i += MJD_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t* pos = A.rst + g.rst_off;
  const uint32_t start = k ? pos[k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[k] : d.scan_len;
  const uint8_t* scan = A.packed + d.scan_off;
  int16_t* levels = A.levels + g.block_off * 64;
  const uint32_t len = end > start ? end - start : 0, lanes = len ? (len + (uint32_t)S - 1) / (uint32_t)S : 1;
  const uint32_t nblocks = jpeg_interval_blocks(d, k);
  const int m0 = k * d.ri, max_syms = 8 * S + 32;
  JpegSyncState carry;                                              // the true state in front of the chunk, the blocks complete and the DC sums there
  carry.pos = start; carry.buk = 0;
  uint32_t cb = 0, cdc[3] = {0, 0, 0};
  int most = 0;
  for (uint32_t c0 = 0; c0 < lanes; c0 += MJD_THREADS) {
    const bool active = c0 + (uint32_t)tid < lanes;
    const uint32_t first = active ? start + (c0 + (uint32_t)tid) * (uint32_t)S : end;
    const uint32_t limit = active && end - first > (uint32_t)S ? first + (uint32_t)S : end;
    JpegSyncState entry = tid == 0 || !active ? carry : jpeg_sync_cold(scan, first);
    JpegSyncWalk w;
    w.exit = entry; w.blocks = 0; w.dc[0] = w.dc[1] = w.dc[2] = 0; w.bad_at = JPEG_SYNC_NONE;
    int rounds = 0;
    for (int r = 0; r <= MJD_THREADS; r++) {
      bool go = active && r == 0;
      if (r > 0 && active && tid > 0) {
        const JpegSyncState e = sExit[tid - 1];
        if (!jpeg_sync_same(e, entry)) { entry = e; go = true; }
      }
      if (!__syncthreads_or(go)) break;                             // (also: every read of sExit is done before the writes below)
      if (go) {
        w = jpeg_sync_walk<false>(d, L, sHuff, scan, end, entry, limit, max_syms, 0, 0, 0, nullptr, nullptr);
        sExit[tid] = w.exit;
      }
      rounds++;
      __syncthreads();
    }
    most = rounds > most ? rounds : most;
    const uint32_t v[4] = {w.blocks, w.dc[0], w.dc[1], w.dc[2]};
    uint32_t base[4], tot[4];
    mjd_block_scan4(v, base, tot, sSum);
    base[0] += cb; base[1] += cdc[0]; base[2] += cdc[1]; base[3] += cdc[2];
    const bool last = lanes - c0 <= (uint32_t)MJD_THREADS;
    const bool dirty = (w.bad_at != JPEG_SYNC_NONE && base[0] + w.bad_at < nblocks) || (last && cb + tot[0] < nblocks);
    if (__syncthreads_or(dirty)) {
      if (tid == 0) {
        const int st = jpeg_decode_rest(d, L, scan, end, k, carry, cb, cdc, levels);
        if (st) atomicMax(&A.status[f], st);
        atomicAdd(&info[1], 1);
      }
      break;
    }
    if (active) jpeg_sync_walk<true>(d, L, sHuff, scan, end, entry, limit, max_syms, m0, base[0], nblocks, &base[1], levels);
    carry = sExit[last ? lanes - c0 - 1 : MJD_THREADS - 1];          // (the next chunk writes sExit only behind its first barrier)
    cb += tot[0]; cdc[0] += tot[1]; cdc[1] += tot[2]; cdc[2] += tot[3];
    if (cb >= nblocks) break;                                       // what is left is padding
  }
  if (tid == 0) atomicMax(&info[0], most);
}

template <bool TABLE>
__global__ __launch_bounds__(MJD_THREADS) void mjpegd_idct_kernel(MjdArgs A) {
  __shared__ uint16_t sQ[4][64];
  const int tid = threadIdx.x, f = blockIdx.y;
  const JpegDesc& d = mjd_desc(A, f);
  sQ[tid >> 6][tid & 63] = d.q[tid >> 6][tid & 63];
  __syncthreads();
  const MjdWhere g = mjd_where<TABLE>(A, f);
  const JpegLayout L = jpeg_layout(d);
  const uint32_t bi = blockIdx.x * MJD_THREADS + tid;
  if (bi >= L.blocks || L.blocks > g.block_cap) return;
  const int c = d.ncomp == 3 ? (bi >= L.boff[2] ? 2 : bi >= L.boff[1] ? 1 : 0) : 0;
  const uint32_t local = bi - L.boff[c], by = local / (uint32_t)L.bw[c], bx = local % (uint32_t)L.bw[c];
  const uint4* lv = (const uint4*)(A.levels + (g.block_off + bi) * 64);
  const uint16_t* q = sQ[d.tq[c] & 3];
  int32_t co[64];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint4 v = lv[j];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 8; i++) co[j * 8 + i] = (int32_t)(int16_t)(w[i >> 1] >> ((i & 1) * 16)) * (int32_t)q[j * 8 + i];
  }
  uint8_t px[64];
  jpeg_idct_islow(co, px);
  const size_t pw = (size_t)L.bw[c] * 8;
  uint8_t* dst = A.planes + (g.block_off + L.boff[c]) * 64 + (size_t)by * 8 * pw + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    uint2 o;
    o.x = px[r * 8] | (px[r * 8 + 1] << 8) | (px[r * 8 + 2] << 16) | ((uint32_t)px[r * 8 + 3] << 24);
    o.y = px[r * 8 + 4] | (px[r * 8 + 5] << 8) | (px[r * 8 + 6] << 16) | ((uint32_t)px[r * 8 + 7] << 24);
    *(uint2*)(dst + r * pw) = o;
  }
}

template <bool TABLE>
__global__ __launch_bounds__(MJD_THREADS) void mjpegd_colour_kernel(MjdArgs A) {
  const int f = blockIdx.y;
  const JpegDesc& d = mjd_desc(A, f);
  const MjdWhere g = mjd_where<TABLE>(A, f);
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > g.block_cap) return;
  const int H = TABLE ? d.H : A.H, W = TABLE ? d.W : A.W;          // (video: the parser insisted on the handle's size)
  const size_t npix = (size_t)H * W, p0 = ((size_t)blockIdx.x * MJD_THREADS + threadIdx.x) * 4;   // (TABLE: the grid covers the batch's largest frame)
  if (p0 >= npix) return;
  const uint8_t* planes = A.planes + g.block_off * 64;
  uint8_t* dst = A.out + g.out_off + p0 * 3;
  const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
  uint8_t rgb[12];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const size_t p = p0 + i < npix ? p0 + i : npix - 1;
    jpeg_pixel(d, L, planes, (int)(p / (size_t)W), (int)(p % (size_t)W), rgb + 3 * i);
  }
  if (n == 4 && ((uintptr_t)dst & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 3; i++)
      ((uint32_t*)dst)[i] = rgb[4 * i] | (rgb[4 * i + 1] << 8) | (rgb[4 * i + 2] << 16) | ((uint32_t)rgb[4 * i + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 12; i++)
      if (i < 3 * n) dst[i] = rgb[i];
  }
}

// In the colour kernel's place (vbt_jpeg_stills_decode_resized): grid (groups of 256 output pixels, frame), one thread per pixel of
// the [h][w][3] network input, consecutive lanes = consecutive output columns as in yuv_resize_kernel - a wave reads a luma row
// segment per tap row and the chroma rows under it.  The statement is jpeg_resized_pixel (jpeg_core.h); the frame at source size
// is never written.
__global__ __launch_bounds__(MJD_THREADS) void mjpegd_resized_kernel(MjdArgs A) {
  const int f = blockIdx.y;
  const JpegDesc& d = mjd_desc(A, f);
  const MjdWhere g = mjd_where<true>(A, f);
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > g.block_cap) return;
  const uint32_t idx = blockIdx.x * MJD_THREADS + threadIdx.x;      // h w <= 2^24 (the host checked)
  if (idx >= (uint32_t)A.h * (uint32_t)A.w) return;
  const int oy = (int)(idx / (uint32_t)A.w), ox = (int)(idx % (uint32_t)A.w);
  uint8_t px[3];
  jpeg_resized_pixel(d, L, A.planes + g.block_off * 64, g.sy, g.sx, oy, ox, A.swap_rb, px);
  uint8_t* dst = A.out + g.out_off + (size_t)idx * 3;
  dst[0] = px[0]; dst[1] = px[1]; dst[2] = px[2];
}

}  // namespace vbt

using namespace vbt;

// what the two handles share: the scratch, the staging of the compressed bytes, the entropy settings and the launches (mjd_enqueue)
struct MjdHandle {
  int device = 0, max_batch = 0;
  size_t blocks_cap = 0, rst_words = 0;  // the scratch: blocks of levels and planes, words of restart table
  uint64_t last_upload = 0;              // bytes of the last batch's H2D copy
  DevBuf<uint8_t> blob;                  // status | rst_count | rst | levels | planes | info in one allocation
  DevBuf<uint8_t> packed;                // the batch's descriptors and scans on the device; grows on demand up to MJD_MAX_PACKED
  size_t packed_cap = 0;                 // (0 whenever packed is empty; stage_cap likewise)
  PinnedBuf<uint8_t> stage[2];           // pinned staging, used in turn
  size_t stage_cap[2] = {0, 0};
  Event copied[2];                       // recorded behind the H2D copy out of stage[i]: the host waits for it before it refills stage[i]
  bool in_flight[2] = {false, false};
  int next = 0, last_B = 0;
  Event stamp[7];                        // VBT_MJPEG_DECODE_STAMPS=1: around each stage of a decode (vbt_mjpeg_decode_stage_ms)
  bool stamps = false;
  int entropy = VBT_MJPEG_ENTROPY_AUTO, subseq = 0;   // vbt_mjpeg_decoder_set_entropy
  int last_path = 0, last_subseq = 0;    // of the last batch
  int32_t* info = nullptr;               // in blob: { most rounds of any chunk, intervals the single lane finished } of the last batch in SYNC
  std::vector<JpegDesc> descs;
  std::vector<MjdFrame> geom;
  MjdArgs args{};
  ~MjdHandle() {
    if (blob) (void)hipSetDevice(device);   // (the members go after this: the blob's free waits for the kernels still using it)
  }
};

// one frame size: every frame of a batch gets the same share of the scratch
struct vbt_mjpeg_decoder : MjdHandle {
  int H = 0, W = 0;
  size_t frame_blocks = 0, rst_cap = 0;
};

// every frame its own size: the frames of a batch share a budget of blocks.  Nothing is allocated before the first batch, so that
// every refusal of an argument, a header or a batch over the budget is made without a device; blob tells whether it has been
struct vbt_jpeg_stills : MjdHandle {
  size_t block_budget = 0;
};

namespace {

constexpr size_t STILLS_MAX_BUDGET = (size_t)1 << 24;              // blocks: one 16384 x 16384 frame at 4:4:4 takes 3 x 2^22
constexpr int STILLS_MAX_TARGET = 4096;                            // h, w of decode_resized

size_t align256(size_t v) { return Carver<256>::align(v); }
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

int sampling_code(const JpegDesc& d) { return (d.hs << 4) | d.vs; }

// the scratch for `blocks` blocks and `rst_words` restart positions, the device buffer of the compressed bytes (packed_init bytes to
// begin with), the events.  The caller has selected the device; after an error the handle holds none of them
hipError_t mjd_alloc(MjdHandle* m, size_t blocks, size_t rst_words, size_t packed_init, size_t* bytes) {
  const size_t B = (size_t)m->max_batch;
  Carver<256> C;
  const auto status = C.add<int32_t>(B);
  const auto count = C.add<uint32_t>(B), rst = C.add<uint32_t>(rst_words);
  const auto levels = C.add<int16_t>(blocks * 64);
  const auto planes = C.add<uint8_t>(blocks * 64);
  const auto info = C.add<int32_t>(64);
  m->blocks_cap = blocks; m->rst_words = rst_words;
  const size_t packed_cap = std::min(MJD_MAX_PACKED, align256(packed_init));
  *bytes = C.bytes() + packed_cap;
  hipError_t e = m->blob.alloc(C.bytes());
  if (e == hipSuccess) e = m->packed.alloc(packed_cap);
  for (int i = 0; i < 2 && e == hipSuccess; i++) e = m->copied[i].create(hipEventDisableTiming);
  const char* env = getenv("VBT_MJPEG_DECODE_STAMPS");
  const bool stamps = env && env[0] == '1';
  for (int i = 0; i < 7 && stamps && e == hipSuccess; i++) e = m->stamp[i].create(hipEventDefault);
  if (e != hipSuccess) {
    m->blob.reset(); m->packed.reset();
    for (Event& ev : m->copied) ev.reset();
    for (Event& ev : m->stamp) ev.reset();
    return e;
  }
  m->packed_cap = packed_cap;
  m->stamps = stamps;
  uint8_t* const blob = m->blob.get();
  MjdArgs& A = m->args;
  A.status = C.ptr(blob, status); A.rst_count = C.ptr(blob, count); A.rst = C.ptr(blob, rst);
  A.levels = C.ptr(blob, levels); A.planes = C.ptr(blob, planes);
  m->info = C.ptr(blob, info);
  return e;
}

// what the parse loop of a batch collects
struct MjdBatch {
  size_t total = 0;          // bytes of the packed buffer: descriptors, geometry table, scans
  size_t blocks = 0;         // blocks of levels to clear: the frames' shares lie one behind the other from block 0
  uint32_t max_int = 1, max_blocks = 1;
  size_t max_npix = 1;
  bool sync = false;
};

// the descriptors and, for the stills handle, the geometry table in front of the scans
size_t mjd_head_bytes(int B, bool table) { return align16((size_t)B * (sizeof(JpegDesc) + (table ? sizeof(MjdFrame) : 0))); }

// one header into m->descs[i] and the batch's sums; false: refused, *why says it
bool mjd_parse_one(MjdHandle* m, MjdBatch* b, int i, const uint8_t* bytes, uint64_t n, int H, int W, std::string* why) {
  JpegDesc& d = m->descs[(size_t)i];
  if (!jpeg_parse(bytes, n, H, W, &d, why)) return false;
  b->max_int = std::max(b->max_int, (uint32_t)d.n_int);
  if (m->entropy == VBT_MJPEG_ENTROPY_AUTO && d.scan_len / (uint32_t)d.n_int >= (uint32_t)MJD_AUTO_MIN_INTERVAL) b->sync = true;
  b->max_blocks = std::max(b->max_blocks, jpeg_layout(d).blocks);
  b->max_npix = std::max(b->max_npix, (size_t)d.H * (size_t)d.W);
  b->total += align16(d.scan_len);
  return true;
}

// the four launches of a batch, the kernels reading the geometry table (TABLE) or computing it; h > 0: mjpegd_resized_kernel is the last
template <bool TABLE, class Stamp>
hipError_t mjd_launch(const MjdArgs& A, const MjdBatch& b, int B, int S, int32_t* info, hipStream_t st, Stamp stamp) {
  mjpegd_markers_kernel<TABLE><<<dim3((unsigned)B), MJD_THREADS, 0, st>>>(A);
  if (hipError_t e = stamp(3)) return e;
  if (b.sync) mjpegd_entropy_sync_kernel<<<dim3(b.max_int, (unsigned)B), MJD_THREADS, 0, st>>>(A, S, info);
  else mjpegd_entropy_kernel<TABLE><<<dim3((b.max_int + 63) / 64, (unsigned)B), 64, 0, st>>>(A);
  if (hipError_t e = stamp(4)) return e;
  mjpegd_idct_kernel<TABLE><<<dim3((b.max_blocks + MJD_THREADS - 1) / MJD_THREADS, (unsigned)B), MJD_THREADS, 0, st>>>(A);
  if (hipError_t e = stamp(5)) return e;
  if (TABLE && A.h > 0) {
    const size_t groups = ((size_t)A.h * A.w + MJD_THREADS - 1) / MJD_THREADS;
    mjpegd_resized_kernel<<<dim3((unsigned)groups, (unsigned)B), MJD_THREADS, 0, st>>>(A);
  } else {
    const size_t groups = (b.max_npix + MJD_THREADS * 4 - 1) / (MJD_THREADS * 4);
    mjpegd_colour_kernel<TABLE><<<dim3((unsigned)groups, (unsigned)B), MJD_THREADS, 0, st>>>(A);
  }
  return stamp(6);
}

// The batch whose headers are m->descs[0 .. B): pack, one H2D copy, the launches.  table: the stills handle's geometry, m->geom[0 .. B),
// travels behind the descriptors and the kernels read it (A0.frame_blocks = 0); the video handle's A0 carries its geometry as arguments.
int mjd_enqueue(MjdHandle* m, const char* who, const MjdBatch& b, const uint8_t* host_bytes, const uint64_t* offsets, int B, bool table, const MjdArgs& A0,
                void* stream) {
  const size_t total = b.total;
  VBT_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)stream;
  const int s = m->next;
  if (m->in_flight[s]) {                                          // host-side gate: the copy that last read this staging buffer is done
    VBT_HIP_CHECK(hipEventSynchronize(m->copied[s].get()));
    m->in_flight[s] = false;
  }
  if (total > m->stage_cap[s]) {
    const size_t cap = std::min(MJD_MAX_PACKED, align256(total + total / 4));
    m->stage_cap[s] = 0;
    VBT_HIP_CHECK(m->stage[s].alloc(cap));
    m->stage_cap[s] = cap;
  }
  if (total > m->packed_cap) {                                    // growth frees the old buffer, which waits for the work that reads it
    const size_t cap = std::min(MJD_MAX_PACKED, align256(total + total / 4));
    m->packed_cap = 0;
    const hipError_t e = m->packed.alloc(cap);
    if (e != hipSuccess) { set_error("%s: %zu bytes of device memory for the compressed frames: %s", who, cap, hipGetErrorString(e)); return VBT_ERR_HIP; }
    m->packed_cap = cap;
  }
  uint8_t* pk = m->stage[s].get();
  size_t at = mjd_head_bytes(B, table);
  for (int i = 0; i < B; i++) {
    JpegDesc& d = m->descs[(size_t)i];
    memcpy(pk + at, host_bytes + offsets[i] + d.scan_off, d.scan_len);
    d.scan_off = at;
    at += align16(d.scan_len);
  }
  memcpy(pk, m->descs.data(), (size_t)B * sizeof(JpegDesc));
  if (table) memcpy(pk + (size_t)B * sizeof(JpegDesc), m->geom.data(), (size_t)B * sizeof(MjdFrame));
  auto stamp = [&](int i) { return m->stamps ? hipEventRecord(m->stamp[i].get(), st) : hipSuccess; };
  VBT_HIP_CHECK(stamp(0));
  VBT_HIP_CHECK(hipMemcpyAsync(m->packed.get(), pk, total, hipMemcpyHostToDevice, st));
  VBT_HIP_CHECK(hipEventRecord(m->copied[s].get(), st));
  VBT_HIP_CHECK(stamp(1));
  m->in_flight[s] = true;
  m->next = s ^ 1;
  m->last_upload = total;
  MjdArgs A = A0;
  A.packed = m->packed.get(); A.B = B;
  VBT_HIP_CHECK(hipMemsetAsync(A.status, 0, (size_t)B * 4, st));
  VBT_HIP_CHECK(hipMemsetAsync(A.levels, 0, b.blocks * 128, st));
  if (b.sync) VBT_HIP_CHECK(hipMemsetAsync(m->info, 0, 8, st));
  VBT_HIP_CHECK(stamp(2));
  const int S = m->subseq ? m->subseq : MJD_SUBSEQ;
  VBT_HIP_CHECK(table ? mjd_launch<true>(A, b, B, S, m->info, st, stamp) : mjd_launch<false>(A, b, B, S, m->info, st, stamp));
  VBT_HIP_CHECK(hipGetLastError());
  m->last_B = B;
  m->last_path = b.sync ? VBT_MJPEG_ENTROPY_SYNC : VBT_MJPEG_ENTROPY_INTERVAL;
  m->last_subseq = b.sync ? S : 0;
  return VBT_OK;
}

int mjd_set_entropy(MjdHandle* m, const char* who, int mode, int subseq_bytes) {
  if (!m) { set_error("%s: handle is NULL", who); return VBT_ERR_ARG; }
  if (mode < VBT_MJPEG_ENTROPY_AUTO || mode > VBT_MJPEG_ENTROPY_SYNC) { set_error("%s: mode %d is none of AUTO (0), INTERVAL (1), SYNC (2)", who, mode); return VBT_ERR_ARG; }
  if (subseq_bytes && (subseq_bytes < 4 || subseq_bytes > 4096 || (subseq_bytes & (subseq_bytes - 1)))) {
    set_error("%s: subseq_bytes %d is neither 0 nor a power of two in 4..4096", who, subseq_bytes);
    return VBT_ERR_ARG;
  }
  m->entropy = mode;
  m->subseq = subseq_bytes;
  return VBT_OK;
}

int mjd_get_entropy(MjdHandle* m, const char* who, int* mode, int* subseq_bytes, int* auto_min_interval_bytes) {
  if (!m) { set_error("%s: handle is NULL", who); return VBT_ERR_ARG; }
  if (mode) *mode = m->entropy;
  if (subseq_bytes) *subseq_bytes = m->subseq ? m->subseq : MJD_SUBSEQ;
  if (auto_min_interval_bytes) *auto_min_interval_bytes = MJD_AUTO_MIN_INTERVAL;
  return VBT_OK;
}

int mjd_status(MjdHandle* m, const char* who, const char* first, int32_t* status, void* stream) {
  if (!m || !status) { set_error("%s: bad argument", who); return VBT_ERR_ARG; }
  if (!m->last_B) { set_error("%s: no batch has been decoded (%s first)", who, first); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  VBT_HIP_CHECK(hipMemcpy(status, m->args.status, (size_t)m->last_B * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int mjd_entropy_info(MjdHandle* m, const char* who, const char* first, int32_t* info4, void* stream) {
  if (!m || !info4) { set_error("%s: bad argument", who); return VBT_ERR_ARG; }
  if (!m->last_B) { set_error("%s: no batch has been decoded (%s first)", who, first); return VBT_ERR_STATE; }
  info4[0] = m->last_path; info4[1] = m->last_subseq; info4[2] = info4[3] = 0;
  VBT_HIP_CHECK(hipSetDevice(m->device));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  if (m->last_path == VBT_MJPEG_ENTROPY_SYNC) VBT_HIP_CHECK(hipMemcpy(info4 + 2, m->info, 8, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int mjd_stage_ms(MjdHandle* m, const char* who, float* ms6) {
  if (!m || !ms6) { set_error("%s: bad argument", who); return VBT_ERR_ARG; }
  if (!m->stamps || !m->last_B) { set_error("%s: needs VBT_MJPEG_DECODE_STAMPS=1 at create and a decoded batch", who); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  VBT_HIP_CHECK(hipEventSynchronize(m->stamp[6].get()));
  for (int i = 0; i < 6; i++) VBT_HIP_CHECK(hipEventElapsedTime(&ms6[i], m->stamp[i].get(), m->stamp[i + 1].get()));
  return VBT_OK;
}

}  // namespace

extern "C" {

int vbt_jpeg_probe(const uint8_t* bytes, uint64_t n, int* H, int* W, int* components, int* sampling) {
  if (!bytes) { set_error("vbt_jpeg_probe: bytes is NULL"); return VBT_ERR_ARG; }
  JpegDesc d;
  std::string why;
  if (!jpeg_parse(bytes, n, 0, 0, &d, &why)) { set_error("vbt_jpeg_probe: %s", why.c_str()); return VBT_ERR_IO; }
  if (H) *H = d.H;
  if (W) *W = d.W;
  if (components) *components = d.ncomp;
  if (sampling) *sampling = sampling_code(d);
  return VBT_OK;
}

int vbt_jpeg_blocks(const uint8_t* bytes, uint64_t n, uint32_t* blocks) {
  if (!bytes || !blocks) { set_error("vbt_jpeg_blocks: bytes or blocks is NULL"); return VBT_ERR_ARG; }
  JpegDesc d;
  std::string why;
  if (!jpeg_parse(bytes, n, 0, 0, &d, &why)) { set_error("vbt_jpeg_blocks: %s", why.c_str()); return VBT_ERR_IO; }
  *blocks = jpeg_layout(d).blocks;
  return VBT_OK;
}

// ---- the video handle: one frame size
int vbt_mjpeg_decoder_create(int device, int H, int W, int max_batch, vbt_mjpeg_decoder** out) {
  if (!out) { set_error("vbt_mjpeg_decoder_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (H < 1 || W < 1 || H > JPEG_MAX_SIDE || W > JPEG_MAX_SIDE) { set_error("vbt_mjpeg_decoder_create: frames of 1..16384 pixels a side, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (max_batch < 1 || max_batch > MJD_MAX_BATCH) { set_error("vbt_mjpeg_decoder_create: max_batch %d outside 1..%d", max_batch, MJD_MAX_BATCH); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_mjpeg_decoder_create", device)) return rc;
  std::unique_ptr<vbt_mjpeg_decoder> m(new vbt_mjpeg_decoder());
  m->device = device; m->H = H; m->W = W; m->max_batch = max_batch;
  m->frame_blocks = (size_t)jpeg_max_blocks(H, W);
  m->rst_cap = (size_t)((W + 7) / 8) * (size_t)((H + 7) / 8);
  const size_t B = (size_t)max_batch;
  size_t bytes = 0;
  const hipError_t e = mjd_alloc(m.get(), B * m->frame_blocks, B * m->rst_cap, B * sizeof(JpegDesc) + B * (4096 + (size_t)H * W / 4), &bytes);
  if (e != hipSuccess) {
    set_error("vbt_mjpeg_decoder_create: %zu bytes of device memory for %d frames of %d x %d: %s", bytes, max_batch, W, H, hipGetErrorString(e));
    return VBT_ERR_HIP;
  }
  *out = m.release();
  return VBT_OK;
}

void vbt_mjpeg_decoder_destroy(vbt_mjpeg_decoder* m) { delete m; }

int vbt_mjpeg_decode(vbt_mjpeg_decoder* m, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* frames_dev_out, void* stream) {
  if (!m || !host_bytes || !offsets || !frames_dev_out || B < 1) { set_error("vbt_mjpeg_decode: bad argument (handle, bytes, offsets, frames, B >= 1)"); return VBT_ERR_ARG; }
  if (B > m->max_batch) { set_error("vbt_mjpeg_decode: %d frames, the handle was created for %d", B, m->max_batch); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < B; i++)
    if (offsets[i + 1] < offsets[i]) { set_error("vbt_mjpeg_decode: offsets[%d] > offsets[%d]", i, i + 1); return VBT_ERR_ARG; }
  // ---- every header first: a refusal leaves nothing enqueued
  m->descs.resize((size_t)B);
  MjdBatch b;
  b.total = mjd_head_bytes(B, false);
  b.sync = m->entropy == VBT_MJPEG_ENTROPY_SYNC;
  for (int i = 0; i < B; i++) {
    std::string why;
    if (!mjd_parse_one(m, &b, i, host_bytes + offsets[i], offsets[i + 1] - offsets[i], m->H, m->W, &why)) {
      set_error("vbt_mjpeg_decode: frame %d of the batch: %s", i, why.c_str());
      return VBT_ERR_IO;
    }
  }
  if (b.total > MJD_MAX_PACKED || b.max_blocks > m->frame_blocks) {
    set_error("vbt_mjpeg_decode: %zu compressed bytes in one batch, the bound is %zu: decode fewer frames at a time", b.total, MJD_MAX_PACKED);
    return VBT_ERR_CAPACITY;
  }
  b.blocks = (size_t)B * b.max_blocks;                          // frame f takes the batch's largest block count from block f max_blocks on
  MjdArgs A = m->args;
  A.H = m->H; A.W = m->W; A.rst_cap = (uint32_t)m->rst_cap; A.frame_blocks = b.max_blocks; A.out = frames_dev_out;
  A.h = A.w = A.swap_rb = 0;
  return mjd_enqueue(m, "vbt_mjpeg_decode", b, host_bytes, offsets, B, false, A, stream);
}

int vbt_mjpeg_decoder_set_entropy(vbt_mjpeg_decoder* m, int mode, int subseq_bytes) { return mjd_set_entropy(m, "vbt_mjpeg_decoder_set_entropy", mode, subseq_bytes); }

int vbt_mjpeg_decoder_get_entropy(vbt_mjpeg_decoder* m, int* mode, int* subseq_bytes, int* auto_min_interval_bytes) {
  return mjd_get_entropy(m, "vbt_mjpeg_decoder_get_entropy", mode, subseq_bytes, auto_min_interval_bytes);
}

int vbt_mjpeg_decode_status(vbt_mjpeg_decoder* m, int32_t* status, void* stream) { return mjd_status(m, "vbt_mjpeg_decode_status", "vbt_mjpeg_decode", status, stream); }

int vbt_mjpeg_decode_entropy_info(vbt_mjpeg_decoder* m, int32_t* info4, void* stream) {
  return mjd_entropy_info(m, "vbt_mjpeg_decode_entropy_info", "vbt_mjpeg_decode", info4, stream);
}

int vbt_mjpeg_decode_stage_ms(vbt_mjpeg_decoder* m, float* ms6) { return mjd_stage_ms(m, "vbt_mjpeg_decode_stage_ms", ms6); }

// ---- the stills handle: every frame its own size
int vbt_jpeg_stills_create(int device, int max_batch, uint64_t block_budget, vbt_jpeg_stills** out) {
  if (!out) { set_error("vbt_jpeg_stills_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (device < 0) { set_error("vbt_jpeg_stills_create: device %d", device); return VBT_ERR_ARG; }
  if (max_batch < 1 || max_batch > MJD_MAX_BATCH) { set_error("vbt_jpeg_stills_create: max_batch %d outside 1..%d", max_batch, MJD_MAX_BATCH); return VBT_ERR_ARG; }
  if (block_budget < 1 || block_budget > STILLS_MAX_BUDGET) {
    set_error("vbt_jpeg_stills_create: a budget of %llu blocks, outside 1..%zu", (unsigned long long)block_budget, STILLS_MAX_BUDGET);
    return VBT_ERR_ARG;
  }
  vbt_jpeg_stills* m = new vbt_jpeg_stills();
  m->device = device; m->max_batch = max_batch; m->block_budget = (size_t)block_budget;
  *out = m;
  return VBT_OK;
}

void vbt_jpeg_stills_destroy(vbt_jpeg_stills* m) { delete m; }

}  // extern "C"

namespace {

// Both stills entry points.  h > 0: straight to [B][h][w][3] at out; otherwise frame i to out + out_offsets[i].  Arguments, headers
// and the budget are checked before the first device call.
int stills_run(vbt_jpeg_stills* m, const char* who, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* out, const uint64_t* out_offsets, int h,
               int w, int swap_rb, void* stream) {
  const bool resized = out_offsets == nullptr;
  if (!m || !host_bytes || !offsets || !out) { set_error("%s: bad argument (handle, bytes, offsets and the output must not be NULL)", who); return VBT_ERR_ARG; }
  if (B < 1) { set_error("%s: B = %d, at least one frame", who, B); return VBT_ERR_ARG; }
  if (B > m->max_batch) { set_error("%s: %d frames, the handle was created for %d", who, B, m->max_batch); return VBT_ERR_CAPACITY; }
  if (resized && (h < 1 || w < 1 || h > STILLS_MAX_TARGET || w > STILLS_MAX_TARGET)) { set_error("%s: a target of 1..%d pixels a side, got %d x %d", who, STILLS_MAX_TARGET, w, h); return VBT_ERR_ARG; }
  for (int i = 0; i < B; i++)
    if (offsets[i + 1] < offsets[i]) { set_error("%s: offsets[%d] > offsets[%d]", who, i, i + 1); return VBT_ERR_ARG; }
  m->descs.resize((size_t)B);
  m->geom.resize((size_t)B);
  MjdBatch b;
  b.total = mjd_head_bytes(B, true);
  b.sync = m->entropy == VBT_MJPEG_ENTROPY_SYNC;
  size_t blocks = 0, rst = 0;
  for (int i = 0; i < B; i++) {
    std::string why;
    if (!mjd_parse_one(m, &b, i, host_bytes + offsets[i], offsets[i + 1] - offsets[i], 0, 0, &why)) {
      set_error("%s: frame %d of the batch: %s", who, i, why.c_str());
      return VBT_ERR_IO;
    }
    const JpegDesc& d = m->descs[(size_t)i];
    MjdFrame& g = m->geom[(size_t)i];
    g.block_off = (uint32_t)blocks; g.block_cap = jpeg_layout(d).blocks;            // (block_off <= the budget <= 2^24 when the batch is taken)
    g.rst_off = (uint32_t)rst; g.rst_cap = (uint32_t)d.n_int - 1;                    // n_int - 1 < MCUs <= blocks: the table's words never run out before the blocks do
    g.out_off = resized ? (uint64_t)i * (uint64_t)h * (uint64_t)w * 3 : out_offsets[i];
    g.sy = resized ? jpeg_resize_scale(d.H, h) : 0.f;
    g.sx = resized ? jpeg_resize_scale(d.W, w) : 0.f;
    blocks += g.block_cap;
    rst += g.rst_cap;
  }
  if (blocks > m->block_budget) {
    set_error("%s: the batch takes %zu blocks, the handle's budget is %zu: decode fewer files at a time (vbt_jpeg_blocks)", who, blocks, m->block_budget);
    return VBT_ERR_CAPACITY;
  }
  if (b.total > MJD_MAX_PACKED) {
    set_error("%s: %zu compressed bytes in one batch, the bound is %zu: decode fewer files at a time", who, b.total, MJD_MAX_PACKED);
    return VBT_ERR_CAPACITY;
  }
  b.blocks = blocks;
  if (!m->blob) {
    if (int rc = use_device(who, m->device)) return rc;
    size_t bytes = 0;
    const hipError_t e = mjd_alloc(m, m->block_budget, m->block_budget, (size_t)m->max_batch * (sizeof(JpegDesc) + sizeof(MjdFrame) + 4096) + 16 * m->block_budget, &bytes);
    if (e != hipSuccess) {                                          // (the handle holds nothing: the next batch tries again)
      set_error("%s: %zu bytes of device memory for a budget of %zu blocks and %d frames: %s", who, bytes, m->block_budget, m->max_batch, hipGetErrorString(e));
      return VBT_ERR_HIP;
    }
  }
  MjdArgs A = m->args;
  A.H = A.W = 0; A.rst_cap = 0; A.frame_blocks = 0; A.out = out;
  A.h = resized ? h : 0; A.w = resized ? w : 0; A.swap_rb = swap_rb ? 1 : 0;
  return mjd_enqueue(m, who, b, host_bytes, offsets, B, true, A, stream);
}

}  // namespace

extern "C" {

int vbt_jpeg_stills_decode_resized(vbt_jpeg_stills* m, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* dst_dev, int h, int w, int swap_rb,
                                   void* stream) {
  return stills_run(m, "vbt_jpeg_stills_decode_resized", host_bytes, offsets, B, dst_dev, nullptr, h, w, swap_rb, stream);
}

int vbt_jpeg_stills_decode(vbt_jpeg_stills* m, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* frames_dev_out, const uint64_t* out_offsets,
                           void* stream) {
  if (!out_offsets) { set_error("vbt_jpeg_stills_decode: out_offsets is NULL"); return VBT_ERR_ARG; }
  return stills_run(m, "vbt_jpeg_stills_decode", host_bytes, offsets, B, frames_dev_out, out_offsets, 0, 0, 0, stream);
}

int vbt_jpeg_stills_set_entropy(vbt_jpeg_stills* m, int mode, int subseq_bytes) { return mjd_set_entropy(m, "vbt_jpeg_stills_set_entropy", mode, subseq_bytes); }

int vbt_jpeg_stills_get_entropy(vbt_jpeg_stills* m, int* mode, int* subseq_bytes, int* auto_min_interval_bytes) {
  return mjd_get_entropy(m, "vbt_jpeg_stills_get_entropy", mode, subseq_bytes, auto_min_interval_bytes);
}

int vbt_jpeg_stills_status(vbt_jpeg_stills* m, int32_t* status, void* stream) { return mjd_status(m, "vbt_jpeg_stills_status", "a decode", status, stream); }

int vbt_jpeg_stills_entropy_info(vbt_jpeg_stills* m, int32_t* info4, void* stream) { return mjd_entropy_info(m, "vbt_jpeg_stills_entropy_info", "a decode", info4, stream); }

int vbt_jpeg_stills_stage_ms(vbt_jpeg_stills* m, float* ms6) { return mjd_stage_ms(m, "vbt_jpeg_stills_stage_ms", ms6); }

int vbt_jpeg_stills_uploaded_bytes(vbt_jpeg_stills* m, uint64_t* bytes) {
  if (!m || !bytes) { set_error("vbt_jpeg_stills_uploaded_bytes: bad argument"); return VBT_ERR_ARG; }
  *bytes = m->last_B ? m->last_upload : 0;
  return VBT_OK;
}

}  // extern "C"

