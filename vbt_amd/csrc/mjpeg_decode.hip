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
#include <algorithm>

#include "common.h"
#include "jpeg_parse.h"

namespace vbt {

constexpr int MJD_THREADS = 256;
constexpr int MJD_SLICE = 16;                                     // bytes of the scan per thread and chunk of the marker kernel
constexpr int MJD_MAX_BATCH = 1024;
constexpr size_t MJD_MAX_PACKED = (size_t)1 << 30;                // descriptors + entropy-coded bytes of one batch: 1 GiB
constexpr int MJD_SUBSEQ = 1024;                                  // VBT_MJPEG_ENTROPY_SYNC: bytes per subsequence when the caller names none ...
constexpr int MJD_AUTO_MIN_INTERVAL = 13920;                      // ... and VBT_MJPEG_ENTROPY_AUTO: the mean interval length from which a frame takes that path (profiles/mjpeg_decode.md)

struct MjdArgs {
  const uint8_t* packed;     // [B] JpegDesc, then the frames' scans, each 16-byte aligned (scan_off counts from packed)
  int B, H, W;
  uint32_t* rst;             // [B][rst_cap]: byte offset of every RSTm inside its frame's scan, in order
  uint32_t rst_cap;
  uint32_t* rst_count;       // [B]
  int32_t* status;           // [B]
  int16_t* levels;           // [B][frame_blocks][64]
  uint8_t* planes;           // [B][frame_blocks][64]
  uint32_t frame_blocks;     // the batch's largest jpeg_layout().blocks
  uint8_t* out;              // [B][H][W][3]
};

__device__ __forceinline__ const JpegDesc& mjd_desc(const MjdArgs& A, int f) { return ((const JpegDesc*)A.packed)[f]; }

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

__global__ __launch_bounds__(MJD_THREADS) void mjpegd_markers_kernel(MjdArgs A) {
  __shared__ int wsum[MJD_THREADS / 64];
  const int tid = threadIdx.x, f = blockIdx.x;
  const JpegDesc& d = mjd_desc(A, f);
  const uint8_t* scan = A.packed + d.scan_off;
  const uint32_t len = d.scan_len, want = (uint32_t)d.n_int - 1;    // want < rst_cap: n_int <= MCUs <= ceil(W / 8) ceil(H / 8)
  uint32_t* pos = A.rst + (size_t)f * A.rst_cap;
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
        if (k < want && k < A.rst_cap) {
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

__global__ __launch_bounds__(64) void mjpegd_entropy_kernel(MjdArgs A) {
  const int f = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
  const JpegDesc& d = mjd_desc(A, f);
  if (k >= d.n_int || A.rst_count[f] != (uint32_t)d.n_int - 1) return;   // (a frame whose marker count is off is not walked at all)
  const uint32_t* pos = A.rst + (size_t)f * A.rst_cap;
  const uint32_t start = k ? pos[k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[k] : d.scan_len;
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > A.frame_blocks) return;
  const int st = jpeg_decode_interval(d, L, A.packed + d.scan_off, start, end, k, A.levels + (size_t)f * A.frame_blocks * 64);
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
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > A.frame_blocks) return;
  {
    const uint32_t* src = (const uint32_t*)d.dc;
    uint32_t* dst = (uint32_t*)sHuff;
    for (int i = tid; i < (int)(4 * sizeof(JpegHuff) / 4); i += MJD_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t* pos = A.rst + (size_t)f * A.rst_cap;
  const uint32_t start = k ? pos[k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[k] : d.scan_len;
  const uint8_t* scan = A.packed + d.scan_off;
  int16_t* levels = A.levels + (size_t)f * A.frame_blocks * 64;
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

__global__ __launch_bounds__(MJD_THREADS) void mjpegd_idct_kernel(MjdArgs A) {
  __shared__ uint16_t sQ[4][64];
  const int tid = threadIdx.x, f = blockIdx.y;
  const JpegDesc& d = mjd_desc(A, f);
  sQ[tid >> 6][tid & 63] = d.q[tid >> 6][tid & 63];
  __syncthreads();
  const JpegLayout L = jpeg_layout(d);
  const uint32_t bi = blockIdx.x * MJD_THREADS + tid;
  if (bi >= L.blocks || L.blocks > A.frame_blocks) return;
  const int c = d.ncomp == 3 ? (bi >= L.boff[2] ? 2 : bi >= L.boff[1] ? 1 : 0) : 0;
  const uint32_t local = bi - L.boff[c], by = local / (uint32_t)L.bw[c], bx = local % (uint32_t)L.bw[c];
  const uint4* lv = (const uint4*)(A.levels + ((size_t)f * A.frame_blocks + bi) * 64);
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
  uint8_t* dst = A.planes + ((size_t)f * A.frame_blocks + L.boff[c]) * 64 + (size_t)by * 8 * pw + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    uint2 o;
    o.x = px[r * 8] | (px[r * 8 + 1] << 8) | (px[r * 8 + 2] << 16) | ((uint32_t)px[r * 8 + 3] << 24);
    o.y = px[r * 8 + 4] | (px[r * 8 + 5] << 8) | (px[r * 8 + 6] << 16) | ((uint32_t)px[r * 8 + 7] << 24);
    *(uint2*)(dst + r * pw) = o;
  }
}

__global__ __launch_bounds__(MJD_THREADS) void mjpegd_colour_kernel(MjdArgs A) {
  const int f = blockIdx.y;
  const JpegDesc& d = mjd_desc(A, f);
  const JpegLayout L = jpeg_layout(d);
  if (L.blocks > A.frame_blocks) return;
  const size_t npix = (size_t)A.H * A.W, p0 = ((size_t)blockIdx.x * MJD_THREADS + threadIdx.x) * 4;
  if (p0 >= npix) return;
  const uint8_t* planes = A.planes + (size_t)f * A.frame_blocks * 64;
  uint8_t* dst = A.out + (size_t)f * npix * 3 + p0 * 3;
  const int n = npix - p0 < 4 ? (int)(npix - p0) : 4;
  uint8_t rgb[12];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const size_t p = p0 + i < npix ? p0 + i : npix - 1;
    jpeg_pixel(d, L, planes, (int)(p / (size_t)A.W), (int)(p % (size_t)A.W), rgb + 3 * i);
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

}  // namespace vbt

using namespace vbt;

struct vbt_mjpeg_decoder {
  int device = 0, H = 0, W = 0, max_batch = 0;
  size_t frame_blocks = 0, rst_cap = 0;
  uint8_t* blob = nullptr;               // status | rst_count | rst | levels | planes in one allocation
  uint8_t* packed = nullptr;             // the batch's descriptors and scans on the device; grows on demand up to MJD_MAX_PACKED
  size_t packed_cap = 0;
  uint8_t* stage[2] = {nullptr, nullptr};   // pinned staging, used in turn
  size_t stage_cap[2] = {0, 0};
  hipEvent_t copied[2] = {nullptr, nullptr};   // recorded behind the H2D copy out of stage[i]: the host waits for it before it refills stage[i]
  bool in_flight[2] = {false, false};
  int next = 0, last_B = 0;
  hipEvent_t stamp[7] = {};              // VBT_MJPEG_DECODE_STAMPS=1: around each stage of a decode (vbt_mjpeg_decode_stage_ms)
  bool stamps = false;
  int entropy = VBT_MJPEG_ENTROPY_AUTO, subseq = 0;   // vbt_mjpeg_decoder_set_entropy
  int last_path = 0, last_subseq = 0;    // of the last batch
  int32_t* info = nullptr;               // in blob: { most rounds of any chunk, intervals the single lane finished } of the last batch in SYNC
  std::vector<JpegDesc> descs;
  MjdArgs args{};
};

namespace {

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

int sampling_code(const JpegDesc& d) { return (d.hs << 4) | d.vs; }

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

int vbt_mjpeg_decoder_create(int device, int H, int W, int max_batch, vbt_mjpeg_decoder** out) {
  if (!out) { set_error("vbt_mjpeg_decoder_create: out is NULL"); return VBT_ERR_ARG; }
  *out = nullptr;
  if (H < 1 || W < 1 || H > JPEG_MAX_SIDE || W > JPEG_MAX_SIDE) { set_error("vbt_mjpeg_decoder_create: frames of 1..16384 pixels a side, got %d x %d", H, W); return VBT_ERR_ARG; }
  if (max_batch < 1 || max_batch > MJD_MAX_BATCH) { set_error("vbt_mjpeg_decoder_create: max_batch %d outside 1..%d", max_batch, MJD_MAX_BATCH); return VBT_ERR_ARG; }
  if (int rc = use_device("vbt_mjpeg_decoder_create", device)) return rc;
  vbt_mjpeg_decoder* m = new vbt_mjpeg_decoder();
  m->device = device; m->H = H; m->W = W; m->max_batch = max_batch;
  m->frame_blocks = (size_t)jpeg_max_blocks(H, W);
  m->rst_cap = (size_t)((W + 7) / 8) * (size_t)((H + 7) / 8);
  const size_t B = (size_t)max_batch;
  const size_t o_status = 0, o_count = align256(B * 4), o_rst = o_count + align256(B * 4), o_levels = o_rst + align256(B * m->rst_cap * 4),
               o_planes = o_levels + align256(B * m->frame_blocks * 128), o_info = o_planes + align256(B * m->frame_blocks * 64), total = o_info + 256;
  m->packed_cap = std::min(MJD_MAX_PACKED, align256(B * sizeof(JpegDesc) + B * (4096 + (size_t)H * W / 4)));
  hipError_t e = hipMalloc((void**)&m->blob, total);
  if (e == hipSuccess) e = hipMalloc((void**)&m->packed, m->packed_cap);
  for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&m->copied[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    set_error("vbt_mjpeg_decoder_create: %zu bytes of device memory for %d frames of %d x %d: %s", total + m->packed_cap, max_batch, W, H, hipGetErrorString(e));
    vbt_mjpeg_decoder_destroy(m);
    return VBT_ERR_HIP;
  }
  const char* env = getenv("VBT_MJPEG_DECODE_STAMPS");
  if (env && env[0] == '1') {
    for (int i = 0; i < 7; i++) {
      if (hipEventCreate(&m->stamp[i]) != hipSuccess) {
        set_error("vbt_mjpeg_decoder_create: cannot create the stage events");
        vbt_mjpeg_decoder_destroy(m);
        return VBT_ERR_HIP;
      }
    }
    m->stamps = true;
  }
  MjdArgs& A = m->args;
  A.H = H; A.W = W;
  A.status = (int32_t*)(m->blob + o_status); A.rst_count = (uint32_t*)(m->blob + o_count); A.rst = (uint32_t*)(m->blob + o_rst);
  A.rst_cap = (uint32_t)m->rst_cap; A.levels = (int16_t*)(m->blob + o_levels); A.planes = m->blob + o_planes;
  m->info = (int32_t*)(m->blob + o_info);
  *out = m;
  return VBT_OK;
}

void vbt_mjpeg_decoder_destroy(vbt_mjpeg_decoder* m) {
  if (!m) return;
  if (hipSetDevice(m->device) == hipSuccess) {
    if (m->blob) (void)hipFree(m->blob);                          // (waits for the kernels still using it)
    if (m->packed) (void)hipFree(m->packed);
    for (int i = 0; i < 2; i++) {
      if (m->stage[i]) (void)hipHostFree(m->stage[i]);
      if (m->copied[i]) (void)hipEventDestroy(m->copied[i]);
    }
    for (int i = 0; i < 7; i++)
      if (m->stamp[i]) (void)hipEventDestroy(m->stamp[i]);
  }
  delete m;
}

int vbt_mjpeg_decode(vbt_mjpeg_decoder* m, const uint8_t* host_bytes, const uint64_t* offsets, int B, uint8_t* frames_dev_out, void* stream) {
  if (!m || !host_bytes || !offsets || !frames_dev_out || B < 1) { set_error("vbt_mjpeg_decode: bad argument (handle, bytes, offsets, frames, B >= 1)"); return VBT_ERR_ARG; }
  if (B > m->max_batch) { set_error("vbt_mjpeg_decode: %d frames, the handle was created for %d", B, m->max_batch); return VBT_ERR_CAPACITY; }
  for (int i = 0; i < B; i++)
    if (offsets[i + 1] < offsets[i]) { set_error("vbt_mjpeg_decode: offsets[%d] > offsets[%d]", i, i + 1); return VBT_ERR_ARG; }
  // ---- every header first: a refusal leaves nothing enqueued
  m->descs.resize((size_t)B);
  size_t total = align16((size_t)B * sizeof(JpegDesc));
  uint32_t max_int = 1, max_blocks = 1;
  bool sync = m->entropy == VBT_MJPEG_ENTROPY_SYNC;
  for (int i = 0; i < B; i++) {
    JpegDesc& d = m->descs[(size_t)i];
    std::string why;
    if (!jpeg_parse(host_bytes + offsets[i], offsets[i + 1] - offsets[i], m->H, m->W, &d, &why)) {
      set_error("vbt_mjpeg_decode: frame %d of the batch: %s", i, why.c_str());
      return VBT_ERR_IO;
    }
    max_int = std::max(max_int, (uint32_t)d.n_int);
    if (m->entropy == VBT_MJPEG_ENTROPY_AUTO && d.scan_len / (uint32_t)d.n_int >= (uint32_t)MJD_AUTO_MIN_INTERVAL) sync = true;
    max_blocks = std::max(max_blocks, jpeg_layout(d).blocks);
    total += align16(d.scan_len);
  }
  if (total > MJD_MAX_PACKED || max_blocks > m->frame_blocks) {
    set_error("vbt_mjpeg_decode: %zu compressed bytes in one batch, the bound is %zu: decode fewer frames at a time", total, MJD_MAX_PACKED);
    return VBT_ERR_CAPACITY;
  }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  hipStream_t st = (hipStream_t)stream;
  const int s = m->next;
  if (m->in_flight[s]) {                                          // host-side gate: the copy that last read this staging buffer is done
    VBT_HIP_CHECK(hipEventSynchronize(m->copied[s]));
    m->in_flight[s] = false;
  }
  if (total > m->stage_cap[s]) {
    if (m->stage[s]) (void)hipHostFree(m->stage[s]);
    m->stage[s] = nullptr;
    m->stage_cap[s] = 0;
    const size_t cap = std::min(MJD_MAX_PACKED, align256(total + total / 4));
    VBT_HIP_CHECK(hipHostMalloc((void**)&m->stage[s], cap, hipHostMallocDefault));
    m->stage_cap[s] = cap;
  }
  if (total > m->packed_cap) {                                    // growth frees the old buffer, which waits for the work that reads it
    const size_t cap = std::min(MJD_MAX_PACKED, align256(total + total / 4));
    (void)hipFree(m->packed);
    m->packed = nullptr;
    m->packed_cap = 0;
    hipError_t e = hipMalloc((void**)&m->packed, cap);
    if (e != hipSuccess) { set_error("vbt_mjpeg_decode: %zu bytes of device memory for the compressed frames: %s", cap, hipGetErrorString(e)); return VBT_ERR_HIP; }
    m->packed_cap = cap;
  }
  uint8_t* pk = m->stage[s];
  size_t at = align16((size_t)B * sizeof(JpegDesc));
  for (int i = 0; i < B; i++) {
    JpegDesc& d = m->descs[(size_t)i];
    memcpy(pk + at, host_bytes + offsets[i] + d.scan_off, d.scan_len);
    d.scan_off = at;
    at += align16(d.scan_len);
  }
  memcpy(pk, m->descs.data(), (size_t)B * sizeof(JpegDesc));
  auto stamp = [&](int i) { return m->stamps ? hipEventRecord(m->stamp[i], st) : hipSuccess; };
  VBT_HIP_CHECK(stamp(0));
  VBT_HIP_CHECK(hipMemcpyAsync(m->packed, pk, total, hipMemcpyHostToDevice, st));
  VBT_HIP_CHECK(hipEventRecord(m->copied[s], st));
  VBT_HIP_CHECK(stamp(1));
  m->in_flight[s] = true;
  m->next = s ^ 1;
  MjdArgs A = m->args;
  A.packed = m->packed; A.B = B; A.frame_blocks = max_blocks; A.out = frames_dev_out;
  VBT_HIP_CHECK(hipMemsetAsync(A.status, 0, (size_t)B * 4, st));
  VBT_HIP_CHECK(hipMemsetAsync(A.levels, 0, (size_t)B * max_blocks * 128, st));
  if (sync) VBT_HIP_CHECK(hipMemsetAsync(m->info, 0, 8, st));
  VBT_HIP_CHECK(stamp(2));
  mjpegd_markers_kernel<<<dim3((unsigned)B), MJD_THREADS, 0, st>>>(A);
  VBT_HIP_CHECK(stamp(3));
  const int S = m->subseq ? m->subseq : MJD_SUBSEQ;
  if (sync) mjpegd_entropy_sync_kernel<<<dim3(max_int, (unsigned)B), MJD_THREADS, 0, st>>>(A, S, m->info);
  else mjpegd_entropy_kernel<<<dim3((max_int + 63) / 64, (unsigned)B), 64, 0, st>>>(A);
  VBT_HIP_CHECK(stamp(4));
  mjpegd_idct_kernel<<<dim3((max_blocks + MJD_THREADS - 1) / MJD_THREADS, (unsigned)B), MJD_THREADS, 0, st>>>(A);
  VBT_HIP_CHECK(stamp(5));
  const size_t groups = ((size_t)m->H * m->W + MJD_THREADS * 4 - 1) / (MJD_THREADS * 4);
  mjpegd_colour_kernel<<<dim3((unsigned)groups, (unsigned)B), MJD_THREADS, 0, st>>>(A);
  VBT_HIP_CHECK(stamp(6));
  VBT_HIP_CHECK(hipGetLastError());
  m->last_B = B;
  m->last_path = sync ? VBT_MJPEG_ENTROPY_SYNC : VBT_MJPEG_ENTROPY_INTERVAL;
  m->last_subseq = sync ? S : 0;
  return VBT_OK;
}

int vbt_mjpeg_decoder_set_entropy(vbt_mjpeg_decoder* m, int mode, int subseq_bytes) {
  if (!m) { set_error("vbt_mjpeg_decoder_set_entropy: handle is NULL"); return VBT_ERR_ARG; }
  if (mode < VBT_MJPEG_ENTROPY_AUTO || mode > VBT_MJPEG_ENTROPY_SYNC) { set_error("vbt_mjpeg_decoder_set_entropy: mode %d is none of AUTO (0), INTERVAL (1), SYNC (2)", mode); return VBT_ERR_ARG; }
  if (subseq_bytes && (subseq_bytes < 4 || subseq_bytes > 4096 || (subseq_bytes & (subseq_bytes - 1)))) {
    set_error("vbt_mjpeg_decoder_set_entropy: subseq_bytes %d is neither 0 nor a power of two in 4..4096", subseq_bytes);
    return VBT_ERR_ARG;
  }
  m->entropy = mode;
  m->subseq = subseq_bytes;
  return VBT_OK;
}

int vbt_mjpeg_decoder_get_entropy(vbt_mjpeg_decoder* m, int* mode, int* subseq_bytes, int* auto_min_interval_bytes) {
  if (!m) { set_error("vbt_mjpeg_decoder_get_entropy: handle is NULL"); return VBT_ERR_ARG; }
  if (mode) *mode = m->entropy;
  if (subseq_bytes) *subseq_bytes = m->subseq ? m->subseq : MJD_SUBSEQ;
  if (auto_min_interval_bytes) *auto_min_interval_bytes = MJD_AUTO_MIN_INTERVAL;
  return VBT_OK;
}

int vbt_mjpeg_decode_status(vbt_mjpeg_decoder* m, int32_t* status, void* stream) {
  if (!m || !status) { set_error("vbt_mjpeg_decode_status: bad argument"); return VBT_ERR_ARG; }
  if (!m->last_B) { set_error("vbt_mjpeg_decode_status: no batch has been decoded (vbt_mjpeg_decode first)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  VBT_HIP_CHECK(hipMemcpy(status, m->args.status, (size_t)m->last_B * 4, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt_mjpeg_decode_entropy_info(vbt_mjpeg_decoder* m, int32_t* info4, void* stream) {
  if (!m || !info4) { set_error("vbt_mjpeg_decode_entropy_info: bad argument"); return VBT_ERR_ARG; }
  if (!m->last_B) { set_error("vbt_mjpeg_decode_entropy_info: no batch has been decoded (vbt_mjpeg_decode first)"); return VBT_ERR_STATE; }
  info4[0] = m->last_path; info4[1] = m->last_subseq; info4[2] = info4[3] = 0;
  VBT_HIP_CHECK(hipSetDevice(m->device));
  VBT_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  if (m->last_path == VBT_MJPEG_ENTROPY_SYNC) VBT_HIP_CHECK(hipMemcpy(info4 + 2, m->info, 8, hipMemcpyDeviceToHost));
  return VBT_OK;
}

int vbt_mjpeg_decode_stage_ms(vbt_mjpeg_decoder* m, float* ms6) {
  if (!m || !ms6) { set_error("vbt_mjpeg_decode_stage_ms: bad argument"); return VBT_ERR_ARG; }
  if (!m->stamps || !m->last_B) { set_error("vbt_mjpeg_decode_stage_ms: needs VBT_MJPEG_DECODE_STAMPS=1 at create and a decoded batch"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(m->device));
  VBT_HIP_CHECK(hipEventSynchronize(m->stamp[6]));
  for (int i = 0; i < 6; i++) VBT_HIP_CHECK(hipEventElapsedTime(&ms6[i], m->stamp[i], m->stamp[i + 1]));
  return VBT_OK;
}

}  // extern "C"
