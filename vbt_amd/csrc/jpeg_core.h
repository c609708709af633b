// MJPEG import (include/vbt_hip.h, "MJPEG import"): the decoding core as host + device functions, so that the kernels of
// mjpeg_decode.hip and a host loop (tests/fuzz/jpeg_fuzz.cc, built with g++ -fsanitize=address,undefined) run the same statements.
// Plain C++: no HIP header is needed to compile it for the host.
//   JpegBits             the bounded bit reader over one restart interval, FF 00 de-stuffed
//   jpeg_symbol          one Huffman symbol: an 8-bit look-up table, then canonical maxcode / valoff for lengths 9..16
//   jpeg_decode_block    one block: DC difference + AC run / size pairs into 64 int16 levels, natural order
//   jpeg_decode_interval the MCUs of one restart interval
//   jpeg_sync_walk       one subsequence of an interval from a (possibly guessed) state: the lane's work in the decode by subsequences
//                        that synchronise; jpeg_sync_cold: the guess; jpeg_decode_rest: one lane finishes an interval from a true state
//   jpeg_idct_islow      dequantised coefficients -> 64 samples (the "islow" integer IDCT)
//   jpeg_chroma_at       one chroma sample at full resolution ("fancy" triangle upsampling); jpeg_ycc_rgb: the colour tables
//   jpeg_resized_pixel   one pixel of the network input: the four taps of the bilinear resize taken through jpeg_pixel
// Every loop is bounded by a count known before it starts (MCUs of the interval, 64 coefficients, 16 code lengths, 7 bytes of a
// refill, the 8 S + 32 symbols of a subsequence of S bytes); none is bounded by the data.  A read past the interval's end, a code no
// table holds and a coefficient index above 63 each return a status and end the interval.  Nothing is read outside [start, end) of
// the scan or written outside the frame's levels.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBT_HD __host__ __device__
#else
#define VBT_HD
#endif

namespace vbt {

// per-frame scan status (vbt_mjpeg_decode_status); the largest code raised in a frame is the one reported
enum { JPEG_ST_OK = 0, JPEG_ST_OVERRUN = 1, JPEG_ST_BAD_CODE = 2, JPEG_ST_BAD_INDEX = 3, JPEG_ST_RST_COUNT = 4, JPEG_ST_RST_ORDER = 5 };

struct JpegHuff {
  uint16_t look[256];    // by the next 8 bits: (length << 8) | symbol for codes of 1..8 bits, 0 otherwise
  int32_t maxcode[17];   // by length 1..16: the largest code of that length, -1 when there is none
  int32_t valoff[17];    // by length: index of the length's first symbol minus its first code
  uint8_t vals[256];
};

// what the host parser (jpeg_parse.h) makes of one frame's headers; travels to the device in front of the compressed bytes
struct JpegDesc {
  uint64_t scan_off;     // the entropy-coded segment: offset (the parser: in the frame; on the device: in the packed buffer) ...
  uint32_t scan_len;     // ... and length, up to the marker that ends it
  int32_t H, W, ncomp;   // 1 (grey) or 3 (YCbCr)
  int32_t hs, vs;        // luma sampling: 1x1, 2x1 or 2x2; chroma is 1x1
  int32_t ri;            // MCUs per restart interval (a frame without DRI: all of them)
  int32_t n_int;         // restart intervals = ceil(mcus / ri)
  int32_t mcus, MW, MH;
  uint8_t tq[4], td[4], ta[4];   // per component: quantisation, DC and AC table
  uint16_t q[4][64];     // natural order
  JpegHuff dc[2], ac[2];
};

// where a frame's blocks and samples live: component c is bh[c] x bw[c] blocks (whole MCUs), blocks row-major from boff[c];
// a block is 64 int16 levels (128 B) in the levels scratch and 8 x 8 samples of a plane 8 bw[c] wide in the planes scratch
struct JpegLayout {
  int32_t bw[3], bh[3];
  uint32_t boff[3], blocks;
};

VBT_HD inline JpegLayout jpeg_layout(const JpegDesc& d) {
  JpegLayout L;
  uint32_t at = 0;
  for (int c = 0; c < 3; c++) {
    const bool on = c < d.ncomp;
    L.bw[c] = on ? d.MW * (c == 0 ? d.hs : 1) : 0;
    L.bh[c] = on ? d.MH * (c == 0 ? d.vs : 1) : 0;
    L.boff[c] = at;
    at += (uint32_t)L.bw[c] * (uint32_t)L.bh[c];
  }
  L.blocks = at;
  return L;
}

// an upper bound of jpeg_layout().blocks over every accepted sampling of an H x W frame
inline uint64_t jpeg_max_blocks(int H, int W) { return 3ull * (uint64_t)(2 * ((W + 15) / 16)) * (uint64_t)(2 * ((H + 15) / 16)); }

VBT_HD inline int jpeg_zigzag(int k) {    // natural index of zigzag position k, k in 0..63
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// RSTm at byte i of a scan of len bytes?  (FF 00 and FF FF never look like one: the test needs no context)
VBT_HD inline bool jpeg_is_rst(const uint8_t* scan, uint32_t len, uint32_t i) {
  return i + 1 < len && scan[i] == 0xFF && (scan[i + 1] & 0xF8) == 0xD0;
}

// ---- the bit reader: bits of p[pos .. end), most significant first, in the top n bits of acc; the bits below are 0
struct JpegBits {
  const uint8_t* p;
  uint32_t pos, end;
  uint64_t acc;
  int n;
};

VBT_HD inline void jpeg_bits_init(JpegBits& b, const uint8_t* p, uint32_t start, uint32_t end) {
  b.p = p; b.pos = start; b.end = end; b.acc = 0; b.n = 0;
}

// at least 57 bits, or all that are left
VBT_HD inline void jpeg_bits_fill(JpegBits& b) {
  for (int i = 0; i < 8; i++) {
    if (b.n > 56 || b.pos >= b.end) break;
    const uint32_t v = b.p[b.pos++];
    if (v == 0xFF) {
      if (b.pos < b.end && b.p[b.pos] == 0) b.pos++;                 // FF 00: a stuffed 0xFF
      else { b.pos = b.end; break; }                                 // a marker, a fill byte or a lone FF: the data ends here
    }
    b.acc |= (uint64_t)v << (56 - b.n);
    b.n += 8;
  }
}

VBT_HD inline uint32_t jpeg_bits_peek(const JpegBits& b, int k) { return (uint32_t)(b.acc >> (64 - k)); }   // 1 <= k <= 32

VBT_HD inline bool jpeg_bits_skip(JpegBits& b, int k) {              // 1 <= k <= 32; false: the bits were not there
  if (k > b.n) { b.acc = 0; b.n = 0; return false; }
  b.acc <<= k;
  b.n -= k;
  return true;
}

// one symbol (call jpeg_bits_fill first); -1 with *st set otherwise
VBT_HD inline int jpeg_symbol(JpegBits& b, const JpegHuff& h, int* st) {
  const uint32_t top = jpeg_bits_peek(b, 16);
  const uint32_t e = h.look[top >> 8];
  int len = (int)(e >> 8), sym = (int)(e & 255);
  if (len == 0) {
    for (int l = 9; l <= 16; l++) {
      const int32_t c = (int32_t)(top >> (16 - l));
      if (c <= h.maxcode[l]) {
        len = l;
        sym = h.vals[(uint32_t)(h.valoff[l] + c) & 255];
        break;
      }
    }
    if (len == 0) { *st = b.n < 16 ? JPEG_ST_OVERRUN : JPEG_ST_BAD_CODE; return -1; }   // (fewer than 16 bits left: the data ended first)
  }
  if (!jpeg_bits_skip(b, len)) { *st = JPEG_ST_OVERRUN; return -1; }
  return sym;
}

VBT_HD inline int jpeg_extend(uint32_t r, int s) { return r < (1u << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r; }   // 1 <= s <= 16

// the AC coefficients of one block from zigzag index k (1..63) on, into out[64]
VBT_HD inline int jpeg_decode_ac(JpegBits& b, const JpegHuff& ac, int k, int16_t* out) {
  int st = JPEG_ST_OK;
  for (int i = 1; i < 64 && k < 64; i++) {
    jpeg_bits_fill(b);
    const int rs = jpeg_symbol(b, ac, &st);
    if (rs < 0) return st;
    const int r = rs >> 4, s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return JPEG_ST_BAD_INDEX;
      const uint32_t v = jpeg_bits_peek(b, s);
      if (!jpeg_bits_skip(b, s)) return JPEG_ST_OVERRUN;
      out[jpeg_zigzag(k)] = (int16_t)jpeg_extend(v, s);
      k++;
    } else if (r == 15) {
      k += 16;
    } else {
      break;                                                         // EOB
    }
  }
  return JPEG_ST_OK;
}

// one block into out[64] (natural order; the caller zeroed it); *pred: the component's DC predictor
VBT_HD inline int jpeg_decode_block(JpegBits& b, const JpegHuff& dc, const JpegHuff& ac, int* pred, int16_t* out) {
  int st = JPEG_ST_OK;
  jpeg_bits_fill(b);
  int s = jpeg_symbol(b, dc, &st);
  if (s < 0) return st;
  if (s > 16) return JPEG_ST_BAD_CODE;
  if (s) {
    const uint32_t r = jpeg_bits_peek(b, s);
    if (!jpeg_bits_skip(b, s)) return JPEG_ST_OVERRUN;
    *pred = (int)((uint32_t)*pred + (uint32_t)jpeg_extend(r, s));
  }
  out[0] = (int16_t)*pred;
  return jpeg_decode_ac(b, ac, 1, out);
}

// restart interval k of a frame: scan[start .. end) -> the levels of its MCUs (levels: the frame's, jpeg_layout().blocks x 64, zeroed)
VBT_HD inline int jpeg_decode_interval(const JpegDesc& d, const JpegLayout& L, const uint8_t* scan, uint32_t start, uint32_t end, int k, int16_t* levels) {
  JpegBits b;
  jpeg_bits_init(b, scan, start, end);
  int pred[3] = {0, 0, 0};
  const int m0 = k * d.ri, nm = d.mcus - m0 < d.ri ? d.mcus - m0 : d.ri;
  for (int i = 0; i < nm; i++) {
    const int my = (m0 + i) / d.MW, mx = (m0 + i) % d.MW;
    for (int c = 0; c < d.ncomp; c++) {
      const int h = c == 0 ? d.hs : 1, v = c == 0 ? d.vs : 1;
      const JpegHuff& dc = d.dc[d.td[c] & 1];
      const JpegHuff& ac = d.ac[d.ta[c] & 1];
      for (int j = 0; j < h * v; j++) {
        const uint32_t blk = L.boff[c] + (uint32_t)(my * v + j / h) * (uint32_t)L.bw[c] + (uint32_t)(mx * h + j % h);
        const int st = jpeg_decode_block(b, dc, ac, &pred[c], levels + (size_t)blk * 64);
        if (st) return st;
      }
    }
  }
  return JPEG_ST_OK;
}

// ---- subsequences that synchronise (include/vbt_hip.h, "Entropy decoding"): an interval scan[start, end) is cut into subsequences
// of S raw bytes; lane i owns the symbols that BEGIN in bytes [start + i S, start + (i + 1) S).  The decoder's state at a symbol
// boundary is (p, u, k): p the raw byte and bit of the next unread bit (a stuffed FF 00 is named by its FF), u the block slot inside
// the MCU (0 .. hs vs + 1; 0 for grey), k the zigzag index (0: a DC size comes next).  A lane that does not know its state guesses
// (jpeg_sync_cold), walks, and takes its left neighbour's exit as its next entry until no entry changes: a walk is a pure function
// of its entry and the bytes, so lanes 0 .. r - 1 are final after round r.  A walk from a guess meets bad codes all the time; it
// records where the first one was and goes on by a fixed rule.  A chunk in which a lane with a true entry recorded one before the
// interval's last block is finished by one lane with the statements of jpeg_decode_block (jpeg_decode_rest).
struct JpegSyncState {
  uint32_t pos;          // raw byte that holds the next unread bit (end: no bit is left)
  uint32_t buk;          // bit inside it, from the top (0..7) | u << 3 | k << 8
};
VBT_HD inline bool jpeg_sync_same(const JpegSyncState& a, const JpegSyncState& b) { return a.pos == b.pos && a.buk == b.buk; }

constexpr uint32_t JPEG_SYNC_NONE = 0xFFFFFFFFu;

struct JpegSyncWalk {
  JpegSyncState exit;
  uint32_t blocks;       // blocks completed
  uint32_t dc[3];        // per component: the wrapping sum of the DC differences read
  uint32_t bad_at;       // blocks completed when the first status was recorded; JPEG_SYNC_NONE: none was
};

VBT_HD inline int jpeg_blocks_per_mcu(const JpegDesc& d) { return d.ncomp == 1 ? 1 : d.hs * d.vs + 2; }
// blocks of restart interval k
VBT_HD inline uint32_t jpeg_interval_blocks(const JpegDesc& d, int k) {
  const int m0 = k * d.ri, nm = d.mcus - m0 < d.ri ? d.mcus - m0 : d.ri;
  return (uint32_t)nm * (uint32_t)jpeg_blocks_per_mcu(d);
}
VBT_HD inline int jpeg_slot_component(const JpegDesc& d, int u) { const int hv = d.hs * d.vs; return u < hv ? 0 : u - hv + 1; }
// the block of slot u of MCU (my, mx), by the arithmetic of jpeg_decode_interval
VBT_HD inline uint32_t jpeg_slot_block(const JpegDesc& d, const JpegLayout& L, int my, int mx, int u) {
  const int c = jpeg_slot_component(d, u), h = c == 0 ? d.hs : 1, v = c == 0 ? d.vs : 1, j = c == 0 ? u : 0;
  return L.boff[c] + (uint32_t)(my * v + j / h) * (uint32_t)L.bw[c] + (uint32_t)(mx * h + j % h);
}

// the guess of a lane whose first byte is scan[pos], pos > start: a block begins there - behind the 00 if the byte is a stuffed one
VBT_HD inline JpegSyncState jpeg_sync_cold(const uint8_t* scan, uint32_t pos) {
  JpegSyncState s;
  s.pos = scan[pos] == 0 && scan[pos - 1] == 0xFF ? pos + 1 : pos;
  s.buk = 0;
  return s;
}

// jpeg_bits_fill, but only bytes that begin before lim (lim <= b.end); returns the bits it added.  jpeg_bits_fill_to, then
// jpeg_bits_fill, leaves in b what jpeg_bits_fill alone leaves
VBT_HD inline int jpeg_bits_fill_to(JpegBits& b, uint32_t lim) {
  int added = 0;
  for (int i = 0; i < 8; i++) {
    if (b.n > 56 || b.pos >= lim) break;
    const uint32_t v = b.p[b.pos++];
    if (v == 0xFF) {
      if (b.pos < b.end && b.p[b.pos] == 0) b.pos++;
      else { b.pos = b.end; break; }
    }
    b.acc |= (uint64_t)v << (56 - b.n);
    b.n += 8;
    added += 8;
  }
  return added;
}

// The symbols that begin before raw byte `limit` (<= end), from state `in`, at most max_syms of them (8 S + 32 covers a subsequence
// of S bytes: every symbol takes a bit).  huff: the frame's dc[0], dc[1], ac[0], ac[1].  Bits are read up to `end` under the rules
// of JpegBits and with its statements, so a walk from a true state sees what jpeg_decode_block sees.  A status is recorded, not
// raised: an unmatched code consumes up to 16 bits and the walk goes on, an index above 63 ends the block, a DC size above 16 counts
// as 0; when the bits run out the walk ends at `end`.
// WRITE: the levels are stored as jpeg_decode_block stores them.  n0: the interval's blocks completed before `in` (the block `in`
// lies in); pred: the predictors there; the walk stops behind block nblocks - 1 of the interval, whose first MCU is m0, and at a status.
template <bool WRITE>
VBT_HD inline JpegSyncWalk jpeg_sync_walk(const JpegDesc& d, const JpegLayout& L, const JpegHuff* huff, const uint8_t* scan, uint32_t end, JpegSyncState in,
                                          uint32_t limit, int max_syms, int m0, uint32_t n0, uint32_t nblocks, const uint32_t* pred, int16_t* levels) {
  JpegSyncWalk w;
  w.exit = in; w.blocks = 0; w.dc[0] = w.dc[1] = w.dc[2] = 0; w.bad_at = JPEG_SYNC_NONE;
  if (in.pos >= limit) return w;
  if (WRITE && n0 >= nblocks) return w;
  const int bpm = jpeg_blocks_per_mcu(d);
  int u = (int)(in.buk >> 3) & 31, k = (int)(in.buk >> 8) & 63;
  if (u >= bpm) u = 0;
  uint32_t pr[3] = {0, 0, 0};
  int mx = 0, my = 0;
  int16_t* out = levels;
  if (WRITE) {
    u = (int)(n0 % (uint32_t)bpm);                                   // (what a true state holds; from n0, so that the MCU stays inside the interval whatever `in` is)
    pr[0] = pred[0]; pr[1] = pred[1]; pr[2] = pred[2];
    const int mcu = m0 + (int)(n0 / (uint32_t)bpm);
    my = mcu / d.MW; mx = mcu % d.MW;
    out = levels + (size_t)jpeg_slot_block(d, L, my, mx, u) * 64;
  }
  JpegBits b;
  jpeg_bits_init(b, scan, in.pos, end);
  int before = jpeg_bits_fill_to(b, limit);                          // bits of b.acc out of bytes that begin before limit
  bool past = b.pos >= limit;
  uint32_t lpos = b.pos;                                             // once past: the first raw byte that was not counted in `before`
  if (in.buk & 7) { jpeg_bits_skip(b, (int)(in.buk & 7)); before -= (int)(in.buk & 7); }
  for (int it = 0; it < max_syms; it++) {
    if (!past) {
      before += jpeg_bits_fill_to(b, limit);
      past = b.pos >= limit;
      lpos = b.pos;
    }
    if (before <= 0 || b.n == 0) break;
    jpeg_bits_fill(b);
    const int n_was = b.n, c = jpeg_slot_component(d, u);
    int st = JPEG_ST_OK;
    bool done = false;
    if (k == 0) {
      int s = jpeg_symbol(b, huff[d.td[c] & 1], &st);
      if (s < 0) {
        if (b.n) jpeg_bits_skip(b, b.n < 16 ? b.n : 16);
      } else {
        if (s > 16) { st = JPEG_ST_BAD_CODE; s = 0; }
        bool have = true;
        uint32_t diff = 0;
        if (s) {
          const uint32_t r = jpeg_bits_peek(b, s);
          if (jpeg_bits_skip(b, s)) diff = (uint32_t)jpeg_extend(r, s);
          else { st = JPEG_ST_OVERRUN; have = false; }
        }
        if (have) {
          w.dc[0] += c == 0 ? diff : 0; w.dc[1] += c == 1 ? diff : 0; w.dc[2] += c == 2 ? diff : 0;   // (no runtime index: registers)
          if (WRITE) {
            pr[0] += c == 0 ? diff : 0; pr[1] += c == 1 ? diff : 0; pr[2] += c == 2 ? diff : 0;
            out[0] = (int16_t)(int)(c == 0 ? pr[0] : c == 1 ? pr[1] : pr[2]);
          }
          k = 1;
        }
      }
    } else {
      const int rs = jpeg_symbol(b, huff[2 + (d.ta[c] & 1)], &st);
      if (rs < 0) {
        if (b.n) jpeg_bits_skip(b, b.n < 16 ? b.n : 16);
      } else {
        const int r = rs >> 4, s = rs & 15;
        if (s) {
          k += r;
          if (k > 63) { st = JPEG_ST_BAD_INDEX; done = true; }
          else {
            const uint32_t v = jpeg_bits_peek(b, s);
            if (!jpeg_bits_skip(b, s)) st = JPEG_ST_OVERRUN;
            else {
              if (WRITE) out[jpeg_zigzag(k)] = (int16_t)jpeg_extend(v, s);
              k++;
              done = k > 63;
            }
          }
        } else if (r == 15) {
          k += 16;
          done = k > 63;
        } else {
          done = true;                                               // EOB
        }
      }
    }
    before -= n_was - b.n;
    if (st && w.bad_at == JPEG_SYNC_NONE) w.bad_at = w.blocks;
    if (WRITE && st) break;
    if (done) {
      w.blocks++;
      k = 0;
      u = u + 1 == bpm ? 0 : u + 1;
      if (WRITE) {
        if (n0 + w.blocks >= nblocks) break;
        if (u == 0 && ++mx == d.MW) { mx = 0; my++; }
        out = levels + (size_t)jpeg_slot_block(d, L, my, mx, u) * 64;
      }
    }
  }
  // the raw position of the next unread bit
  uint32_t q = end;
  int over = 0;
  if (b.n == 0 && b.pos >= b.end) {
    // every bit of the interval is used up
  } else if (past && before <= 0) {
    q = lpos;
    over = -before;                                                  // bits used out of the bytes from lpos on: whole data bytes, all below end
    for (int i = 0; i < 8 && over >= 8; i++) {
      q += q < end && scan[q] == 0xFF ? 2 : 1;
      over -= 8;
    }
    if (q >= end) { q = end; over = 0; }
  } else {
    w.bad_at = 0;                                                    // (not reached: max_syms symbols without passing limit)
  }
  w.exit.pos = q;
  w.exit.buk = (uint32_t)(over & 7) | (uint32_t)u << 3 | (uint32_t)k << 8;
  return w;
}

// One lane finishes restart interval kint from the true state `in`: n0 blocks of the interval are complete, the predictors are
// pred[3].  The rest of the block `in` lies in, then whole blocks, with the statements and the status of jpeg_decode_interval.
VBT_HD inline int jpeg_decode_rest(const JpegDesc& d, const JpegLayout& L, const uint8_t* scan, uint32_t end, int kint, JpegSyncState in, uint32_t n0,
                                   const uint32_t* pred, int16_t* levels) {
  JpegBits b;
  jpeg_bits_init(b, scan, in.pos < end ? in.pos : end, end);
  if (in.buk & 7) {
    jpeg_bits_fill(b);
    if (!jpeg_bits_skip(b, (int)(in.buk & 7))) return JPEG_ST_OVERRUN;
  }
  int pr[3] = {(int)pred[0], (int)pred[1], (int)pred[2]};
  const int m0 = kint * d.ri, bpm = jpeg_blocks_per_mcu(d), k = (int)(in.buk >> 8) & 63;
  const uint32_t nblocks = jpeg_interval_blocks(d, kint);
  for (uint32_t n = n0; n < nblocks; n++) {
    const int mcu = m0 + (int)(n / (uint32_t)bpm), u = (int)(n % (uint32_t)bpm), c = jpeg_slot_component(d, u);
    int16_t* out = levels + (size_t)jpeg_slot_block(d, L, mcu / d.MW, mcu % d.MW, u) * 64;
    const JpegHuff& ac = d.ac[d.ta[c] & 1];
    const int st = n == n0 && k ? jpeg_decode_ac(b, ac, k, out) : jpeg_decode_block(b, d.dc[d.td[c] & 1], ac, &pr[c], out);
    if (st) return st;
  }
  return JPEG_ST_OK;
}

// ---- the islow IDCT: 13-bit constants, 2 extra bits kept between the passes.  int32 two's complement, wrapping (written with
// unsigned operations so that no input, however damaged, is undefined behaviour); >> of a negative number is arithmetic.
#define VBT_JM(a, c) ((int32_t)((uint32_t)(a) * (uint32_t)(c)))
#define VBT_JA(a, b) ((int32_t)((uint32_t)(a) + (uint32_t)(b)))
#define VBT_JS(a, b) ((int32_t)((uint32_t)(a) - (uint32_t)(b)))
template <int SHIFT>
VBT_HD inline void jpeg_idct8(const int32_t (&x)[8], int32_t (&y)[8]) {
  int32_t z1 = VBT_JM(VBT_JA(x[2], x[6]), 4433);
  const int32_t t2 = VBT_JS(z1, VBT_JM(x[6], 15137)), t3 = VBT_JA(z1, VBT_JM(x[2], 6270));
  const int32_t t0 = VBT_JM(VBT_JA(x[0], x[4]), 8192), t1 = VBT_JM(VBT_JS(x[0], x[4]), 8192);
  const int32_t t10 = VBT_JA(t0, t3), t13 = VBT_JS(t0, t3), t11 = VBT_JA(t1, t2), t12 = VBT_JS(t1, t2);
  int32_t a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
  z1 = VBT_JA(a0, a3);
  int32_t z2 = VBT_JA(a1, a2), z3 = VBT_JA(a0, a2), z4 = VBT_JA(a1, a3);
  const int32_t z5 = VBT_JM(VBT_JA(z3, z4), 9633);
  a0 = VBT_JM(a0, 2446); a1 = VBT_JM(a1, 16819); a2 = VBT_JM(a2, 25172); a3 = VBT_JM(a3, 12299);
  z1 = VBT_JM(z1, -7373); z2 = VBT_JM(z2, -20995);
  z3 = VBT_JA(VBT_JM(z3, -16069), z5); z4 = VBT_JA(VBT_JM(z4, -3196), z5);
  a0 = VBT_JA(a0, VBT_JA(z1, z3)); a1 = VBT_JA(a1, VBT_JA(z2, z4)); a2 = VBT_JA(a2, VBT_JA(z2, z3)); a3 = VBT_JA(a3, VBT_JA(z1, z4));
  constexpr int32_t r = 1 << (SHIFT - 1);
  y[0] = VBT_JA(VBT_JA(t10, a3), r) >> SHIFT; y[7] = VBT_JA(VBT_JS(t10, a3), r) >> SHIFT;
  y[1] = VBT_JA(VBT_JA(t11, a2), r) >> SHIFT; y[6] = VBT_JA(VBT_JS(t11, a2), r) >> SHIFT;
  y[2] = VBT_JA(VBT_JA(t12, a1), r) >> SHIFT; y[5] = VBT_JA(VBT_JS(t12, a1), r) >> SHIFT;
  y[3] = VBT_JA(VBT_JA(t13, a0), r) >> SHIFT; y[4] = VBT_JA(VBT_JS(t13, a0), r) >> SHIFT;
}

// c: the 64 dequantised coefficients, natural order [v][u] -> px: the 64 samples [y][x]
VBT_HD inline void jpeg_idct_islow(const int32_t (&c)[64], uint8_t (&px)[64]) {
  int32_t ws[64];
#pragma unroll
  for (int u = 0; u < 8; u++) {                                      // pass 1: columns
    int32_t x[8], y[8];
#pragma unroll
    for (int v = 0; v < 8; v++) x[v] = c[v * 8 + u];
    jpeg_idct8<11>(x, y);
#pragma unroll
    for (int v = 0; v < 8; v++) ws[v * 8 + u] = y[v];
  }
#pragma unroll
  for (int v = 0; v < 8; v++) {                                      // pass 2: rows
    int32_t x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; u++) x[u] = ws[v * 8 + u];
    jpeg_idct8<18>(x, y);
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int32_t s = VBT_JA(y[u], 128);
      px[v * 8 + u] = (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
    }
  }
}
#undef VBT_JM
#undef VBT_JA
#undef VBT_JS

// ---- upsampling and colour
// The chroma sample of pixel (y, x): c = the component's plane, pw samples per row; the component holds dh x dw samples proper
// (ceil(H / vs), ceil(W / hs)) and nothing outside them is read.  hs = 1: the sample itself.  hs = 2: the triangle filter, by the
// rule of the IJG decoder - a component of one or two columns is replicated instead.
VBT_HD inline int jpeg_chroma_at(const uint8_t* c, int pw, int hs, int vs, int dw, int dh, int y, int x) {
  if (hs == 1) return c[(size_t)y * pw + x];
  const int i = x >> 1;
  if (vs == 1) {
    const uint8_t* r = c + (size_t)y * pw;
    if (dw <= 2) return r[i];
    if (x & 1) return i == dw - 1 ? r[i] : (3 * r[i] + r[i + 1] + 2) >> 2;
    return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;
  if (dw <= 2) return c[(size_t)j * pw + i];
  const int o = (y & 1) ? (j + 1 < dh ? j + 1 : dh - 1) : (j > 0 ? j - 1 : 0);
  const uint8_t *r0 = c + (size_t)j * pw, *r1 = c + (size_t)o * pw;
  const int cur = 3 * r0[i] + r1[i];
  if (x & 1) return i == dw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
  return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

VBT_HD inline void jpeg_ycc_rgb(int y, int cb, int cr, uint8_t* rgb) {
  cb -= 128;
  cr -= 128;
  const int r = y + ((91881 * cr + 32768) >> 16), g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16), b = y + ((116130 * cb + 32768) >> 16);
  rgb[0] = (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
  rgb[1] = (uint8_t)(g < 0 ? 0 : g > 255 ? 255 : g);
  rgb[2] = (uint8_t)(b < 0 ? 0 : b > 255 ? 255 : b);
}

// pixel (y, x) of a frame from its planes (planes: the frame's, jpeg_layout().blocks x 64 samples) -> rgb[3]
VBT_HD inline void jpeg_pixel(const JpegDesc& d, const JpegLayout& L, const uint8_t* planes, int y, int x, uint8_t* rgb) {
  const int Y = planes[(size_t)y * (L.bw[0] * 8) + x];
  if (d.ncomp == 1) { rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y; return; }
  const int dw = (d.W + d.hs - 1) / d.hs, dh = (d.H + d.vs - 1) / d.vs, pw = L.bw[1] * 8;
  const int cb = jpeg_chroma_at(planes + (size_t)L.boff[1] * 64, pw, d.hs, d.vs, dw, dh, y, x);
  const int cr = jpeg_chroma_at(planes + (size_t)L.boff[2] * 64, pw, d.hs, d.vs, dw, dh, y, x);
  jpeg_ycc_rgb(Y, cb, cr, rgb);
}

// ---- straight to the network input (include/vbt_hip.h, "JPEG stills"): preprocess_image of the decoded frame, the frame never written.
// jpeg_resize_scale: the source-to-target ratio of one axis, float32 as resize_frames_dev (detector.hip) and oracle/preprocess.py take it; computed on
// the host and handed to the kernel
inline float jpeg_resize_scale(int n_in, int n_out) { return (float)n_in / (float)n_out; }

// Output pixel (oy, ox) of the bilinear resize (half-pixel centres, float32, truncating cast: resize_bilinear_kernel, frames.hip)
// of a frame that exists only as its planes: the four taps are jpeg_pixel - fancy upsampling and colour at full resolution - and
// they are lerped in the order yuv_resize_kernel (yuv_kernels.h) uses.  sy = H / h, sx = W / w (jpeg_resize_scale).  Taps are
// clamped to 0 .. H - 1 and 0 .. W - 1, so jpeg_pixel reads what it reads for the frame's own pixels and nothing else.
// swap: out3 = B, G, R.  No contraction of a multiply and an add is allowed (built with -ffp-contract=off).
VBT_HD inline void jpeg_resized_pixel(const JpegDesc& d, const JpegLayout& L, const uint8_t* planes, float sy, float sx, int oy, int ox, int swap, uint8_t* out3) {
  const float iy = ((float)oy + 0.5f) * sy - 0.5f, ix = ((float)ox + 0.5f) * sx - 0.5f;
  const float fy = floorf(iy), fx = floorf(ix);
  const int cy = (int)ceilf(iy), cx = (int)ceilf(ix);
  const int y0 = (int)fy > 0 ? (int)fy : 0, y1 = cy < d.H - 1 ? cy : d.H - 1;
  const int x0 = (int)fx > 0 ? (int)fx : 0, x1 = cx < d.W - 1 ? cx : d.W - 1;
  const float ly = iy - fy, lx = ix - fx;
  uint8_t tl[3], tr[3], bl[3], br[3];
  jpeg_pixel(d, L, planes, y0, x0, tl);
  jpeg_pixel(d, L, planes, y0, x1, tr);
  jpeg_pixel(d, L, planes, y1, x0, bl);
  jpeg_pixel(d, L, planes, y1, x1, br);
  for (int c = 0; c < 3; c++) {
    const float a = (float)tl[c], b = (float)tr[c], e = (float)bl[c], f = (float)br[c];
    const float top = a + (b - a) * lx;
    const float bot = e + (f - e) * lx;
    const float v = top + (bot - top) * ly;
    out3[swap ? 2 - c : c] = (uint8_t)(int)v;
  }
}

}  // namespace vbt
