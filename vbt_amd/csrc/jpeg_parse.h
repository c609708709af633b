// MJPEG import (include/vbt_hip.h, "MJPEG import"): the host header parser, from the bytes of one JPEG file to the descriptor the
// kernels read (jpeg_core.h: JpegDesc).  Pure C++ (no HIP): vbt_mjpeg_decode and vbt_jpeg_probe parse through this header, and
// tests/fuzz/jpeg_fuzz.cc builds the same code with g++ -fsanitize=address,undefined and feeds it truncated and bit-flipped files -
// whatever the bytes are, the answer is a descriptor whose every index and length is in range, or a refusal with its reason.
#pragma once
#include <cstdio>
#include <cstring>
#include <string>

#include "jpeg_core.h"

namespace vbt {

constexpr int JPEG_MAX_SIDE = 16384;

// canonical decoding tables (T.81 Annex C / F.2.2.3) of one DHT entry; false: more codes than a length holds
inline bool jpeg_build_huff(const uint8_t* bits, const uint8_t* vals, int n, JpegHuff* h) {
  memset(h, 0, sizeof(*h));
  memcpy(h->vals, vals, (size_t)(n < 256 ? n : 256));
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; l++) {
    h->valoff[l] = k - (int32_t)code;
    for (int i = 0; i < bits[l - 1]; i++) {
      if (code >= (1u << l) || k >= 256) return false;
      if (l <= 8)
        for (uint32_t j = 0; j < (1u << (8 - l)); j++) h->look[(code << (8 - l)) + j] = (uint16_t)((l << 8) | h->vals[k]);
      code++;
      k++;
    }
    h->maxcode[l] = bits[l - 1] ? (int32_t)code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[0] = -1;
  return true;
}

namespace jpeg_detail {
// Annex K.3: a frame without DHT uses these (the MJPG-in-AVI convention)
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

inline std::string fmt(const char* f, long a = 0, long b = 0, long c = 0, long d = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), f, a, b, c, d);
  return buf;
}
inline const char* sof_kind(int m) {
  return m == 0xC1 ? "extended sequential" : m == 0xC2 ? "progressive" : m >= 0xC9 ? "arithmetic" : (m == 0xC3 || m == 0xC7 || m == 0xCB) ? "lossless" : "hierarchical";
}
}  // namespace jpeg_detail

// b[0 .. n): one JPEG file.  expect_H, expect_W > 0: the size it must have.  true: *d is complete, scan_off counts from b.
// false: *err is the reason.
inline bool jpeg_parse(const uint8_t* b, uint64_t n, int expect_H, int expect_W, JpegDesc* d, std::string* err) {
  using jpeg_detail::fmt;
  auto fail = [&](const std::string& s) { *err = s; return false; };
  if (!b || n < 4 || b[0] != 0xFF || b[1] != 0xD8) return fail("no SOI marker");
  if (n > 0x7FFFFFFFull) return fail("a frame of 2 GiB or more");
  memset(d, 0, sizeof(*d));
  bool have_q[4] = {false, false, false, false}, have_h[2][2] = {{false, false}, {false, false}}, any_dht = false, have_sof = false;
  uint8_t cid[3] = {0, 0, 0}, chs[3] = {0, 0, 0}, cvs[3] = {0, 0, 0};
  uint64_t p = 2;
  while (true) {
    if (p + 2 > n) return fail("missing SOS: the data ends in the headers");
    if (b[p] != 0xFF) return fail(fmt("byte %ld: 0x%02lx where a marker should start", (long)p, b[p]));
    while (p + 1 < n && b[p + 1] == 0xFF) p++;                        // fill bytes
    if (p + 2 > n) return fail("missing SOS: the data ends in the headers");
    const int m = b[p + 1];
    p += 2;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) return fail("missing SOS: EOI before any scan");
    if (p + 2 > n) return fail(fmt("segment length past the end: marker 0x%02lx at byte %ld", m, (long)p - 2));
    const uint64_t L = ((uint64_t)b[p] << 8) | b[p + 1];
    if (L < 2 || p + L > n) return fail(fmt("segment length past the end: marker 0x%02lx at byte %ld says %ld bytes, %ld are left", m, (long)p - 2, (long)L, (long)(n - p)));
    uint64_t s = p + 2;
    const uint64_t e = p + L;
    if (m == 0xDB) {
      while (s < e) {
        const int pq = b[s] >> 4, tq = b[s] & 15;
        if (pq != 0) return fail("16-bit DQT (8-bit tables only)");
        if (tq > 3 || s + 65 > e) return fail("malformed DQT");
        for (int k = 0; k < 64; k++) d->q[tq][jpeg_zigzag(k)] = b[s + 1 + k];
        have_q[tq] = true;
        s += 65;
      }
    } else if (m == 0xC4) {
      while (s < e) {
        if (s + 17 > e) return fail("malformed DHT");
        const int tc = b[s] >> 4, th = b[s] & 15;
        int cnt = 0;
        for (int i = 0; i < 16; i++) cnt += b[s + 1 + i];
        if (tc > 1 || th > 1 || cnt > 256 || s + 17 + (uint64_t)cnt > e) return fail("malformed DHT (class 0-1, id 0-1, at most 256 symbols)");
        if (!jpeg_build_huff(b + s + 1, b + s + 17, cnt, tc ? &d->ac[th] : &d->dc[th])) return fail("malformed DHT (more codes than a length holds)");
        have_h[tc][th] = any_dht = true;
        s += 17 + (uint64_t)cnt;
      }
    } else if (m == 0xC0) {
      if (have_sof) return fail("two SOF segments");
      if (L < 8) return fail("malformed SOF0");
      const int prec = b[s], H = (b[s + 1] << 8) | b[s + 2], W = (b[s + 3] << 8) | b[s + 4], nc = b[s + 5];
      if (prec != 8) return fail(fmt("%ld-bit precision (8-bit only)", prec));
      if ((nc != 1 && nc != 3) || L != 8 + 3 * (uint64_t)nc) return fail(fmt("%ld components (1 or 3)", nc));
      if (H < 1 || W < 1 || H > JPEG_MAX_SIDE || W > JPEG_MAX_SIDE) return fail(fmt("size %ldx%ld outside 1..%ld", W, H, JPEG_MAX_SIDE));
      d->H = H; d->W = W; d->ncomp = nc;
      for (int i = 0; i < nc; i++) {
        cid[i] = b[s + 6 + 3 * i];
        chs[i] = b[s + 7 + 3 * i] >> 4;
        cvs[i] = b[s + 7 + 3 * i] & 15;
        d->tq[i] = b[s + 8 + 3 * i];
      }
      have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return fail(fmt("SOF%ld (", m - 0xC0) + jpeg_detail::sof_kind(m) + "): baseline SOF0 only");
    } else if (m == 0xDD) {
      if (L != 4) return fail("malformed DRI");
      d->ri = (b[s] << 8) | b[s + 1];
    } else if (m == 0xEE) {
      if (L >= 14 && memcmp(b + s, "Adobe", 5) == 0 && b[s + 11] != 1) return fail(fmt("Adobe APP14 transform %ld (YCbCr only)", b[s + 11]));
    } else if (m == 0xDA) {
      if (!have_sof) return fail("missing SOF before SOS");
      const int nc = d->ncomp;
      if (L != 6 + 2 * (uint64_t)nc || b[s] != nc) return fail("more than one scan (the scan does not hold all components)");
      for (int i = 0; i < nc; i++) {
        if (b[s + 1 + 2 * i] != cid[i]) return fail("the scan's components are not the frame's");
        d->td[i] = b[s + 2 + 2 * i] >> 4;
        d->ta[i] = b[s + 2 + 2 * i] & 15;
        if (d->td[i] > 1 || d->ta[i] > 1) return fail("Huffman table id above 1");
        if (d->tq[i] > 3 || !have_q[d->tq[i]]) return fail(fmt("missing DQT: table %ld", d->tq[i]));
      }
      if (b[s + 1 + 2 * nc] != 0 || b[s + 2 + 2 * nc] != 63 || b[s + 3 + 2 * nc] != 0) return fail("the scan is not Ss 0, Se 63, Ah/Al 0 (progressive?)");
      if (nc == 1) {
        d->hs = d->vs = 1;
      } else {
        const bool luma_ok = (chs[0] == 1 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 2);
        if (!luma_ok || chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1)
          return fail(fmt("sampling %ldx%ld,", chs[0], cvs[0]) + fmt("%ldx%ld,%ldx%ld (4:4:4, 4:2:2, 4:2:0 only)", chs[1], cvs[1], chs[2], cvs[2]));
        d->hs = chs[0];
        d->vs = cvs[0];
      }
      if (!any_dht) {
        for (int t = 0; t < 2; t++) {
          jpeg_build_huff(jpeg_detail::DC_BITS[t], jpeg_detail::DC_VALS, 12, &d->dc[t]);
          jpeg_build_huff(jpeg_detail::AC_BITS[t], jpeg_detail::AC_VALS[t], 162, &d->ac[t]);
          have_h[0][t] = have_h[1][t] = true;
        }
      }
      for (int i = 0; i < nc; i++)
        if (!have_h[0][d->td[i]] || !have_h[1][d->ta[i]]) return fail("missing DHT: a table the scan names");
      if (expect_H > 0 && expect_W > 0 && (d->H != expect_H || d->W != expect_W)) return fail(fmt("size %ldx%ld, the handle is for %ldx%ld", d->W, d->H, expect_W, expect_H));
      d->MW = (d->W + 8 * d->hs - 1) / (8 * d->hs);
      d->MH = (d->H + 8 * d->vs - 1) / (8 * d->vs);
      d->mcus = d->MW * d->MH;
      if (d->ri == 0 || d->ri > d->mcus) d->ri = d->mcus;            // (an interval longer than the frame is one interval)
      d->n_int = (d->mcus + d->ri - 1) / d->ri;
      uint64_t k = e;
      for (; k < n; k++) {
        if (b[k] != 0xFF) continue;
        if (k + 1 >= n) break;
        const int x = b[k + 1];
        if (x != 0 && x != 0xFF && !(x >= 0xD0 && x <= 0xD7)) break;
      }
      d->scan_off = e;
      d->scan_len = (uint32_t)(k - e);
      while (k + 1 < n) {                                            // behind the scan: nothing but EOI is expected
        if (b[k] != 0xFF) break;
        const int x = b[k + 1];
        if (x == 0xFF) { k++; continue; }
        if (x == 0xD9) break;
        if (x == 0xDA || (x >= 0xC0 && x <= 0xCF) || x == 0xDB || x == 0xDD) return fail("more than one scan");
        if (k + 4 > n) break;
        k += 2 + (((uint64_t)b[k + 2] << 8) | b[k + 3]);
      }
      return true;
    }
    p = e;
  }
}

}  // namespace vbt
