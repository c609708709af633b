"""The staged frame layout and the upload plan of the host-fed pipeline (vbt_amd/csrc/upload_plan.h), host side (no GPU): a stand-alone
program executes the plans with memcpy on host buffers and walks the whole of a small space - network rows h in 1..6; source rows H from
2h + 1 to 40 and every multiple of h up to 48 (even H only with a chroma plane); row bytes 3, 4, 6, 8; packed rows and luma + chroma
plane; 1..4 frames; first frame slot 0..2; compact on and off.  Per case:

  - content: the source bytes depend on their position, the staged buffer starts as a sentinel.  After the plan pair d of frame b
    holds source rows q(d), q(d) + 1 at (slot0 + b) * frame_bytes + 2 d * row, with q(d) recomputed here from the resize kernels'
    statements (sy = (float)H / (float)h; iy = (d + 0.5f) * sy - 0.5f; q = min(max((int)floorf(iy), 0), H - 2) - and the same with the
    scale not rounded first, (d + 0.5f) * (float)H / (float)h: the two agree on every size used here); every chroma byte c is at
    chroma_off + c; with compact off the frame is there whole;
  - bounds: every byte of [slot0, slot0 + nf) * frame_bytes is written exactly once and no other, no source byte at or beyond
    nf * frame is read, and a strided copy is no wider than either of its pitches (what hipMemcpy2DAsync asks);
  - bytes: the sum of width * height is nf * frame_bytes, frame_bytes = 2 h row for packed rows and
    2 (h - 1) row + (H - q(h - 1)) row + H / 2 * row with a chroma plane (_compact_bytes of tests/test_gpu_pixfmt.py);
  - copies - the call count is what the upload costs the host: whole frames 1 flat copy; packed rows 1 at an integer scale, nf at a
    uniform pitch, else h; chroma plane (uniform && nf < h - 1 ? nf : h - 1) + 1, `uniform` being what each path of the upload has
    always asked: all of the pairs it copies as pairs (h of them, or h - 1) one step apart, and at least two of them.

At (H, h) = (642, 320), (643, 320), (1080, 320), (1920, 320), (1080, 448) the same counts and bytes, without executing the plan.

The expectations are restated in the program, not taken from a second call of the functions under test.  The program is built twice,
plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "upload_plan.h"

using namespace vbt;

static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

// first source row of output row d, as resize_bilinear_kernel / yuv_resize_kernel / pix_resize_kernel compute it
static int q(int d, int H, int h) {
  const float sy = (float)H / (float)h;
  const float iy = ((float)d + 0.5f) * sy - 0.5f;
  const int a = std::min(std::max((int)floorf(iy), 0), H - 2);
  const float iy2 = ((float)d + 0.5f) * (float)H / (float)h - 0.5f;
  const int b = std::min(std::max((int)floorf(iy2), 0), H - 2);
  CHECK(a == b, "H %d h %d d %d: row %d with the scale rounded first, %d without", H, h, d, a, b);
  return a;
}

struct Want { size_t frame, staged, chroma_off; long copies; };

// the layout and the copy count, from the description of the upload
static Want want_of(size_t row, bool chroma, int H, int h, bool compact, int nf) {
  Want w;
  w.frame = chroma ? (size_t)H * row + (size_t)(H / 2) * row : (size_t)H * row;
  if (!compact) {
    w.staged = w.frame;
    w.chroma_off = chroma ? (size_t)H * row : 0;
    w.copies = 1;
    return w;
  }
  const int step = h > 1 ? q(1, H, h) - q(0, H, h) : 0;
  if (!chroma) {
    w.staged = (size_t)2 * h * row;
    w.chroma_off = 0;
    bool uniform = h > 1;
    for (int d = 1; d < h; d++) uniform = uniform && q(d, H, h) - q(d - 1, H, h) == step;
    w.copies = uniform && (long)step * h == H ? 1 : uniform ? nf : h;
  } else {
    w.staged = (size_t)2 * (h - 1) * row + (size_t)(H - q(h - 1, H, h)) * row + (size_t)(H / 2) * row;
    w.chroma_off = w.staged - (size_t)(H / 2) * row;
    bool uniform = h > 2;
    for (int d = 1; d < h - 1; d++) uniform = uniform && q(d, H, h) - q(d - 1, H, h) == step;
    w.copies = (uniform && nf < h - 1 ? nf : h - 1) + 1;
  }
  return w;
}

static uint8_t src_byte(size_t i) { return (uint8_t)(((uint32_t)i * 2654435761u) >> 11); }

// layout, copy count and byte count of one case; the plan is left in `plan`
static bool check_plan(size_t row, bool chroma, int H, int h, bool compact, int slot0, int nf, std::vector<int>& tab, std::vector<UploadCopy>& plan,
                       Want* w_out) {
  const long f0 = fails;
  const Want w = want_of(row, chroma, H, h, compact, nf);
  if (compact) {
    row_table(H, h, tab);
    CHECK((int)tab.size() == h, "H %d h %d: table of %zu rows", H, h, tab.size());
    for (int d = 0; d < h && d < (int)tab.size(); d++) CHECK(tab[d] == q(d, H, h), "H %d h %d: p(%d) = %d, the kernels read %d", H, h, d, tab[d], q(d, H, h));
  }
  const StagedLayout sl = staged_layout(row, chroma, H, h, compact, tab);
  CHECK(sl.frame_bytes == w.staged && sl.chroma_off == w.chroma_off, "row %zu chroma %d H %d h %d compact %d: staged frame %zu / chroma at %zu, expected %zu / %zu",
        row, (int)chroma, H, h, (int)compact, sl.frame_bytes, sl.chroma_off, w.staged, w.chroma_off);
  upload_plan(row, chroma, H, h, compact, tab, slot0, nf, plan);
  CHECK((long)plan.size() == w.copies, "row %zu chroma %d H %d h %d compact %d nf %d: %zu copies, expected %ld", row, (int)chroma, H, h, (int)compact, nf,
        plan.size(), w.copies);
  size_t bytes = 0;
  for (const UploadCopy& c : plan) {
    bytes += c.width * c.height;
    CHECK(c.flat == !compact, "row %zu chroma %d H %d h %d compact %d: flat mark %d", row, (int)chroma, H, h, (int)compact, (int)c.flat);
    if (c.flat) CHECK(c.height == 1, "a flat copy of %zu rows", c.height);
    else CHECK(c.width <= c.dst_pitch && c.width <= c.src_pitch, "H %d h %d: a strided copy %zu wide at pitches %zu / %zu", H, h, c.width, c.dst_pitch, c.src_pitch);
  }
  CHECK(bytes == (size_t)nf * w.staged, "row %zu chroma %d H %d h %d compact %d nf %d: %zu bytes, expected %zu", row, (int)chroma, H, h, (int)compact, nf, bytes,
        (size_t)nf * w.staged);
  *w_out = w;
  return fails == f0;
}

static void run_case(size_t row, bool chroma, int H, int h, bool compact, int slot0, int nf) {
  cases++;
  static std::vector<int> tab;
  static std::vector<UploadCopy> plan;
  Want w;
  if (!check_plan(row, chroma, H, h, compact, slot0, nf, tab, plan, &w)) return;   // (do not execute a plan that is already wrong)
  // exactly nf source frames on the heap: the sanitizer build sees a read past them; one spare frame slot behind the staged range
  std::vector<uint8_t> src((size_t)nf * w.frame), dst((size_t)(slot0 + nf + 1) * w.staged, 0xA5);
  std::vector<uint8_t> writes(dst.size(), 0);
  for (size_t i = 0; i < src.size(); i++) src[i] = src_byte(i);
  const size_t lo = (size_t)slot0 * w.staged, hi = (size_t)(slot0 + nf) * w.staged;
  for (const UploadCopy& c : plan) {
    for (size_t r = 0; r < c.height; r++) {
      const size_t d0 = c.dst_off + r * c.dst_pitch, s0 = c.src_off + r * c.src_pitch;
      if (d0 < lo || d0 + c.width > hi) { CHECK(false, "H %d h %d: a copy writes [%zu, %zu), the frames' range is [%zu, %zu)", H, h, d0, d0 + c.width, lo, hi); return; }
      if (s0 + c.width > src.size()) { CHECK(false, "H %d h %d: a copy reads up to %zu of %zu source bytes", H, h, s0 + c.width, src.size()); return; }
      memcpy(dst.data() + d0, src.data() + s0, c.width);
      for (size_t i = 0; i < c.width; i++) writes[d0 + i]++;
    }
  }
  long bad_cover = 0, bad_content = 0;
  for (size_t i = 0; i < dst.size(); i++) {
    const bool in = i >= lo && i < hi;
    if (writes[i] != (in ? 1 : 0) || (!in && dst[i] != 0xA5)) bad_cover++;
  }
  for (int b = 0; b < nf; b++) {
    const uint8_t* st = dst.data() + (size_t)(slot0 + b) * w.staged;
    const size_t f = (size_t)b * w.frame;   // source frame b
    if (!compact) {
      for (size_t i = 0; i < w.frame; i++) bad_content += st[i] != src_byte(f + i);
    } else {
      for (int d = 0; d < h; d++)
        for (size_t i = 0; i < 2 * row; i++) bad_content += st[(size_t)2 * d * row + i] != src_byte(f + (size_t)q(d, H, h) * row + i);
    }
    if (chroma)
      for (size_t c = 0; c < (size_t)(H / 2) * row; c++) bad_content += st[w.chroma_off + c] != src_byte(f + (size_t)H * row + c);
  }
  CHECK(bad_cover == 0, "row %zu chroma %d H %d h %d compact %d slot0 %d nf %d: %ld bytes written twice, not at all or outside the frames", row, (int)chroma, H, h,
        (int)compact, slot0, nf, bad_cover);
  CHECK(bad_content == 0, "row %zu chroma %d H %d h %d compact %d slot0 %d nf %d: %ld bytes are not where the kernels read them", row, (int)chroma, H, h,
        (int)compact, slot0, nf, bad_content);
}

int main() {
  const size_t rows[] = {3, 4, 6, 8};
  for (int h = 1; h <= 6; h++)
    for (int H = 2 * h + 1; H <= 48; H++) {
      if (H > 40 && H % h != 0) continue;
      for (int chroma = 0; chroma < 2; chroma++) {
        if (chroma && (H & 1)) continue;
        for (size_t row : rows)
          for (int nf = 1; nf <= 4; nf++)
            for (int slot0 = 0; slot0 <= 2; slot0++)
              for (int compact = 0; compact < 2; compact++) run_case(row, chroma != 0, H, h, compact != 0, slot0, nf);
      }
    }
  printf("%ld cases\n", cases);
  CHECK(cases > 30000, "only %ld cases", cases);
  // the sizes the pipeline's GPU tests and the benchmark run at: counts and bytes
  {
    const int sizes[][2] = {{642, 320}, {643, 320}, {1080, 320}, {1920, 320}, {1080, 448}};
    const int nfs[] = {1, 8, 64, 318, 319};   // (a chroma-plane upload goes per frame below h - 1 frames)
    std::vector<int> tab;
    std::vector<UploadCopy> plan;
    for (const auto& s : sizes)
      for (int chroma = 0; chroma < 2; chroma++) {
        if (chroma && (s[0] & 1)) continue;
        for (size_t row : {(size_t)1920, (size_t)3840, (size_t)5760})
          for (int nf : nfs)
            for (int compact = 0; compact < 2; compact++) {
              Want w;
              check_plan(row, chroma != 0, s[0], s[1], compact != 0, 1, nf, tab, plan, &w);
              // 1920 -> 320 is the one integer scale among them: ONE copy for packed rows; the others go row by row
              if (compact && !chroma) CHECK(w.copies == (s[0] == 1920 ? 1 : s[1]), "%d -> %d rows: %ld copies expected?", s[0], s[1], w.copies);
              if (compact && chroma && s[0] == 1920) CHECK(w.copies == (nf < 319 ? nf : 319) + 1, "1920 -> 320 rows, %d frames: %ld copies expected?", nf, w.copies);
            }
      }
  }
  printf("%ld failures\n", fails);
  return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_upload_plan(tmp_path, sanitize):
    src, exe = tmp_path / "upload_plan.cpp", tmp_path / "upload_plan"
    src.write_text(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I" + os.path.join(ROOT, "vbt_amd", "csrc"), str(src), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("0 failures") and "runtime error" not in res.stderr, res.stdout[-3000:] + res.stderr[-3000:]
