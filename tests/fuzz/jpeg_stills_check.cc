// Host-only build of the JPEG stills' path to the network input (vbt_amd/csrc/jpeg_parse.h, jpeg_core.h) for the sanitizer run of
// tests/test_jpeg_stills_host.py:  g++ -fsanitize=address,undefined jpeg_stills_check.cc -o jpeg_stills_check
//   jpeg_stills_check <dir> h w [h w ...]   every file of <dir>: header parse, entropy decode and IDCT with the functions the kernels
//                       of mjpeg_decode.hip call, then for every target size and both channel orders jpeg_resized_pixel - the
//                       statement mjpegd_resized_kernel runs per output pixel - over the whole output
// One line per (file, target, order): "ok <name> <h>x<w> swap=<0|1> blocks=<n> fnv=<FNV-1a of the [h][w][3] output>", or
// "refused <name>: <why>".  The planes live in a heap block of exactly blocks * 64 bytes, as a frame's share of the handle's scratch
// is, so a tap that reads one sample too far is a sanitizer report - the failure the test looks for.
#include <dirent.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../vbt_amd/csrc/jpeg_parse.h"

static std::vector<std::string> files_of(const char* dir) {
  std::vector<std::string> out;
  DIR* d = opendir(dir);
  if (!d) return out;
  while (dirent* e = readdir(d))
    if (e->d_name[0] != '.') out.push_back(std::string(dir) + "/" + e->d_name);
  closedir(d);
  std::sort(out.begin(), out.end());
  return out;
}

static bool read_file(const std::string& path, uint8_t** data, size_t* n) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  *n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  *data = (uint8_t*)malloc(*n ? *n : 1);
  const bool ok = fread(*data, 1, *n, f) == *n;
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 4 || argc % 2) { fprintf(stderr, "usage: jpeg_stills_check <dir> h w [h w ...]\n"); return 2; }
  for (const std::string& path : files_of(argv[1])) {
    uint8_t* file = nullptr;
    size_t n = 0;
    if (!read_file(path, &file, &n)) { printf("refused %s: unreadable\n", path.c_str()); free(file); continue; }
    vbt::JpegDesc d;
    std::string err;
    if (!vbt::jpeg_parse(file, n, 0, 0, &d, &err)) {
      printf("refused %s: %s\n", path.c_str(), err.c_str());
      free(file);
      continue;
    }
    if ((uint64_t)d.H * d.W > (1u << 24)) { printf("refused %s: %d x %d is more than this harness decodes\n", path.c_str(), d.W, d.H); free(file); continue; }
    uint8_t* scan = (uint8_t*)malloc(d.scan_len ? d.scan_len : 1);
    memcpy(scan, file + d.scan_off, d.scan_len);
    free(file);
    const vbt::JpegLayout L = vbt::jpeg_layout(d);
    std::vector<uint32_t> pos((size_t)d.n_int - 1);
    uint32_t count = 0;
    for (uint32_t i = 0; i < d.scan_len; i++) {
      if (!vbt::jpeg_is_rst(scan, d.scan_len, i)) continue;
      if (count < pos.size()) pos[count] = i;
      count++;
    }
    int16_t* levels = (int16_t*)calloc((size_t)L.blocks * 64, 2);
    uint8_t* planes = (uint8_t*)malloc((size_t)L.blocks * 64);
    if (count == pos.size()) {
      for (int k = 0; k < d.n_int; k++) {
        const uint32_t start = k ? pos[(size_t)k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[(size_t)k] : d.scan_len;
        vbt::jpeg_decode_interval(d, L, scan, start, end, k, levels);
      }
    }
    for (int c = 0; c < d.ncomp; c++) {
      for (int by = 0; by < L.bh[c]; by++) {
        for (int bx = 0; bx < L.bw[c]; bx++) {
          const int16_t* lv = levels + ((size_t)L.boff[c] + (size_t)by * L.bw[c] + bx) * 64;
          int32_t co[64];
          uint8_t px[64];
          for (int i = 0; i < 64; i++) co[i] = (int32_t)lv[i] * (int32_t)d.q[d.tq[c]][i];
          vbt::jpeg_idct_islow(co, px);
          for (int r = 0; r < 8; r++) memcpy(planes + (size_t)L.boff[c] * 64 + ((size_t)by * 8 + r) * ((size_t)L.bw[c] * 8) + (size_t)bx * 8, px + r * 8, 8);
        }
      }
    }
    for (int a = 2; a + 1 < argc; a += 2) {
      const int h = atoi(argv[a]), w = atoi(argv[a + 1]);
      if (h < 1 || w < 1 || h > 4096 || w > 4096) { fprintf(stderr, "target %s x %s\n", argv[a], argv[a + 1]); return 2; }
      const float sy = vbt::jpeg_resize_scale(d.H, h), sx = vbt::jpeg_resize_scale(d.W, w);
      uint8_t* out = (uint8_t*)malloc((size_t)h * w * 3);
      for (int swap = 0; swap < 2; swap++) {
        uint32_t fnv = 2166136261u;
        for (int oy = 0; oy < h; oy++)
          for (int ox = 0; ox < w; ox++) vbt::jpeg_resized_pixel(d, L, planes, sy, sx, oy, ox, swap, out + ((size_t)oy * w + ox) * 3);
        for (size_t i = 0; i < (size_t)h * w * 3; i++) fnv = (fnv ^ out[i]) * 16777619u;
        printf("ok %s %dx%d swap=%d blocks=%u fnv=%08x\n", path.c_str(), h, w, swap, L.blocks, fnv);
      }
      free(out);
    }
    free(scan); free(levels); free(planes);
  }
  return 0;
}
