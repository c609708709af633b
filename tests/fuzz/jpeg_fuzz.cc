// Host-only build of the MJPEG import's parser and decoding core (vbt_amd/csrc/jpeg_parse.h, jpeg_core.h) for the sanitizer run of
// tests/test_mjpeg_decode_host.py:  g++ -fsanitize=address,undefined jpeg_fuzz.cc -o jpeg_fuzz
//   jpeg_fuzz <dir> [H W]   every file of <dir>: header parse (H W: the frame size a handle would insist on), then - the way the kernels of mjpeg_decode.hip do it, with the same
//                       functions - marker scan, one walk per restart interval, IDCT, upsampling and colour
// One line per file: "ok <name> status=<scan status> fnv=<FNV-1a of the RGB24 frame>" or "refused <name>: <why>".  The scan, the
// levels, the planes and the frame live in heap blocks of exactly their size, so a read or write outside one is a sanitizer report -
// the failure the test looks for.
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
  if (argc != 2 && argc != 4) { fprintf(stderr, "usage: jpeg_fuzz <dir> [H W]\n"); return 2; }
  const int want_H = argc == 4 ? atoi(argv[2]) : 0, want_W = argc == 4 ? atoi(argv[3]) : 0;
  for (const std::string& path : files_of(argv[1])) {
    uint8_t* file = nullptr;
    size_t n = 0;
    if (!read_file(path, &file, &n)) { printf("refused %s: unreadable\n", path.c_str()); free(file); continue; }
    vbt::JpegDesc d;
    std::string err;
    if (!vbt::jpeg_parse(file, n, want_H, want_W, &d, &err)) {
      printf("refused %s: %s\n", path.c_str(), err.c_str());
      free(file);
      continue;
    }
    if ((uint64_t)d.H * d.W > (1u << 24)) { printf("refused %s: %d x %d is more than this harness decodes\n", path.c_str(), d.W, d.H); free(file); continue; }
    uint8_t* scan = (uint8_t*)malloc(d.scan_len ? d.scan_len : 1);
    memcpy(scan, file + d.scan_off, d.scan_len);
    free(file);
    const vbt::JpegLayout L = vbt::jpeg_layout(d);
    int status = 0;
    // marker scan
    std::vector<uint32_t> pos((size_t)d.n_int - 1);
    uint32_t count = 0;
    for (uint32_t i = 0; i < d.scan_len; i++) {
      if (!vbt::jpeg_is_rst(scan, d.scan_len, i)) continue;
      if (count < pos.size()) {
        pos[count] = i;
        if ((scan[i + 1] & 7u) != (count & 7u)) status = std::max(status, (int)vbt::JPEG_ST_RST_ORDER);
      }
      count++;
    }
    if (count != pos.size()) status = std::max(status, (int)vbt::JPEG_ST_RST_COUNT);
    int16_t* levels = (int16_t*)calloc((size_t)L.blocks * 64, 2);
    uint8_t* planes = (uint8_t*)malloc((size_t)L.blocks * 64);
    uint8_t* rgb = (uint8_t*)malloc((size_t)d.H * d.W * 3);
    if (count == pos.size()) {
      for (int k = 0; k < d.n_int; k++) {
        const uint32_t start = k ? pos[(size_t)k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[(size_t)k] : d.scan_len;
        status = std::max(status, vbt::jpeg_decode_interval(d, L, scan, start, end, k, levels));
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
    uint32_t fnv = 2166136261u;
    for (int y = 0; y < d.H; y++) {
      for (int x = 0; x < d.W; x++) {
        uint8_t* o = rgb + ((size_t)y * d.W + x) * 3;
        vbt::jpeg_pixel(d, L, planes, y, x, o);
        for (int i = 0; i < 3; i++) fnv = (fnv ^ o[i]) * 16777619u;
      }
    }
    printf("ok %s status=%d fnv=%08x\n", path.c_str(), status, fnv);
    free(scan); free(levels); free(planes); free(rgb);
  }
  return 0;
}
