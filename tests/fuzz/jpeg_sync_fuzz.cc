// Host-only build of the MJPEG import's decode by subsequences that synchronise (vbt_amd/csrc/jpeg_core.h: jpeg_sync_walk,
// jpeg_sync_cold, jpeg_decode_rest) for the sanitizer run of tests/test_mjpeg_sync_host.py:
//   g++ -fsanitize=address,undefined jpeg_sync_fuzz.cc -o jpeg_sync_fuzz
//   jpeg_sync_fuzz <dir> <S> <N> [H W]   every file of <dir>, as jpeg_fuzz walks it, but every restart interval by the schedule of
//                       mjpegd_entropy_sync_kernel (mjpeg_decode.hip) with the functions that kernel calls: subsequences of S bytes,
//                       N lanes to a chunk (the lanes of a round in a plain loop, each reading the exits the round before left),
//                       rounds until no entry changes, prefix sums, the storing walk, or one lane finishing the interval
// One line per file: jpeg_fuzz's ("ok <name> status=<scan status> fnv=<FNV-1a of the RGB24 frame>" or "refused <name>: <why>"), an
// "ok" line followed by " rounds=<most rounds of any chunk> single=<intervals the single lane finished> lanes=<lanes of the longest
// interval>".  A chunk of L lanes that takes more than min(L, N) + 1 rounds ends the program with exit code 3.  The scan, the levels,
// the planes and the frame live in heap blocks of exactly their size, so a read or write outside one is a sanitizer report.
#include <dirent.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../vbt_amd/csrc/jpeg_parse.h"

using namespace vbt;

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

struct Tally {
  int rounds = 0, single = 0;
  uint32_t lanes = 0;
};

// restart interval k, the way one workgroup of mjpegd_entropy_sync_kernel decodes it; returns the status it raises
static int sync_interval(const JpegDesc& d, const JpegLayout& L, const uint8_t* scan, uint32_t start, uint32_t end, int k, int16_t* levels, uint32_t S, uint32_t N,
                         Tally* tally) {
  const uint32_t len = end > start ? end - start : 0, lanes = len ? (len + S - 1) / S : 1;
  const uint32_t nblocks = jpeg_interval_blocks(d, k);
  const int m0 = k * d.ri, max_syms = (int)(8 * S + 32);
  tally->lanes = std::max(tally->lanes, lanes);
  const JpegHuff huff[4] = {d.dc[0], d.dc[1], d.ac[0], d.ac[1]};      // (the kernel's copy in LDS)
  JpegSyncState carry;
  carry.pos = start; carry.buk = 0;
  uint32_t cb = 0, cdc[3] = {0, 0, 0};
  std::vector<JpegSyncState> entry(N), exits(N), seen(N);
  std::vector<JpegSyncWalk> w(N);
  std::vector<uint32_t> limit(N), base(4 * (size_t)N);
  std::vector<char> go(N);
  for (uint32_t c0 = 0; c0 < lanes; c0 += N) {
    const uint32_t n_act = std::min(N, lanes - c0);
    for (uint32_t i = 0; i < n_act; i++) {
      const uint32_t first = start + (c0 + i) * S;
      limit[i] = end - first > S ? first + S : end;
      entry[i] = i == 0 ? carry : jpeg_sync_cold(scan, first);
      w[i].exit = entry[i]; w[i].blocks = 0; w[i].dc[0] = w[i].dc[1] = w[i].dc[2] = 0; w[i].bad_at = JPEG_SYNC_NONE;
    }
    int rounds = 0;
    for (uint32_t r = 0; r <= N; r++) {
      bool any = false;
      seen = exits;                                                   // what the barrier in front of the round's walks leaves every lane to read
      for (uint32_t i = 0; i < n_act; i++) {
        go[i] = r == 0;
        if (r > 0 && i > 0 && !jpeg_sync_same(seen[i - 1], entry[i])) { entry[i] = seen[i - 1]; go[i] = 1; }
        any = any || go[i];
      }
      if (!any) break;
      for (uint32_t i = 0; i < n_act; i++) {
        if (!go[i]) continue;
        w[i] = jpeg_sync_walk<false>(d, L, huff, scan, end, entry[i], limit[i], max_syms, 0, 0, 0, nullptr, nullptr);
        exits[i] = w[i].exit;
      }
      rounds++;
    }
    tally->rounds = std::max(tally->rounds, rounds);
    if ((uint32_t)rounds > n_act + 1) { fprintf(stderr, "a chunk of %u lanes took %d rounds\n", n_act, rounds); exit(3); }
    uint32_t run[4] = {cb, cdc[0], cdc[1], cdc[2]};
    const bool last = lanes - c0 <= N;
    bool dirty = false;
    for (uint32_t i = 0; i < n_act; i++) {
      for (int j = 0; j < 4; j++) base[4 * (size_t)i + j] = run[j];
      if (w[i].bad_at != JPEG_SYNC_NONE && run[0] + w[i].bad_at < nblocks) dirty = true;
      run[0] += w[i].blocks; run[1] += w[i].dc[0]; run[2] += w[i].dc[1]; run[3] += w[i].dc[2];
    }
    if (last && run[0] < nblocks) dirty = true;
    if (dirty) {
      tally->single++;
      return jpeg_decode_rest(d, L, scan, end, k, carry, cb, cdc, levels);
    }
    for (uint32_t i = 0; i < n_act; i++)
      jpeg_sync_walk<true>(d, L, huff, scan, end, entry[i], limit[i], max_syms, m0, base[4 * (size_t)i], nblocks, &base[4 * (size_t)i + 1], levels);
    carry = exits[n_act - 1];
    cb = run[0]; cdc[0] = run[1]; cdc[1] = run[2]; cdc[2] = run[3];
    if (cb >= nblocks) break;
  }
  return JPEG_ST_OK;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 6) { fprintf(stderr, "usage: jpeg_sync_fuzz <dir> <S> <N> [H W]\n"); return 2; }
  const uint32_t S = (uint32_t)atoi(argv[2]), N = (uint32_t)atoi(argv[3]);
  if (S < 4 || S > 4096 || (S & (S - 1)) || N < 1 || N > 4096) { fprintf(stderr, "S: a power of two in 4..4096; N: 1..4096\n"); return 2; }
  const int want_H = argc == 6 ? atoi(argv[4]) : 0, want_W = argc == 6 ? atoi(argv[5]) : 0;
  for (const std::string& path : files_of(argv[1])) {
    uint8_t* file = nullptr;
    size_t n = 0;
    if (!read_file(path, &file, &n)) { printf("refused %s: unreadable\n", path.c_str()); free(file); continue; }
    JpegDesc d;
    std::string err;
    if (!jpeg_parse(file, n, want_H, want_W, &d, &err)) {
      printf("refused %s: %s\n", path.c_str(), err.c_str());
      free(file);
      continue;
    }
    if ((uint64_t)d.H * d.W > (1u << 24)) { printf("refused %s: %d x %d is more than this harness decodes\n", path.c_str(), d.W, d.H); free(file); continue; }
    uint8_t* scan = (uint8_t*)malloc(d.scan_len ? d.scan_len : 1);
    memcpy(scan, file + d.scan_off, d.scan_len);
    free(file);
    const JpegLayout L = jpeg_layout(d);
    int status = 0;
    std::vector<uint32_t> pos((size_t)d.n_int - 1);
    uint32_t count = 0;
    for (uint32_t i = 0; i < d.scan_len; i++) {
      if (!jpeg_is_rst(scan, d.scan_len, i)) continue;
      if (count < pos.size()) {
        pos[count] = i;
        if ((scan[i + 1] & 7u) != (count & 7u)) status = std::max(status, (int)JPEG_ST_RST_ORDER);
      }
      count++;
    }
    if (count != pos.size()) status = std::max(status, (int)JPEG_ST_RST_COUNT);
    int16_t* levels = (int16_t*)calloc((size_t)L.blocks * 64, 2);
    uint8_t* planes = (uint8_t*)malloc((size_t)L.blocks * 64);
    uint8_t* rgb = (uint8_t*)malloc((size_t)d.H * d.W * 3);
    Tally tally;
    if (count == pos.size()) {
      for (int k = 0; k < d.n_int; k++) {
        const uint32_t start = k ? pos[(size_t)k - 1] + 2 : 0, end = k + 1 < d.n_int ? pos[(size_t)k] : d.scan_len;
        status = std::max(status, sync_interval(d, L, scan, start, end, k, levels, S, N, &tally));
      }
    }
    for (int c = 0; c < d.ncomp; c++) {
      for (int by = 0; by < L.bh[c]; by++) {
        for (int bx = 0; bx < L.bw[c]; bx++) {
          const int16_t* lv = levels + ((size_t)L.boff[c] + (size_t)by * L.bw[c] + bx) * 64;
          int32_t co[64];
          uint8_t px[64];
          for (int i = 0; i < 64; i++) co[i] = (int32_t)lv[i] * (int32_t)d.q[d.tq[c]][i];
          jpeg_idct_islow(co, px);
          for (int r = 0; r < 8; r++) memcpy(planes + (size_t)L.boff[c] * 64 + ((size_t)by * 8 + r) * ((size_t)L.bw[c] * 8) + (size_t)bx * 8, px + r * 8, 8);
        }
      }
    }
    uint32_t fnv = 2166136261u;
    for (int y = 0; y < d.H; y++) {
      for (int x = 0; x < d.W; x++) {
        uint8_t* o = rgb + ((size_t)y * d.W + x) * 3;
        jpeg_pixel(d, L, planes, y, x, o);
        for (int i = 0; i < 3; i++) fnv = (fnv ^ o[i]) * 16777619u;
      }
    }
    printf("ok %s status=%d fnv=%08x rounds=%d single=%d lanes=%u\n", path.c_str(), status, fnv, tally.rounds, tally.single, tally.lanes);
    free(scan); free(levels); free(planes); free(rgb);
  }
  return 0;
}
