// Live rep analysis of the on-device tracker (vbt_tracker_live_enable / poll / tracks): the VelocityTracker of every id that can still
// win the export, fed after every tracker launch (live_tables.h holds the tables and their device helpers).
#include "common.h"
#include "live_tables.h"
#include "tracker_host.h"

namespace vbt {

// One wavefront per clip, after every tracker launch, on the tracker launch's stream: consumes rows [cursor, nrows) of the clip's log,
// whatever number of frames the launch walked.  Lane e owns entry e (lane 0 also entry 64): the rows of one frame carry distinct ids,
// so the entries advance side by side, each lane applying its id's rows in log order.  Then the leader: export_id() as it stands.
// M: rep metrics on (b.metrics is there); M = false is the kernel as it is without them.
template <bool M>
__global__ __launch_bounds__(64) void live_analyze_kernel(const ClipState* states, const Row* rows, int rows_cap, LiveBufs b, LiveCfg c) {
  __shared__ long long s_keep[LIVE_ENTRIES];   // ids that can still win the export: the live tracks' and the best dead one
  __shared__ long long s_eid[LIVE_ENTRIES];    // entry ids (-1: free)
  __shared__ int s_free[LIVE_ENTRIES];
  __shared__ int s_ver[LIVE_ENTRIES];
  const int clip = blockIdx.x, lane = threadIdx.x;
  const ClipState& st = states[clip];
  const Row* R = rows + (size_t)clip * rows_cap;
  LiveClip& L = b.clips[clip];
  LiveEntry* E = b.ents + (size_t)clip * LIVE_ENTRIES;
  const int ntrk = st.ntrk, best = st.best_id;
  const int nkeep = ntrk + (best >= 0 ? 1 : 0);
  for (int k = lane; k < LIVE_ENTRIES; k += 64) {
    s_keep[k] = k < ntrk ? (long long)st.trk[st.order[k]].id + 1 : (k == ntrk && best >= 0 ? (long long)best : -2);
    s_eid[k] = E[k].id;
  }
  __syncthreads();
  // retire the entries of ids that can no longer win
  for (int e = lane; e < LIVE_ENTRIES; e += 64) {
    const long long id = s_eid[e];
    bool keep = false;
    for (int k = 0; k < nkeep; k++) keep = keep || s_keep[k] == id;
    if (id >= 0 && !keep) { s_eid[e] = -1; E[e].id = -1; }
  }
  __syncthreads();
  // a keeper without an entry takes a free one, the i-th such keeper the i-th free entry (enough of them: one entry per keeper at most)
  auto missing = [&](int k) {
    if (k >= nkeep) return false;
    for (int e = 0; e < LIVE_ENTRIES; e++)
      if (s_eid[e] == s_keep[k]) return false;
    return true;
  };
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool need0 = missing(lane), need1 = lane == 0 && missing(64);
  const bool free0 = s_eid[lane] < 0, free1 = lane == 0 && s_eid[64] < 0;
  const unsigned long long mn = __ballot(need0), mf = __ballot(free0);
  if (free0) s_free[__popcll(mf & below)] = lane;
  if (free1) s_free[__popcll(mf)] = 64;
  __syncthreads();
  if (need0) { const int e = s_free[__popcll(mn & below)]; live_entry_init(E[e], s_keep[lane]); s_eid[e] = s_keep[lane]; }
  if (need1) { const int e = s_free[__popcll(mn)]; live_entry_init(E[e], s_keep[64]); s_eid[e] = s_keep[64]; }
  __syncthreads();
  // the new rows, 64 at a time: lane j reads row base + j's id, every entry lane collects the positions of its id's rows
  const int n = st.nrows, cur = L.cursor;
  const int my0 = (int)s_eid[lane], my1 = lane == 0 ? (int)s_eid[64] : -3;
  for (int base = cur; base < n; base += 64) {
    const int rid = base + lane < n ? (int)R[base + lane].id : -4;
    unsigned long long m0 = 0ull, m1 = 0ull;
    for (int j = 0; j < 64; j++) {
      const int v = __shfl(rid, j);
      m0 |= (unsigned long long)(v == my0) << j;
      m1 |= (unsigned long long)(v == my1) << j;
    }
    while (m0) {
      const int j = __ffsll((long long)m0) - 1;
      m0 &= m0 - 1;
      live_apply<M>(E[lane], R[base + j], b, c, clip, lane);
    }
    while (m1) {
      const int j = __ffsll((long long)m1) - 1;
      m1 &= m1 - 1;
      live_apply<M>(E[64], R[base + j], b, c, clip, 64);
    }
  }
  s_ver[lane] = my0 >= 0 ? E[lane].s.ver : -1;
  if (lane == 0) s_ver[64] = my1 >= 0 ? E[64].s.ver : -1;
  __syncthreads();
  if (lane == 0) {
    const int ld = export_id(st);
    int ver = -1;
    for (int e = 0; e < LIVE_ENTRIES; e++)
      if (ld >= 0 && s_eid[e] == ld) ver = s_ver[e];
    if (ld != L.leader || ver != L.leader_ver) L.seq += 1;
    L.leader = ld;
    L.leader_ver = ver;
    L.cursor = n;
    if (st.rows_overflow > 0) L.flags |= LIVE_ROWS_LOST;
  }
}

// vbt_tracker_live_poll: per clip a record { int64 leader; int32 rows_consumed, n_phases, phase_state, overflow; uint64 seq } (=
// vbt_live_clip) + the leader's phases [cap][6], packed for ONE copy.  A flagged clip reports no phases.  mdst != null
// (vbt_tracker_live_poll_ex; rep metrics enabled, M): the metrics of those phases too, clip c's at mdst + c * cap * VT_METRICS.
template <bool M>
__global__ __launch_bounds__(64) void live_pack_kernel(LiveBufs b, LiveCfg c, int flush, int cap, unsigned char* out, double* mdst) {
  __shared__ int s_e, s_n, s_flags;
  const int clip = blockIdx.x, lane = threadIdx.x;
  const LiveClip& L = b.clips[clip];
  const LiveEntry* E = b.ents + (size_t)clip * LIVE_ENTRIES;
  unsigned char* o = out + (size_t)clip * (32 + (size_t)cap * 48);
  const long long ld = L.leader;
  if (lane == 0) { s_e = -1; s_flags = L.flags; s_n = 0; }
  __syncthreads();
  if (ld >= 0 && E[lane].id == ld) s_e = lane;
  if (lane == 0 && ld >= 0 && E[64].id == ld) s_e = 64;
  __syncthreads();
  const int e = s_e;
  double* view = b.view + (size_t)clip * c.phase_cap * 6;
  double* mview = M ? b.mview + (size_t)clip * c.phase_cap * VT_METRICS : nullptr;
  int n = 0;
  if (e >= 0) n = live_view<M>(E[e], b, c, clip, e, flush != 0, view, &s_n, &s_flags, lane, mview);
  else if (lane == 0 && ld >= 0) s_flags |= LIVE_ROWS_LOST;   // the leader's rows are not in the log
  __syncthreads();
  const int flags = s_flags;
  if (flags) n = 0;
  if (lane == 0) {
    *(long long*)o = ld;
    int* h = (int*)(o + 8);
    h[0] = L.cursor; h[1] = n; h[2] = e >= 0 ? E[e].s.phase : 2; h[3] = flags;
    *(unsigned long long*)(o + 24) = L.seq;
  }
  double* dst = (double*)(o + 32);
  for (int i = lane; i < min(n, cap) * 6; i += 64) dst[i] = view[i];
  if (M) {
    double* md = mdst + (size_t)clip * cap * VT_METRICS;
    for (int i = lane; i < min(n, cap) * VT_METRICS; i += 64) md[i] = mview[i];
  }
}

// vbt_tracker_live_tracks: every entry of one clip, LIVE_ENTRIES records { int64 id; int32 n_rows, n_phases, flags, phase_state;
// double phases[phase_cap][6] } (free entries: id -1).  One wavefront per entry.
__global__ __launch_bounds__(64) void live_tracks_kernel(LiveBufs b, LiveCfg c, int clip, int flush, unsigned char* out) {
  __shared__ int s_n, s_flags;
  const int e = blockIdx.x, lane = threadIdx.x;
  const LiveEntry& x = b.ents[(size_t)clip * LIVE_ENTRIES + e];
  unsigned char* o = out + (size_t)e * (24 + (size_t)c.phase_cap * 48);
  if (lane == 0) { s_n = 0; s_flags = b.clips[clip].flags; }
  __syncthreads();
  const long long id = x.id;
  int n = 0;
  if (id >= 0) n = live_view(x, b, c, clip, e, flush != 0, (double*)(o + 24), &s_n, &s_flags, lane);
  if (lane == 0) {
    *(long long*)o = id;
    int* h = (int*)(o + 8);
    h[0] = id >= 0 ? x.nrows : 0; h[1] = s_flags ? 0 : n; h[2] = s_flags; h[3] = id >= 0 ? x.s.phase : 2;
  }
}

__global__ void live_init_kernel(LiveClip* clips, LiveEntry* ents, int n_clips) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_clips) live_clip_init(clips[i]);
  if (i < n_clips * LIVE_ENTRIES) live_entry_free(ents[i]);
}

int live_after(vbt_tracker* t, hipStream_t st) {
  t->stepped = true;
  if (!t->live) return VBT_OK;
  if (t->lb.metrics) live_analyze_kernel<true><<<t->n_clips, 64, 0, st>>>(t->states.get(), t->rows.get(), t->rows_cap, t->lb, t->lc);
  else live_analyze_kernel<false><<<t->n_clips, 64, 0, st>>>(t->states.get(), t->rows.get(), t->rows_cap, t->lb, t->lc);
  VBT_HIP_CHECK(hipGetLastError());
  return VBT_OK;
}

void live_init(vbt_tracker* t) {
  live_init_kernel<<<(t->n_clips * LIVE_ENTRIES + 63) / 64, 64>>>(t->lb.clips, t->lb.ents, t->n_clips);
}

void live_free(vbt_tracker* t) {
  t->live_clips.reset(); t->live_ents.reset(); t->live_paths.reset(); t->live_phases.reset(); t->live_view.reset();
  t->live_poll.reset();
  t->live_metrics.reset(); t->live_mview.reset();
  t->lb = LiveBufs{};
  t->live = false;
}

bool live_metrics_alloc(vbt_tracker* t) {
  if (!t->live || !t->rep_metrics || t->lb.metrics) return true;
  const size_t n = (size_t)t->n_clips, cells = (size_t)VT_METRICS * t->lc.phase_cap;
  if (t->live_metrics.alloc(cells * n * LIVE_ENTRIES) != hipSuccess || t->live_mview.alloc(cells * n) != hipSuccess) {
    t->live_metrics.reset(); t->live_mview.reset();
    return false;
  }
  t->lb.metrics = t->live_metrics.get();
  t->lb.mview = t->live_mview.get();
  return true;
}

}  // namespace vbt

using namespace vbt;

extern "C" {

int vbt_tracker_live_enable(vbt_tracker* t, int path_cap, int phase_cap, double plate_diameter, double diff_threshold, double min_distance) {
  if (!t) { set_error("NULL tracker"); return VBT_ERR_ARG; }
  if (path_cap < 2 || path_cap > VBT_LIVE_MAX_PATH || phase_cap < 1 || phase_cap > VBT_LIVE_MAX_PHASES) {
    set_error("vbt_tracker_live_enable: path_cap must be in [2, %d], phase_cap in [1, %d]", VBT_LIVE_MAX_PATH, VBT_LIVE_MAX_PHASES);
    return VBT_ERR_ARG;
  }
  if (t->live) { set_error("vbt_tracker_live_enable: live analysis is already enabled"); return VBT_ERR_STATE; }
  if (t->stepped) { set_error("vbt_tracker_live_enable: the tracker has been stepped (enable before the first update, or after a reset)"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(t->device));
  const size_t n = (size_t)t->n_clips, ne = n * LIVE_ENTRIES;
  if (t->live_clips.alloc(n) != hipSuccess || t->live_ents.alloc(ne) != hipSuccess ||
      t->live_paths.alloc(5 * (size_t)path_cap * ne) != hipSuccess || t->live_phases.alloc(6 * (size_t)phase_cap * ne) != hipSuccess ||
      t->live_view.alloc(6 * (size_t)phase_cap * n) != hipSuccess) {
    live_free(t);
    (void)hipGetLastError();
    set_error("vbt_tracker_live_enable: hipMalloc of the live tables failed (%d clips, path_cap %d, phase_cap %d)", t->n_clips, path_cap, phase_cap);
    return VBT_ERR_HIP;
  }
  t->lb = LiveBufs{t->live_clips.get(), t->live_ents.get(), t->live_paths.get(), t->live_phases.get(), t->live_view.get()};
  t->lc.p = VtParams{plate_diameter, diff_threshold, min_distance, 1, 0};
  t->lc.path_cap = path_cap;
  t->lc.phase_cap = phase_cap;
  t->live = true;
  if (!live_metrics_alloc(t)) {
    live_free(t);
    (void)hipGetLastError();
    set_error("vbt_tracker_live_enable: hipMalloc of the live metrics failed (%d clips, phase_cap %d)", t->n_clips, phase_cap);
    return VBT_ERR_HIP;
  }
  live_init(t);
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { live_free(t); set_error("live init failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  t->live = true;
  return VBT_OK;
}

// One pack launch on `stream` (after the tracker launches it carries), ONE copy into pinned memory, ONE synchronisation of that stream.
// metrics8 != nullptr (vbt_tracker_live_poll_ex): the block carries, behind the n_clips records, n_clips x pcap metrics records.
static int live_poll(vbt_tracker* t, int flush_view, vbt_live_clip* clips, double* phases6, double* metrics8, int cap, void* stream) {
  static_assert(sizeof(vbt_live_clip) == 32, "vbt_live_clip record");
  VBT_HIP_CHECK(hipSetDevice(t->device));
  const int n = t->n_clips;
  const int pcap = std::min(cap, t->lc.phase_cap);   // a clip never reports more than phase_cap phases
  const size_t rec = 32 + (size_t)pcap * 48, mrec = (size_t)pcap * VT_METRICS * sizeof(double);
  const size_t bytes = rec * n + (metrics8 ? mrec * n : 0);
  VBT_HIP_CHECK(t->live_poll.reserve(bytes));
  hipStream_t st = (hipStream_t)stream;
  if (metrics8) live_pack_kernel<true><<<n, 64, 0, st>>>(t->lb, t->lc, flush_view, pcap, t->live_poll.dev(), (double*)(t->live_poll.dev() + rec * n));
  else live_pack_kernel<false><<<n, 64, 0, st>>>(t->lb, t->lc, flush_view, pcap, t->live_poll.dev(), nullptr);
  VBT_HIP_CHECK(hipGetLastError());
  VBT_HIP_CHECK(t->live_poll.fetch(bytes, st));
  for (int c = 0; c < n; c++) {
    const unsigned char* r = t->live_poll.host() + c * rec;
    memcpy(&clips[c], r, sizeof(vbt_live_clip));
    if (int rc = unpack_phases("clip", c, r + 32, clips[c].n_phases, phases6, (size_t)c, cap)) return rc;
    if (metrics8) unpack_metrics(t->live_poll.host() + rec * n + c * mrec, clips[c].n_phases, metrics8, (size_t)c, cap);
  }
  return VBT_OK;
}

int vbt_tracker_live_poll(vbt_tracker* t, int flush_view, vbt_live_clip* clips, double* phases6, int cap, void* stream) {
  if (!t || !clips || cap < 0 || (cap > 0 && !phases6)) { set_error("vbt_tracker_live_poll: bad argument"); return VBT_ERR_ARG; }
  if (!t->live) { set_error("vbt_tracker_live_poll: live analysis is not enabled"); return VBT_ERR_STATE; }
  return live_poll(t, flush_view, clips, phases6, nullptr, cap, stream);
}

int vbt_tracker_live_poll_ex(vbt_tracker* t, int flush_view, vbt_live_clip* clips, double* phases6, double* metrics8, int cap, void* stream) {
  if (!t || !clips || cap < 0 || (cap > 0 && (!phases6 || !metrics8))) { set_error("vbt_tracker_live_poll_ex: bad argument"); return VBT_ERR_ARG; }
  if (!t->live) { set_error("vbt_tracker_live_poll_ex: live analysis is not enabled"); return VBT_ERR_STATE; }
  if (!t->rep_metrics) { set_error("vbt_tracker_live_poll_ex: rep metrics are not enabled (vbt_tracker_rep_metrics_enable)"); return VBT_ERR_STATE; }
  return live_poll(t, flush_view, clips, phases6, cap > 0 ? metrics8 : nullptr, cap, stream);
}

int vbt_tracker_live_tracks(vbt_tracker* t, int clip, int flush_view, int64_t* ids, int32_t* n_rows, int32_t* n_phases, int32_t* flags,
                            double* phases6, int cap_tracks, int cap_phases, int* n) {
  if (!t || !ids || !n_rows || !n_phases || !flags || !phases6 || !n || clip < 0 || clip >= t->n_clips || cap_tracks < 1 || cap_phases < 1) {
    set_error("vbt_tracker_live_tracks: bad argument");
    return VBT_ERR_ARG;
  }
  if (!t->live) { set_error("vbt_tracker_live_tracks: live analysis is not enabled"); return VBT_ERR_STATE; }
  VBT_HIP_CHECK(hipSetDevice(t->device));
  VBT_HIP_CHECK(hipDeviceSynchronize());
  const size_t rec = 24 + (size_t)t->lc.phase_cap * 48, bytes = rec * LIVE_ENTRIES;
  std::vector<unsigned char> h(bytes);
  {
    DevBuf<unsigned char> d;   // freed right after the blocking copy, or on the way out
    VBT_HIP_CHECK(d.alloc(bytes));
    live_tracks_kernel<<<LIVE_ENTRIES, 64>>>(t->lb, t->lc, clip, flush_view, d.get());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(h.data(), d.get(), bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error("live tracks kernel failed: %s", hipGetErrorString(e)); return VBT_ERR_HIP; }
  }
  int m = 0;
  for (int k = 0; k < LIVE_ENTRIES; k++) {
    const unsigned char* r = h.data() + k * rec;
    const long long id = *(const long long*)r;
    const int* hd = (const int*)(r + 8);
    if (id < 0 || hd[0] == 0) continue;   // free, or no row of the id yet
    if (m >= cap_tracks) { set_error("clip %d holds more than %d live tracks", clip, cap_tracks); return VBT_ERR_CAPACITY; }
    if (int rc = unpack_phases("id", id, r + 24, hd[1], phases6, (size_t)m, cap_phases)) return rc;
    ids[m] = id; n_rows[m] = hd[0]; n_phases[m] = hd[1]; flags[m] = hd[2];
    m++;
  }
  *n = m;
  return VBT_OK;
}

}  // extern "C"
