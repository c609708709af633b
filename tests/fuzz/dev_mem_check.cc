// Host-only check of the memory owners of vbt_amd/csrc/dev_mem.h and the event / stream owners of vbt_amd/csrc/hip_handles.h, built with
// -fsanitize=address,undefined (tests/test_dev_mem_host.py).
// It needs no device: the test hides every device, so each allocation fails the way it does on a machine without one, and an
// allocation of 2^60 bytes fails on any machine.  What is checked is the owners' bookkeeping around failures, moves and destruction;
// where an allocation does succeed (a visible device) the same statements hold with a buffer in hand.  Events and streams likewise:
// no create succeeds without a device, and one with flags no runtime knows fails on any machine.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../vbt_amd/csrc/dev_mem.h"
#include "../../vbt_amd/csrc/hip_handles.h"

using namespace vbt;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <class Buf>
static int check_buf(const char* name) {
  constexpr size_t HUGE_COUNT = (size_t)1 << 57;   // x 8 bytes
  {
    Buf empty;                                      // destruction of an empty buffer
    CHECK(!empty && empty.get() == nullptr);
  }
  Buf a;
  CHECK(a.alloc(HUGE_COUNT) != hipSuccess);         // a failed alloc leaves the buffer null
  CHECK(!a && a.get() == nullptr);
  const hipError_t e = a.alloc(16);
  CHECK((e == hipSuccess) == (a.get() != nullptr));
  double* const p = a.get();
  Buf b(std::move(a));                              // a move leaves the source empty
  CHECK(a.get() == nullptr && b.get() == p);
  Buf c;
  c = std::move(b);
  CHECK(b.get() == nullptr && c.get() == p);
  Buf& same = c;
  c = std::move(same);                              // self-move keeps the buffer
  CHECK(c.get() == p);
  CHECK(c.alloc(HUGE_COUNT) != hipSuccess);         // a failed re-alloc frees what was held
  CHECK(c.get() == nullptr);
  a.reset();                                        // reset of a moved-from buffer
  std::printf("ok %s %s\n", name, e == hipSuccess ? "allocated" : "no-device");
  return 0;                                         // a, b, c: destruction of moved-from and empty buffers
}

static int check_mirror() {
  Mirror m;
  CHECK(m.bytes() == 0 && m.dev() == nullptr && m.host() == nullptr);
  CHECK(m.reserve((size_t)1 << 60) != hipSuccess);
  CHECK(m.bytes() == 0 && m.dev() == nullptr);      // the device half failed
  const hipError_t e = m.reserve(4096);             // still usable after a failure
  if (e == hipSuccess) {
    CHECK(m.bytes() == 4096 && m.dev() && m.host());
    unsigned char* const d = m.dev();
    CHECK(m.reserve(1024) == hipSuccess && m.dev() == d && m.bytes() == 4096);   // never shrinks
    CHECK(m.fetch(4096, nullptr) == hipSuccess);
  } else {
    CHECK(m.bytes() == 0 && m.dev() == nullptr && m.host() == nullptr);
    CHECK(m.reserve(4096) != hipSuccess && m.bytes() == 0);
  }
  CHECK(m.reserve(0) == hipSuccess);                // nothing to grow
  m.reset();
  CHECK(m.bytes() == 0 && m.dev() == nullptr && m.host() == nullptr);
  Mirror untouched;                                 // destruction of an empty mirror
  std::printf("ok Mirror %s\n", e == hipSuccess ? "allocated" : "no-device");
  return 0;
}

template <class Own>
static int check_handle(const char* name, unsigned flags) {
  {
    Own empty;                                      // destruction of an empty owner
    CHECK(!empty && empty.get() == nullptr);
  }
  Own a;
  CHECK(a.create(~0u) != hipSuccess);               // a failed create leaves the owner empty
  CHECK(!a && a.get() == nullptr);
  const hipError_t e = a.create(flags);
  CHECK((e == hipSuccess) == (a.get() != nullptr));
  const auto h = a.get();
  Own b(std::move(a));                              // a move leaves the source empty
  CHECK(a.get() == nullptr && b.get() == h);
  Own c;
  c = std::move(b);
  CHECK(b.get() == nullptr && c.get() == h);
  Own& same = c;
  c = std::move(same);                              // self-move keeps the handle
  CHECK(c.get() == h);
  CHECK(c.create(~0u) != hipSuccess);               // a failed re-create destroys what was held
  CHECK(c.get() == nullptr);
  a.reset();                                        // reset of a moved-from owner
  std::printf("ok %s %s\n", name, e == hipSuccess ? "created" : "no-device");
  return 0;                                         // a, b, c: destruction of moved-from and empty owners
}

// PinnedBuf::alloc with explicit flags: the same books as without, and the flags of a record the device writes are taken
static int check_pinned_flags() {
  const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;
  PinnedBuf<double> a, plain;
  CHECK(a.alloc((size_t)1 << 57, flags) != hipSuccess);   // a failed alloc leaves the buffer null
  CHECK(!a && a.get() == nullptr);
  const hipError_t e = a.alloc(16, flags);
  CHECK((e == hipSuccess) == (a.get() != nullptr));
  CHECK(e == plain.alloc(16));                      // the flags are accepted: they change nothing about success or the error
  CHECK(a.alloc((size_t)1 << 57, flags) != hipSuccess);   // a failed re-alloc frees what was held
  CHECK(a.get() == nullptr);
  std::printf("ok PinnedBuf-flags %s\n", e == hipSuccess ? "allocated" : "no-device");
  return 0;
}

// What a handle keeps in a std::vector: events, and a ring slot of one buffer and two events.  resize() default-constructs and, when
// it grows past the capacity, moves every element: each owner must arrive with what it held and leave nothing behind to destroy twice.
struct Slot {
  DevBuf<unsigned char> buf;
  Event free_ev, copy_ev;
  size_t bytes = 0;
};
static int check_vectors() {
  std::vector<Event> evs;
  evs.resize(3);
  hipError_t e = hipSuccess;
  for (Event& ev : evs) {
    const hipError_t ei = ev.create(hipEventDisableTiming);
    CHECK((ei == hipSuccess) == (ev.get() != nullptr));
    if (e == hipSuccess) e = ei;
  }
  const hipEvent_t h0 = evs[0].get(), h2 = evs[2].get();
  evs.resize(evs.capacity() + 6);                   // reallocates: the elements move
  CHECK(evs[0].get() == h0 && evs[2].get() == h2 && !evs[3] && !evs.back());
  std::vector<Event> moved(std::move(evs));
  CHECK(evs.empty() && moved[0].get() == h0);
  moved.resize(1);                                  // destroys the tail, created and empty alike

  std::vector<Slot> ring;
  ring.resize(2);
  for (Slot& s : ring) {
    const hipError_t eb = s.buf.alloc(64);
    if (eb == hipSuccess) s.bytes = 64;
    CHECK((s.bytes == 0) == (s.buf.get() == nullptr));   // the capacity is 0 whenever the buffer is empty
    (void)s.free_ev.create(hipEventDisableTiming);
    (void)s.copy_ev.create(hipEventDisableTiming);
    if (e == hipSuccess) e = eb;
  }
  unsigned char* const b1 = ring[1].buf.get();
  const hipEvent_t f1 = ring[1].free_ev.get(), c1 = ring[1].copy_ev.get();
  ring.resize(ring.capacity() + 5);
  CHECK(ring[1].buf.get() == b1 && ring[1].free_ev.get() == f1 && ring[1].copy_ev.get() == c1);
  CHECK(!ring.back().buf && !ring.back().free_ev && ring.back().bytes == 0);
  std::vector<Slot> ring2;
  ring2 = std::move(ring);
  CHECK(ring.empty() && ring2[1].buf.get() == b1);
  CHECK(ring2[1].buf.alloc((size_t)1 << 60) != hipSuccess && !ring2[1].buf);   // a grow that fails: empty, the events stay
  CHECK(ring2[1].free_ev.get() == f1);
  std::printf("ok vectors %s\n", e == hipSuccess ? "created" : "no-device");
  return 0;                                         // moved, ring2: destruction of what is left
}

int main() {
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  if (check_buf<DevBuf<double>>("DevBuf")) return 1;
  if (check_buf<PinnedBuf<double>>("PinnedBuf")) return 1;
  if (check_mirror()) return 1;
  if (check_handle<Event>("Event", hipEventDisableTiming)) return 1;
  if (check_handle<Stream>("Stream", hipStreamNonBlocking)) return 1;
  if (check_pinned_flags()) return 1;
  return check_vectors();
}
