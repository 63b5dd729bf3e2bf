// Host sanitizer driver of the three owning types of der-vet_amd/csrc/dvh_host.h (DevBuf, DevEvent, PinnedBuf).  Built
// with -fsanitize=address,undefined (tests/test_owner_native.py) and run on the CPU: the six HIP calls the types make
// are counting stand-ins defined here (they take the place of the runtime's), each object they hand out a heap block
// of its own, so a double release or a leak is the sanitizer's to report and the counts must balance.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../der-vet_amd/csrc/dvh_host.h"

static int n_ev_create = 0, n_ev_destroy = 0, n_host_malloc = 0, n_host_free = 0, n_dev_malloc = 0, n_dev_free = 0;
static int fail_next = 0;  // the next create / malloc fails (and writes a stale pointer, which the owner must not keep)
static unsigned last_flags = ~0u;
static size_t last_bytes = 0;
static std::set<void*> live;
static char stale;

static hipError_t make(void** out, int* count, size_t bytes) {
  if (fail_next) {
    --fail_next;
    *out = &stale;
    return hipErrorOutOfMemory;
  }
  *out = std::malloc(bytes ? bytes : 1);
  live.insert(*out);
  ++*count;
  return hipSuccess;
}
static hipError_t drop(void* p, int* count) {
  if (!live.erase(p)) {
    std::printf("FATAL: release of %p, which is not live\n", p);
    std::abort();
  }
  std::free(p);
  ++*count;
  return hipSuccess;
}

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  last_flags = flags;
  return make(reinterpret_cast<void**>(e), &n_ev_create, 8);
}
hipError_t hipEventDestroy(hipEvent_t e) { return drop(e, &n_ev_destroy); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return make(p, &n_host_malloc, bytes); }
hipError_t hipHostFree(void* p) { return drop(p, &n_host_free); }
hipError_t hipMalloc(void** p, size_t bytes) {
  last_bytes = bytes;
  return make(p, &n_dev_malloc, bytes);
}
hipError_t hipFree(void* p) { return drop(p, &n_dev_free); }
}

static int failures = 0;
#define CHECK(name, cond)                                       \
  do {                                                          \
    const bool ok_ = (cond);                                    \
    std::printf("%s %s\n", name, ok_ ? "ok" : "FAILED");        \
    if (!ok_) ++failures;                                       \
  } while (0)

static bool balanced() {
  return live.empty() && n_ev_create == n_ev_destroy && n_host_malloc == n_host_free && n_dev_malloc == n_dev_free;
}

int main() {
  // ---- creates and destroys balance after scopes end; nothing is made before the first ensure()
  {
    DevEvent e, timing_off, arr[4];
    PinnedBuf pin;
    DevBuf buf;
    CHECK("lazy_nothing_made", n_ev_create + n_host_malloc + n_dev_malloc == 0 && !e.e && !pin.p && !buf.p);
    bool ok = e.ensure() == hipSuccess && last_flags == hipEventDefault;
    ok = ok && timing_off.ensure(hipEventDisableTiming) == hipSuccess && last_flags == hipEventDisableTiming;
    for (DevEvent& a : arr) ok = ok && a.ensure() == hipSuccess;
    const hipEvent_t first = e;
    ok = ok && e.ensure() == hipSuccess && first == static_cast<hipEvent_t>(e);  // a second ensure() keeps the event
    ok = ok && pin.ensure(20) == hipSuccess && pin.ensure(20) == hipSuccess && pin.as<int32_t>() != nullptr;
    pin.as<int32_t>()[4] = 7;  // (the sanitizer checks the write against the 20 bytes)
    ok = ok && buf.ensure(100) == hipSuccess;
    CHECK("ensure_creates_once", ok && n_ev_create == 6 && n_host_malloc == 1 && n_dev_malloc == 1);
  }
  CHECK("scope_end_balances", balanced() && n_ev_destroy == 6 && n_host_free == 1 && n_dev_free == 1);

  // ---- a moved-from object releases nothing
  {
    DevEvent a;
    PinnedBuf p;
    a.ensure();
    p.ensure(8);
    const hipEvent_t ea = a;
    void* pa = p.p;
    const int d0 = n_ev_destroy, f0 = n_host_free;
    {
      DevEvent b(std::move(a));
      PinnedBuf q(std::move(p));
      CHECK("move_construct_takes", !a.e && !p.p && static_cast<hipEvent_t>(b) == ea && q.p == pa);
      DevEvent c;
      PinnedBuf r;
      c.ensure();
      r.ensure(8);
      c = std::move(b);  // releases c's own event, takes b's
      r = std::move(q);
      CHECK("move_assign_releases_own_only", n_ev_destroy == d0 + 1 && n_host_free == f0 + 1 && !b.e && !q.p &&
                                                 static_cast<hipEvent_t>(c) == ea && r.p == pa);
      DevEvent& same = c;
      c = std::move(same);  // self-assignment keeps it
      CHECK("self_move_keeps", static_cast<hipEvent_t>(c) == ea && n_ev_destroy == d0 + 1);
    }
    CHECK("moved_to_released_once", n_ev_destroy == d0 + 2 && n_host_free == f0 + 2);
    const int d1 = n_ev_destroy, f1 = n_host_free;
    // a and p (moved from) go out of scope below
    CHECK("moved_from_is_reusable", a.ensure() == hipSuccess && p.ensure(8) == hipSuccess && n_ev_destroy == d1 &&
                                        n_host_free == f1);
  }
  CHECK("moves_balance", balanced());

  // ---- growing a vector of event triples (the handle's chunk-event pool) destroys each event exactly once
  {
    const int c0 = n_ev_create, d0 = n_ev_destroy;
    std::vector<hipEvent_t> seen;
    {
      std::vector<std::array<DevEvent, 3>> pool;
      for (int i = 0; i < 37; ++i) {  // (several reallocations of the vector's storage)
        pool.emplace_back();
        for (DevEvent& e : pool.back()) {
          e.ensure();
          seen.push_back(e);
        }
      }
      bool kept = n_ev_destroy == d0;  // the reallocations moved the events, none was destroyed
      for (size_t i = 0; i < pool.size(); ++i)
        for (int u = 0; u < 3; ++u) kept = kept && static_cast<hipEvent_t>(pool[i][u]) == seen[3 * i + u];
      CHECK("vector_growth_moves", kept && n_ev_create == c0 + 111);
    }
    CHECK("vector_destroys_each_once", balanced() && n_ev_destroy == d0 + 111);
  }

  // ---- a failed create leaves the object empty and reusable
  {
    DevEvent e;
    PinnedBuf p;
    DevBuf b;
    fail_next = 1;
    bool ok = e.ensure() != hipSuccess && !e.e;
    fail_next = 1;
    ok = ok && p.ensure(16) != hipSuccess && !p.p;
    fail_next = 1;
    ok = ok && b.ensure(512) != hipSuccess && !b.p && b.bytes == 0;
    CHECK("failed_create_leaves_empty", ok);
    CHECK("failed_create_is_retried", e.ensure() == hipSuccess && p.ensure(16) == hipSuccess &&
                                          b.ensure(512) == hipSuccess && e.e && p.p && b.p && b.bytes == 512);
  }
  CHECK("failures_balance", balanced());

  // ---- DevBuf::ensure: grow-only, at least 256 bytes, the slack on growth, 0 bytes on an empty buffer
  {
    DevBuf b;
    const int m0 = n_dev_malloc, f0 = n_dev_free;
    CHECK("devbuf_zero_request", b.ensure(0) == hipSuccess && !b.p && n_dev_malloc == m0);
    b.ensure(100);
    void* p1 = b.p;
    CHECK("devbuf_floor_256", b.bytes == 256 && last_bytes == 256 && n_dev_malloc == m0 + 1);
    CHECK("devbuf_keeps_when_it_fits", b.ensure(256) == hipSuccess && b.ensure(1) == hipSuccess && b.p == p1 &&
                                           n_dev_malloc == m0 + 1);
    b.ensure(1000);
    CHECK("devbuf_grows_exactly", b.bytes == 1000 && n_dev_malloc == m0 + 2 && n_dev_free == f0 + 1);
    b.ensure(999);
    CHECK("devbuf_never_shrinks", b.bytes == 1000 && n_dev_malloc == m0 + 2);
    DevBuf s;
    s.slack_div = 4;
    s.ensure(1000);
    CHECK("devbuf_slack", s.bytes == 1250 && last_bytes == 1250);
    s.ensure(1250);
    s.ensure(1251);
    CHECK("devbuf_slack_on_growth_only", s.bytes == 1251 + 1251 / 4 && n_dev_malloc == m0 + 4);
    s.release();
    CHECK("devbuf_release_empties", !s.p && s.bytes == 0 && s.ensure(10) == hipSuccess && s.bytes == 256);
  }
  CHECK("devbuf_balances", balanced());

  std::printf("failures=%d\n%s\n", failures, failures ? "FAILED" : "done");
  return failures ? 1 : 0;
}
