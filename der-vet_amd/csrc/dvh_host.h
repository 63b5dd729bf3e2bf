// dvh_host.h -- what the host units share that needs no handle: the owners of a device buffer, an event and a pinned
// host buffer, and the outage staging.  Apart from dvh_handle.h so that dvh_sizing.cpp, which reaches the handle through
// dvh::HandleView, builds into the sanitizer driver beside that driver's stand-in handle
// (tests/native/sizing_sanitize.cpp); dvh_large.hip includes it for its solver's host state.  Host only, header only
// (tests/native/owner_sanitize.cpp drives the three owners against counting stand-ins of the HIP calls they make).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dervet_hip.h"
#include "dvh_internal.h"

// Grow-only device buffer, freed with its owner.  slack_div: a growth asks for want / slack_div bytes more (0: exactly
// what is asked; the sizing state's buffers take 4, their LPs grow by one window per round).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  size_t slack_div = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t want) {
    if (want <= bytes) return hipSuccess;
    release();
    want = std::max<size_t>(want + (slack_div ? want / slack_div : 0), 256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) bytes = want;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// Event, created by the first ensure() on the current device (flags: hipEventDisableTiming for one that only orders)
// and destroyed with its owner.  Move-only, so that arrays of them may sit in a std::vector (the handle's chunk-event
// pool); a failed ensure() leaves it empty.
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept {
    if (this != &o) {
      release();
      e = o.e;
      o.e = nullptr;
    }
    return *this;
  }
  ~DevEvent() { release(); }
  hipError_t ensure(unsigned flags = hipEventDefault) {
    if (e) return hipSuccess;
    hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r != hipSuccess) e = nullptr;
    return r;
  }
  void release() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  operator hipEvent_t() const { return e; }
};

// Pinned host words, the landing place of a small read-back: allocated by the first ensure(), whose size they keep,
// and freed with their owner.  Move-only; a failed ensure() leaves it empty.
struct PinnedBuf {
  void* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~PinnedBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (p) return hipSuccess;
    hipError_t r = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (r != hipSuccess) p = nullptr;
    return r;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

namespace dvh {

// Host staging of the outage cases' series (outage_pack, dvh_api_outage.cpp; upload_series, dvh_sizing.cpp): a case's
// critical_load, pv_max, pv_vari, init_soe (with_init) and load_shed_pct one after the other, the absent ones skipped.
inline std::vector<double> outage_stage(const dvh_outage_case* cases, int count, bool with_init) {
  size_t nd = 0;
  for (int k = 0; k < count; ++k) {
    const dvh_outage_case& c = cases[k];
    nd += (size_t)c.n_steps * (1 + (c.pv_max ? 1 : 0) + (c.pv_vari ? 1 : 0) + (with_init && c.init_soe ? 1 : 0)) +
          (c.load_shed_pct ? (size_t)c.max_outage : 0);
  }
  return std::vector<double>(std::max<size_t>(nd, 1));
}
// Copies the series into `data` (of outage_stage) and fills oc[k]'s common fields, its pointers into the device copy
// at dbase; outage_len, the output offsets (left 0) and what differs are the caller's.
inline void outage_stage_fill(const dvh_outage_case* cases, int count, bool with_init, std::vector<double>& data,
                              const double* dbase, OutageCase* oc) {
  size_t off = 0;
  auto put = [&](const double* src, size_t n) -> const double* {
    if (!src) return nullptr;
    std::memcpy(&data[off], src, sizeof(double) * n);
    const double* d = dbase + off;
    off += n;
    return d;
  };
  for (int k = 0; k < count; ++k) {
    const dvh_outage_case& c = cases[k];
    OutageCase& o = oc[k] = OutageCase{};
    o.n_steps = c.n_steps;
    o.max_steps = c.max_outage;
    o.dt = c.dt;
    o.soe0 = c.soe0;
    o.dg_gen = c.dg_gen;
    o.gamma = c.gamma;
    o.soe_min = c.soe_min;
    o.soe_max = c.soe_max;
    o.charge_max = c.charge_max;
    o.discharge_max = c.discharge_max;
    o.rte = c.rte;
    o.critical_load = put(c.critical_load, c.n_steps);
    o.pv_max = put(c.pv_max, c.n_steps);
    o.pv_vari = put(c.pv_vari, c.n_steps);
    o.init_soe = with_init ? put(c.init_soe, c.n_steps) : nullptr;
    o.load_shed = put(c.load_shed_pct, c.max_outage);
  }
}

}  // namespace dvh
