// dvh_host.h -- what the host units share that needs no handle: the device buffer and the outage staging.  Apart from
// dvh_handle.h so that dvh_sizing.cpp, which reaches the handle through dvh::HandleView, builds into the sanitizer
// driver beside that driver's stand-in handle (tests/native/sizing_sanitize.cpp).  Host only, header only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dervet_hip.h"
#include "dvh_internal.h"

// Grow-only device buffer, freed with its owner.  slack_div: a growth asks for want / slack_div bytes more (0: exactly
// what is asked; the sizing state's buffers take 4, their LPs grow by one window per round).  (dvh_large.hip keeps a
// copy of its own, `Buf`.)
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
