// dvh_api_valuation.cpp -- the scenario valuation's entry points (dvh_valuation.hip): dvh_bill_windows,
// dvh_value_scenarios, dvh_last_valuation_ms.  Both calls validate on the host (dvh_valuation_validate.h), then launch
// one kernel between two timing events on the caller's stream: no wait, no device allocation.
#include <mutex>
#include <unordered_map>

#include "dvh_handle.h"
#include "dvh_valuation.h"
#include "dvh_valuation_validate.h"

namespace {

// The two calls' timing events, per handle.  Kept beside the handle rather than in it: created by a handle's first
// valuation call on its device and reused by every later one.  dvh_destroy does not know them, so they live until the
// process ends (four events per handle that ever valued); a new handle at a destroyed one's address takes them over,
// re-created when it sits on another device.
struct ValTimers {
  int device = -1;
  hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // {bill, valuation} x {start, stop}
  bool ran[2] = {false, false};
};
std::mutex g_mu;
std::unordered_map<const dvh_handle*, ValTimers> g_timers;

hipError_t timers_for(dvh_handle* h, ValTimers** out) {
  ValTimers& t = g_timers[h];
  if (t.device != h->device) {
    for (auto& pair : t.ev)
      for (hipEvent_t& e : pair) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) {
          t.device = -1;
          return r;
        }
      }
    t.device = h->device;
    t.ran[0] = t.ran[1] = false;
  }
  *out = &t;
  return hipSuccess;
}

// launch() between the events of call `which` on stream s
template <class F>
int timed_launch(dvh_handle* h, int which, hipStream_t s, const char* name, F launch) {
  std::lock_guard<std::mutex> lock(g_mu);
  ValTimers* t = nullptr;
  DVH_HIP(h, hipSetDevice(h->device));
  DVH_HIP(h, timers_for(h, &t));
  DVH_HIP(h, hipEventRecord(t->ev[which][0], s));
  hipError_t e = launch();
  if (e != hipSuccess) return hip_fail(h, e, name);
  DVH_HIP(h, hipEventRecord(t->ev[which][1], s));
  t->ran[which] = true;
  return DVH_OK;
}

}  // namespace

extern "C" int dvh_bill_windows(dvh_handle* h, const dvh_bill_group* group, const dvh_packed* batch, int32_t first,
                                double* bills, double* peaks, int32_t* bad, void* stream) {
  if (!h) return DVH_ERR_ARG;
  const std::string msg = dvh::validate_bill_windows(group, batch, first, bills, bad);
  if (!msg.empty()) return fail(h, DVH_ERR_ARG, msg);
  if (group->J > DVH_BILL_MAX_J)
    return fail(h, DVH_ERR_UNSUPPORTED, "bill: J = " + std::to_string(group->J) + " demand-charge columns (at most " +
                                            std::to_string(DVH_BILL_MAX_J) + ")");
  if (group->G == 0) return DVH_OK;
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  return timed_launch(h, 0, s, "bill_kernel",
                      [&] { return dvh::launch_bill(*group, *batch, first, bills, peaks, bad, s); });
}

extern "C" int dvh_value_scenarios(dvh_handle* h, const dvh_valuation* v, double* values, int32_t* valid,
                                   double* proforma, void* stream) {
  if (!h) return DVH_ERR_ARG;
  const std::string msg = dvh::validate_value_scenarios(v, values, valid);
  if (!msg.empty()) return fail(h, DVH_ERR_ARG, msg);
  if (v->S == 0) return DVH_OK;
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  return timed_launch(h, 1, s, "valuation_kernel",
                      [&] { return dvh::launch_valuation(*v, values, valid, proforma, s); });
}

extern "C" int dvh_last_valuation_ms(const dvh_handle* h, double* ms2) {
  if (!h || !ms2) return DVH_ERR_ARG;
  ms2[0] = ms2[1] = 0.0;
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_timers.find(h);
  if (it == g_timers.end() || it->second.device != h->device) return DVH_OK;
  dvh_handle* hm = const_cast<dvh_handle*>(h);
  for (int k = 0; k < 2; ++k) {
    if (!it->second.ran[k]) continue;
    float ms = 0.0f;
    DVH_HIP(hm, hipEventSynchronize(it->second.ev[k][1]));
    DVH_HIP(hm, hipEventElapsedTime(&ms, it->second.ev[k][0], it->second.ev[k][1]));
    ms2[k] = ms;
  }
  return DVH_OK;
}
