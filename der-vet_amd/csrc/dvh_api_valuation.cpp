// dvh_api_valuation.cpp -- the scenario valuation's entry points (dvh_valuation.hip): dvh_bill_windows,
// dvh_value_scenarios, dvh_last_valuation_ms.  Both calls validate on the host (dvh_valuation_validate.h), then launch
// one kernel between two of the handle's timing events (dvh_handle.h val_ev, created by a call's first run) on the
// caller's stream: no wait, no device allocation.
#include "dvh_handle.h"
#include "dvh_valuation.h"
#include "dvh_valuation_validate.h"

namespace {

// launch() between the events of call `which` on stream s
template <class F>
int timed_launch(dvh_handle* h, int which, hipStream_t s, const char* name, F launch) {
  DevEvent* ev = h->val_ev[which];
  DVH_HIP(h, hipSetDevice(h->device));
  DVH_HIP(h, ev[0].ensure());
  DVH_HIP(h, ev[1].ensure());
  DVH_HIP(h, hipEventRecord(ev[0], s));
  hipError_t e = launch();
  if (e != hipSuccess) return hip_fail(h, e, name);
  DVH_HIP(h, hipEventRecord(ev[1], s));
  h->val_ran[which] = true;
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
  dvh_handle* hm = const_cast<dvh_handle*>(h);
  for (int k = 0; k < 2; ++k) {
    if (!h->val_ran[k]) continue;
    float ms = 0.0f;
    DVH_HIP(hm, hipEventSynchronize(h->val_ev[k][1]));
    DVH_HIP(hm, hipEventElapsedTime(&ms, h->val_ev[k][0], h->val_ev[k][1]));
    ms2[k] = ms;
  }
  return DVH_OK;
}
