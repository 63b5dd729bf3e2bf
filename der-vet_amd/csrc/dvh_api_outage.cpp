// dvh_api_outage.cpp -- the post-facto reliability sweep's entry points (dvh_outage.hip).
#include <cmath>

#include "dvh_handle.h"

// Validates the outage cases and moves them to the device (o_data / o_cases); olen[k] = simulated outage steps
// (int(max_outage / dt), or int(target_hours[k] / dt) for the min-SOE mode).
struct OutagePack {
  std::vector<int> olen;
  size_t nlen = 0, nhist = 0;
  int max_n = 0, max_bins = 0;
};
static int outage_pack(dvh_handle* h, const dvh_outage_case* cases, int32_t count, const int32_t* target_hours,
                       OutagePack& P) {
  hipSetDevice(h->device);
  std::vector<int>& olen = P.olen;
  size_t &nlen = P.nlen, &nhist = P.nhist;
  olen.assign(count, 0);
  for (int k = 0; k < count; ++k) {
    const dvh_outage_case& c = cases[k];
    const std::string w = "outage case " + std::to_string(k) + ": ";
    if (c.n_steps < 1 || !c.critical_load) return fail(h, DVH_ERR_ARG, w + "n_steps >= 1 and critical_load required");
    if (!(c.dt > 0.0) || c.max_outage < 1 || c.max_outage / c.dt < 1.0)
      return fail(h, DVH_ERR_ARG, w + "dt > 0 and max_outage >= dt required");
    if (!(c.rte > 0.0)) return fail(h, DVH_ERR_ARG, w + "rte must be > 0");
    olen[k] = (int)(c.max_outage / c.dt);  // int(self.max_outage_duration / self.dt), Reliability.py:917
    if (target_hours) {  // outage_len = self.outage_duration / self.dt (min_soe_iterative, :712)
      if (target_hours[k] < 1 || target_hours[k] / c.dt < 1.0)
        return fail(h, DVH_ERR_ARG, w + "target outage hours must be >= dt");
      olen[k] = (int)(target_hours[k] / c.dt);
    }
    if (olen[k] + 1 > 16384) return fail(h, DVH_ERR_UNSUPPORTED, w + "more than 16384 outage steps");
    nlen += (size_t)c.n_steps;
    nhist += (size_t)olen[k] + 1;
    P.max_n = std::max(P.max_n, c.n_steps);
    P.max_bins = std::max(P.max_bins, olen[k] + 1);
  }
  std::vector<double> data = dvh::outage_stage(cases, count, true);
  std::vector<dvh::OutageCase> dc(count);
  DVH_HIP(h, h->o_data.ensure(sizeof(double) * data.size()));
  DVH_HIP(h, h->o_cases.ensure(sizeof(dvh::OutageCase) * count));
  DVH_HIP(h, h->o_len.ensure(sizeof(int32_t) * nlen));
  DVH_HIP(h, h->o_hist.ensure(sizeof(int32_t) * nhist));
  dvh::outage_stage_fill(cases, count, true, data, h->o_data.as<double>(), dc.data());
  size_t lo = 0, ho = 0;
  for (int k = 0; k < count; ++k) {
    dc[k].outage_len = olen[k];
    dc[k].len_off = (int64_t)lo;
    dc[k].hist_off = (int64_t)ho;
    lo += cases[k].n_steps;
    ho += olen[k] + 1;
  }
  hipStream_t s = h->stream;
  DVH_HIP(h, hipMemcpyAsync(h->o_data.p, data.data(), sizeof(double) * data.size(), hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipMemcpyAsync(h->o_cases.p, dc.data(), sizeof(dvh::OutageCase) * count, hipMemcpyHostToDevice, s));
  DVH_HIP(h, hipStreamSynchronize(s));  // the host staging vectors end here
  return DVH_OK;
}

extern "C" {

int dvh_outage_coverage(dvh_handle* h, const dvh_outage_case* cases, int32_t count, int32_t* lengths,
                        double* lcp) {
  if (!h) return DVH_ERR_ARG;
  if (count < 0 || (count > 0 && (!cases || !lcp))) return fail(h, DVH_ERR_ARG, "cases and lcp are required");
  if (count == 0) return DVH_OK;
  OutagePack P;
  if (int rc = outage_pack(h, cases, count, nullptr, P)) return rc;
  const std::vector<int>& olen = P.olen;
  const size_t nlen = P.nlen, nhist = P.nhist;
  hipStream_t s = h->stream;
  DVH_HIP(h, hipMemsetAsync(h->o_hist.p, 0, sizeof(int32_t) * nhist, s));
  DVH_HIP(h, hipEventRecord(h->ev[0], s));
  hipError_t e = dvh::launch_outage(h->o_cases.as<dvh::OutageCase>(), count, P.max_n, P.max_bins,
                                    lengths ? h->o_len.as<int32_t>() : nullptr, h->o_hist.as<int32_t>(), s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_outage");
  DVH_HIP(h, hipEventRecord(h->ev[3], s));
  std::vector<int32_t> hist(nhist);
  DVH_HIP(h, hipMemcpyAsync(hist.data(), h->o_hist.p, sizeof(int32_t) * nhist, hipMemcpyDeviceToHost, s));
  if (lengths) DVH_HIP(h, hipMemcpyAsync(lengths, h->o_len.p, sizeof(int32_t) * nlen, hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, h->ev[0], h->ev[3]) == hipSuccess) h->outage_ms = ms;
  // the curve, in the reference's float64 arithmetic (Reliability.py:947-957)
  size_t po = 0, ho = 0;
  for (int k = 0; k < count; ++k) {
    const dvh_outage_case& c = cases[k];
    double length = c.dt;
    int j = 0;
    while (length <= (double)c.max_outage && j < olen[k]) {
      const int first = (int)(length / c.dt);
      double covered = 0.0;
      for (int b = first; b <= olen[k]; ++b) covered += (double)hist[ho + b];
      const double total = (double)c.n_steps - (length / c.dt) + 1.0;
      lcp[po + j] = covered / total;
      ++j;
      length += c.dt;
    }
    for (; j < olen[k]; ++j) lcp[po + j] = NAN;
    po += olen[k];
    ho += olen[k] + 1;
  }
  return DVH_OK;
}

int dvh_outage_min_soe(dvh_handle* h, const dvh_outage_case* cases, int32_t count, const int32_t* target_hours,
                       double* min_soe) {
  if (!h) return DVH_ERR_ARG;
  if (count < 0 || (count > 0 && (!cases || !target_hours || !min_soe)))
    return fail(h, DVH_ERR_ARG, "cases, target_hours and min_soe are required");
  if (count == 0) return DVH_OK;
  OutagePack P;
  if (int rc = outage_pack(h, cases, count, target_hours, P)) return rc;
  hipStream_t s = h->stream;
  DVH_HIP(h, h->o_soe.ensure(sizeof(double) * P.nlen));
  DVH_HIP(h, hipEventRecord(h->ev[0], s));
  hipError_t e = dvh::launch_outage_min_soe(h->o_cases.as<dvh::OutageCase>(), count, P.max_n, h->o_soe.as<double>(), s);
  if (e != hipSuccess) return hip_fail(h, e, "launch_outage_min_soe");
  DVH_HIP(h, hipEventRecord(h->ev[3], s));
  DVH_HIP(h, hipMemcpyAsync(min_soe, h->o_soe.p, sizeof(double) * P.nlen, hipMemcpyDeviceToHost, s));
  DVH_HIP(h, hipStreamSynchronize(s));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, h->ev[0], h->ev[3]) == hipSuccess) h->outage_ms = ms;
  return DVH_OK;
}

int dvh_last_outage_ms(const dvh_handle* h, double* ms) {
  if (!h || !ms) return DVH_ERR_ARG;
  *ms = h->outage_ms;
  return DVH_OK;
}

}  // extern "C"
