// dvh_sizing_validate.cpp -- see dvh_sizing_validate.h.
#include "dvh_sizing_validate.h"

#include <cmath>

namespace dvh {

static std::string at(const char* what, int k) { return std::string(what) + " " + std::to_string(k) + ": "; }

std::string validate_outage_case(const dvh_outage_case& c, int k) {
  const std::string w = at("outage case", k);
  if (c.n_steps < 1 || !c.critical_load) return w + "n_steps >= 1 and critical_load required";
  if (!(c.dt > 0.0) || !std::isfinite(c.dt) || c.max_outage < 1 || c.max_outage / c.dt < 1.0)
    return w + "dt > 0 and max_outage >= dt required";
  if (!(c.rte > 0.0) || !std::isfinite(c.rte)) return w + "rte must be > 0";
  if (!std::isfinite(c.dg_gen)) return w + "dg_gen must be finite";
  return "";
}

std::string validate_scan(const dvh_outage_case* cases, int32_t count, const int32_t* target_steps) {
  if (count < 0 || (count > 0 && (!cases || !target_steps))) return "cases and target_steps are required";
  for (int k = 0; k < count; ++k) {
    std::string m = validate_outage_case(cases[k], k);
    if (!m.empty()) return m;
    if (target_steps[k] < 1 || target_steps[k] > cases[k].max_outage)
      return at("outage case", k) + "target_steps must be in 1 .. max_outage";
  }
  return "";
}

int sizing_steps(const dvh_outage_case& c, const dvh_sizing_spec& s) {
  if (!(s.target_hours > 0.0) || !std::isfinite(s.target_hours) || !(c.dt > 0.0)) return 0;
  const double r = std::nearbyint(s.target_hours / c.dt);  // round half to even, as Python's round
  if (!(r >= 1.0) || r > 1e9) return 0;
  return (int)r;
}

bool sizing_lp_fits(int64_t K, int64_t L) { return K >= 1 && L >= 1 && K <= INT32_MAX / 14 / L; }

std::string validate_sizing(const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count) {
  if (count < 0 || (count > 0 && (!cases || !specs))) return "cases and specs are required";
  for (int k = 0; k < count; ++k) {
    std::string m = validate_outage_case(cases[k], k);
    if (!m.empty()) return m;
    const dvh_outage_case& c = cases[k];
    const dvh_sizing_spec& s = specs[k];
    const std::string w = at("sizing spec", k);
    for (int t = 0; t < c.n_steps; ++t)  // (the seeds are an ordering of the load's rolling sums)
      if (!std::isfinite(c.critical_load[t])) return at("outage case", k) + "critical_load must be finite";
    const int L = sizing_steps(c, s);
    if (L < 1) return w + "target_hours must cover at least one step";
    if (L > c.max_outage) return w + "target outage steps exceed max_outage (the simulation's data window)";
    if (!s.size_energy && !s.size_power) return w + "nothing to size: size_energy or size_power must be set";
    if (!std::isfinite(s.ccost) || !std::isfinite(s.ccost_kw) || !std::isfinite(s.ccost_kwh))
      return w + "costs must be finite";
    if (s.size_energy && !(s.ccost_kwh > 0.0)) return w + "sizing energy needs ccost_kwh > 0";
    if (s.size_power && !(s.ccost_kw > 0.0)) return w + "sizing power needs ccost_kw > 0";
    if (s.size_energy && (!(s.energy_min >= 0.0) || !std::isfinite(s.energy_min) || !(s.energy_max >= s.energy_min)))
      return w + "0 <= energy_min <= energy_max required";
    if (s.size_power && (!(s.power_min >= 0.0) || !std::isfinite(s.power_min) || !(s.power_max >= s.power_min)))
      return w + "0 <= power_min <= power_max required";
    if (!s.size_energy && (!(s.energy >= 0.0) || !std::isfinite(s.energy))) return w + "fixed energy rating must be >= 0";
    if (!s.size_power && (!(s.power >= 0.0) || !std::isfinite(s.power))) return w + "fixed power rating must be >= 0";
    if (!(s.llsoc >= 0.0) || !(s.ulsoc >= s.llsoc) || !std::isfinite(s.ulsoc) || !(s.soc_init >= 0.0) ||
        !std::isfinite(s.soc_init))
      return w + "0 <= llsoc <= ulsoc and soc_init >= 0 required";
    if (s.n_seed < 1 || s.max_rounds < 1 || s.max_rounds > 65536 || s.n_seed > 65536)
      return w + "n_seed and max_rounds must be in 1 .. 65536";
    if (!sizing_lp_fits((int64_t)s.n_seed + s.max_rounds, L)) return w + "the sizing LP would exceed 2^31 nonzeros";
  }
  return "";
}

std::string validate_starts(const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count,
                            const int32_t* starts, const int32_t* n_starts) {
  if (count > 0 && (!starts || !n_starts)) return "starts and n_starts are required";
  int64_t off = 0;
  for (int k = 0; k < count; ++k) {
    const std::string w = at("sizing case", k);
    if (n_starts[k] < 1) return w + "at least one outage start required";
    if (!sizing_lp_fits(n_starts[k], sizing_steps(cases[k], specs[k])))
      return w + "the sizing LP would exceed 2^31 nonzeros";
    for (int i = 0; i < n_starts[k]; ++i)
      if (starts[off + i] < 0 || starts[off + i] >= cases[k].n_steps)
        return w + "start " + std::to_string(starts[off + i]) + " outside the series";
    off += n_starts[k];
  }
  return "";
}

}  // namespace dvh
