// Validation of the economic-sizing entry points' arguments (dvh_value_cuts, dvh_value_master; include/dervet_hip.h)
// before anything is launched.  Only what the host can see: counts, sizes, null pointers, the batch's totals and the
// host copy of the specs -- descriptors, CSR rows and case ids are device memory and are checked by the kernels.
// Plain C++ with no HIP dependency: tests/native/value_cut_sanitize.cpp runs it under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/dervet_hip.h"

namespace dvh {

// "" when valid, else the message dvh_last_error reports; *code = DVH_ERR_ARG or DVH_ERR_UNSUPPORTED.
inline std::string validate_value_cuts(const dvh_battery_group* g, const dvh_packed* b, int32_t first,
                                       const void* cuts_out, int* code) {
  *code = DVH_ERR_ARG;
  if (!g || !b) return "value cuts: null group or batch";
  if (g->G < 0 || g->T < 1 || g->J < 0 || g->mI < 0 || first < 0)
    return "value cuts: count out of range (G = " + std::to_string(g->G) + ", T = " + std::to_string(g->T) + ", J = " +
           std::to_string(g->J) + ", mI = " + std::to_string(g->mI) + ", first = " + std::to_string(first) + ")";
  if ((int64_t)first + g->G > b->count)
    return "value cuts: windows " + std::to_string(first) + " .. " + std::to_string((int64_t)first + g->G - 1) +
           " outside the batch of " + std::to_string(b->count);
  if (g->has_ice || g->has_ev || g->has_emin || g->J > DVH_VALUE_MAX_J) {
    *code = DVH_ERR_UNSUPPORTED;
    if (g->has_ice) return "value cuts: ICE windows are not sized (has_ice)";
    if (g->has_ev) return "value cuts: EV windows are not sized (has_ev)";
    if (g->has_emin) return "value cuts: a minimum-SOE series is not supported (has_emin)";
    return "value cuts: J = " + std::to_string(g->J) + " demand-charge columns (at most " +
           std::to_string(DVH_VALUE_MAX_J) + ")";
  }
  if (g->G == 0) return "";
  if (!cuts_out) return "value cuts: null output array";
  if (!b->desc || !b->indices || !b->data || !b->c || !b->c0 || !b->q || !b->l || !b->u || !b->x || !b->y || !b->istats)
    return "value cuts: null device array in packed batch";
  if (g->mI > 0 && (!g->dcm_t || !g->dcm_j)) return "value cuts: null demand-charge rows";
  if (!g->E || !g->pch || !g->pdis || !g->soc_target || !g->ulsoc || !g->llsoc) return "value cuts: null rating array";
  if (g->has_emax && !g->emax) return "value cuts: null emax series";
  return "";
}

inline std::string validate_value_spec(const dvh_value_spec& s, int k) {
  const std::string at = "value master: case " + std::to_string(k) + ": ";
  if (!s.size_energy && !s.size_power) return at + "nothing is sized";
  if (!std::isfinite(s.alpha) || !(s.alpha > 0.0)) return at + "alpha must be positive and finite";
  if (!std::isfinite(s.c_fixed)) return at + "c_fixed must be finite";
  if (!std::isfinite(s.gap_tol) || !(s.gap_tol > 0.0)) return at + "gap_tol must be positive and finite";
  if (s.max_rounds < 1 || s.max_rounds > 65536) return at + "max_rounds out of range (1 .. 65536)";
  if (!std::isfinite(s.energy_min) || !std::isfinite(s.power_min)) return at + "a lower bound is not finite";
  if (s.size_energy && !std::isfinite(s.energy_max)) return at + "a sized energy needs a finite energy_max";
  if (s.size_power && !std::isfinite(s.power_max)) return at + "a sized power needs a finite power_max";
  if (!std::isfinite(s.energy_max) || !std::isfinite(s.power_max)) return at + "a fixed rating is not finite";
  if (s.energy_min < 0.0 || s.power_min < 0.0 || s.energy_max < s.energy_min || s.power_max < s.power_min)
    return at + "bounds crossed or negative";
  if (!s.size_energy && s.energy_min != s.energy_max) return at + "a fixed energy needs energy_min = energy_max";
  if (!s.size_power && s.power_min != s.power_max) return at + "a fixed power needs power_min = power_max";
  if (s.size_energy && !(std::isfinite(s.c_energy) && s.c_energy > 0.0)) return at + "a sized energy needs c_energy > 0";
  if (s.size_power && !(std::isfinite(s.c_power) && s.c_power > 0.0)) return at + "a sized power needs c_power > 0";
  if (!std::isfinite(s.c_energy) || !std::isfinite(s.c_power)) return at + "a unit cost is not finite";
  return "";
}

inline std::string validate_value_master(const dvh_value_master_args* a) {
  if (!a) return "value master: null arguments";
  if (a->count < 0 || a->n_cases < 0 || a->count > a->n_cases) return "value master: case count out of range";
  if (a->W < 1) return "value master: W must be at least 1";
  if (a->n_cand < 1 || a->n_cand > DVH_VALUE_MAX_CAND || a->n_next < 1 || a->n_next > DVH_VALUE_MAX_CAND)
    return "value master: candidates per round out of range (1 .. " + std::to_string(DVH_VALUE_MAX_CAND) + ")";
  if (a->cut_cap < a->n_cand || a->cut_cap > DVH_VALUE_MAX_CUTS)
    return "value master: cut capacity out of range (n_cand .. " + std::to_string(DVH_VALUE_MAX_CUTS) + ")";
  if (a->count == 0) return "";
  if (!a->spec_host || !a->spec || !a->case_ids || !a->window_cuts || !a->E_in || !a->P_in || !a->cuts || !a->state ||
      !a->flags || !a->E_out || !a->pch_out || !a->pdis_out)
    return "value master: null array";
  for (int k = 0; k < a->n_cases; ++k) {
    const std::string msg = validate_value_spec(a->spec_host[k], k);
    if (!msg.empty()) return msg;
  }
  return "";
}

}  // namespace dvh
