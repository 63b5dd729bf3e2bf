// Validation of the valuation entry points' arguments (dvh_bill_windows, dvh_value_scenarios; include/dervet_hip.h)
// before anything is launched.  Only what the host can see: counts, sizes, null pointers, the batch's totals, the
// host arrays (opt years, the CSR row pointers' host copy) -- the descriptors, the demand-charge rows and the CSR
// entries are device memory and are checked by the kernels.  Plain C++ with no HIP dependency:
// tests/native/cba_sanitize.cpp runs it under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/dervet_hip.h"

namespace dvh {

// "" when valid, else the message dvh_last_error reports (DVH_ERR_ARG); J above DVH_BILL_MAX_J is not an argument
// error but DVH_ERR_UNSUPPORTED, which the entry point reports after this passes.
inline std::string validate_bill_windows(const dvh_bill_group* g, const dvh_packed* b, int32_t first,
                                         const void* bills, const void* bad) {
  if (!g || !b) return "bill: null group or batch";
  if (g->G < 0 || g->T < 1 || g->J < 0 || g->mI < 0 || first < 0)
    return "bill: count out of range (G = " + std::to_string(g->G) + ", T = " + std::to_string(g->T) + ", J = " +
           std::to_string(g->J) + ", mI = " + std::to_string(g->mI) + ", first = " + std::to_string(first) + ")";
  if ((int64_t)first + g->G > b->count)
    return "bill: windows " + std::to_string(first) + " .. " + std::to_string((int64_t)first + g->G - 1) +
           " outside the batch of " + std::to_string(b->count);
  if (!std::isfinite(g->dt) || !(g->dt > 0.0)) return "bill: dt must be positive and finite";
  if (g->G == 0) return "";
  if (!bills || !bad) return "bill: null output array";
  if (!b->desc || !b->x || !b->istats) return "bill: null device array in packed batch";
  if (!g->base) return "bill: null base series";
  if (g->mI > 0 && (!g->dcm_t || !g->dcm_j)) return "bill: null demand-charge rows";
  if (g->J > 0 && !g->demand) return "bill: null demand prices";
  if (g->has_ice && !g->ice_cost) return "bill: null ICE cost";
  if (g->has_ev && (g->has_pv || g->has_ice)) return "bill: an EV block is not combined with has_pv / has_ice";
  return "";
}

inline std::string validate_value_scenarios(const dvh_valuation* v, const void* values, const void* valid) {
  if (!v) return "valuation: null arguments";
  if (v->S < 0) return "valuation: negative scenario count";
  if (v->Y < 1 || v->Y > DVH_CBA_MAX_YEARS)
    return "valuation: Y = " + std::to_string(v->Y) + " years (1 .. " + std::to_string(DVH_CBA_MAX_YEARS) + ")";
  if (v->n_extra < 0 || v->n_extra > DVH_CBA_MAX_EXTRA)
    return "valuation: " + std::to_string(v->n_extra) + " extra columns (0 .. " + std::to_string(DVH_CBA_MAX_EXTRA) + ")";
  if (v->n_opt < 1 || v->n_opt > v->Y || !v->opt_years)
    return "valuation: " + std::to_string(v->n_opt) + " opt years (1 .. Y, not null)";
  for (int o = 0; o < v->n_opt; ++o) {
    if (v->opt_years[o] < 0 || v->opt_years[o] >= v->Y)
      return "valuation: opt year index " + std::to_string(v->opt_years[o]) + " outside 0 .. Y - 1";
    if (o > 0 && v->opt_years[o] <= v->opt_years[o - 1]) return "valuation: opt years not ascending";
  }
  if (!(v->rate > -1.0) || !std::isfinite(v->rate)) return "valuation: rate must be finite and above -1";
  for (int b = 0; b < 5; ++b)
    if (!std::isfinite(v->growth[b]) || !(v->growth[b] > -100.0)) return "valuation: growth must be finite and above -100 %";
  if (v->n_win < 0 || v->n_bills < 0) return "valuation: negative window count";
  if (!v->win_ptr_host) return "valuation: null win_ptr_host";
  if (v->win_ptr_host[0] != 0) return "valuation: win_ptr does not start at 0";
  for (int s = 0; s < v->S; ++s)
    if (v->win_ptr_host[s + 1] < v->win_ptr_host[s]) return "valuation: win_ptr not monotone at scenario " + std::to_string(s);
  if (v->win_ptr_host[v->S] != v->n_win)
    return "valuation: win_ptr ends at " + std::to_string(v->win_ptr_host[v->S]) + ", not at len(win_idx) = " +
           std::to_string(v->n_win);
  if (v->S == 0) return "";
  if (!values || !valid) return "valuation: null output array";
  if (!v->win_ptr || !v->capex || !v->fixed_om) return "valuation: null device array";
  if (v->n_win > 0 && (!v->win_idx || !v->win_year || !v->bills)) return "valuation: null window arrays";
  if (v->n_extra > 0 && !v->extra) return "valuation: null extra columns";
  return "";
}

}  // namespace dvh
