// Validation of the degradation entry points' arguments (dvh_cycle_damage, dvh_degradation_update;
// include/dervet_hip.h) before anything is launched.  Only what the host can see: counts, sizes, null pointers and
// the batch's totals -- the descriptors are device memory and are checked by the kernel.  Plain C++ with no HIP
// dependency: tests/native/rainflow_sanitize.cpp runs it under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/dervet_hip.h"

namespace dvh {

// LDS of one profile: T values and one spare slot (8 (T + 1) bytes); the table's 1 KiB is the rest of the 160 KiB
constexpr int kRainflowMaxT = DVH_RAINFLOW_MAX_T;
static_assert(8 * ((int64_t)kRainflowMaxT + 1) + 16 * DVH_RAINFLOW_MAX_TABLE <= 160 * 1024, "one profile per workgroup");

// "" when valid, else the message dvh_last_error reports (DVH_ERR_ARG)
inline std::string validate_table(const void* upper, const void* life, int32_t n_table) {
  if (!upper || !life) return "null cycle-life table";
  if (n_table < 1 || n_table > DVH_RAINFLOW_MAX_TABLE)
    return "cycle-life table of " + std::to_string(n_table) + " rows (1 .. " + std::to_string(DVH_RAINFLOW_MAX_TABLE) +
           ")";
  return "";
}

inline std::string validate_cycle_damage(const void* ene, int64_t row_stride, int32_t S, int32_t T,
                                         const void* e_rated, const void* upper, const void* life, int32_t n_table,
                                         const void* damage_out) {
  if (S < 0 || T < 0) return "cycle damage: negative count (S = " + std::to_string(S) + ", T = " + std::to_string(T) + ")";
  if (row_stride < T) return "cycle damage: row_stride " + std::to_string(row_stride) + " below T = " + std::to_string(T);
  if (S > 0 && (!e_rated || !damage_out || (T > 0 && !ene))) return "cycle damage: null array";
  return validate_table(upper, life, n_table);
}

inline std::string validate_degradation_update(const dvh_packed* b, int32_t first, int32_t S, int32_t T,
                                               int32_t ene_col, double days, double eol, const void* upper,
                                               const void* life, int32_t n_table, const dvh_degradation_state* st) {
  if (!b || !st) return "degradation update: null batch or state";
  if (S < 0 || T < 0 || ene_col < 0 || first < 0)
    return "degradation update: negative count, column or window (first = " + std::to_string(first) + ", S = " +
           std::to_string(S) + ", T = " + std::to_string(T) + ", ene_col = " + std::to_string(ene_col) + ")";
  if ((int64_t)first + S > b->count)
    return "degradation update: windows " + std::to_string(first) + " .. " + std::to_string((int64_t)first + S - 1) +
           " outside the batch of " + std::to_string(b->count);
  if ((int64_t)ene_col + T > b->total_n)
    return "degradation update: columns " + std::to_string(ene_col) + " .. + " + std::to_string(T) +
           " outside the batch's " + std::to_string(b->total_n);
  if (!std::isfinite(days) || !std::isfinite(eol)) return "degradation update: days or eol_condition not finite";
  if (S > 0 && (!b->desc || !b->x || !b->istats)) return "degradation update: null device array in packed batch";
  if (S > 0 && (!st->e_rated || !st->yearly || !st->soh || !st->replaceable || !st->degrade_perc ||
                !st->replacements || !st->skipped || !st->capacity || !st->degradation || !st->reached))
    return "degradation update: null state array";
  return validate_table(upper, life, n_table);
}

}  // namespace dvh
