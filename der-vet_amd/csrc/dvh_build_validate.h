// Validation and scan of the device builder's EV step codes (dvh_battery_group ev_code, a host array;
// include/dervet_hip.h DVH_EV_*) before anything is launched: the codes decide where the kernel writes, so every
// offset it follows is formed here from checked codes and compared with the LP shape the descriptors must have.
// Plain C++ with no HIP dependency: tests/native/ev_codes_sanitize.cpp runs it under AddressSanitizer / UBSan.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dervet_hip.h"

namespace dvh {

// The scanned layout of one group's EV rows.  tab [3T]: the codes, then per step the row (within the window) and the
// entry (within the window's CSR) of its first EV row -- the start row where it has one, else its load row.
struct EvScan {
  int32_t D = 0, nnz = 0, n_trail = 0;  // start rows, entries of the T + D EV rows, steps of the trailing session
  std::vector<int32_t> tab;
};

// "" when valid, else the message dvh_last_error reports (DVH_ERR_ARG).
inline std::string scan_ev_codes(const int32_t* code, int32_t T, EvScan* out) {
  if (!code || !out) return "battery group: null EV step codes";
  if (T < 1) return "battery group: EV step codes need T >= 1";
  const auto at = [](int32_t t) { return "battery group: EV step code " + std::to_string(t) + ": "; };
  constexpr int32_t kAll = 2 * DVH_EV_TRAIL - 1;
  EvScan s;
  s.tab.resize(3 * (size_t)T);
  int64_t row = (int64_t)T + 1, ent = 4 * (int64_t)T;
  bool first = true;  // the step opens a cycle
  for (int32_t t = 0; t < T; ++t) {
    const int32_t k = code[t];
    if (k < 0 || k > kAll) return at(t) + "unknown flags (" + std::to_string(k) + ")";
    const bool start = k & DVH_EV_START, last = k & DVH_EV_LAST, trail = k & DVH_EV_TRAIL;
    if ((k & DVH_EV_START_TARGET) && !start) return at(t) + "a start value without a start row";
    if ((k & (DVH_EV_END_TARGET | DVH_EV_END_R)) && !last) return at(t) + "an end value inside a cycle";
    if ((k & DVH_EV_END_TARGET) && (k & DVH_EV_END_R)) return at(t) + "two end values";
    if (trail && !(k & DVH_EV_PLUGGED)) return at(t) + "a trailing session's step that is not plugged";
    if (trail && t + 1 < T && !(code[t + 1] & DVH_EV_TRAIL)) return at(t) + "the trailing session does not reach the end";
    if (((k & DVH_EV_END_R) != 0) != (trail && t == T - 1)) return at(t) + "R ends the trailing session and nothing else";
    if (start && (!first || trail)) return at(t) + "a start row inside a cycle or on the trailing session";
    if (first && !start && !trail) return at(t) + "a cycle without a start row that is not the trailing session";
    if (t == T - 1 && !last) return at(t) + "the window's last step does not end its cycle";
    s.tab[t] = k;
    s.tab[(size_t)T + t] = (int32_t)row;
    s.tab[2 * (size_t)T + t] = (int32_t)ent;
    row += 1 + (start ? 1 : 0);
    ent += (start ? 1 : 0) + (last ? 2 : 3);
    s.D += start ? 1 : 0;
    s.n_trail += trail ? 1 : 0;
    first = last;
    if (ent > INT32_MAX) return "battery group: EV rows overflow the entry index";
  }
  if (s.D < 1) return "battery group: EV step codes without a start row";
  s.nnz = (int32_t)(ent - 4 * (int64_t)T);
  *out = std::move(s);
  return "";
}

}  // namespace dvh
