// Validation of the reliability sizing entry points' host inputs (dvh_outage_first_uncovered, dvh_sizing_windows,
// dvh_size_reliability; include/dervet_hip.h) before anything is packed or copied to the device.  Plain C++ with no HIP
// dependency: tests/native/sizing_sanitize.cpp runs it under AddressSanitizer / UBSan.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/dervet_hip.h"

namespace dvh {

// "" when valid, else the message dvh_last_error reports.
std::string validate_outage_case(const dvh_outage_case& c, int k);
std::string validate_scan(const dvh_outage_case* cases, int32_t count, const int32_t* target_steps);
// L = round-half-even(target_hours / dt); 0 when it is not a positive int32.
int sizing_steps(const dvh_outage_case& c, const dvh_sizing_spec& s);
std::string validate_sizing(const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count);
// starts / n_starts of dvh_sizing_windows (after validate_sizing passed); the LP shapes must fit int32.
std::string validate_starts(const dvh_outage_case* cases, const dvh_sizing_spec* specs, int32_t count,
                            const int32_t* starts, const int32_t* n_starts);
// 14 K L (the LP's nonzeros) fits int32
bool sizing_lp_fits(int64_t K, int64_t L);

}  // namespace dvh
