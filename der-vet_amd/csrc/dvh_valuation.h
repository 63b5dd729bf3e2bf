// Launchers of the valuation kernels (dvh_valuation.hip), called by the entry points in dvh_api_valuation.cpp after
// dvh_valuation_validate.h has passed the arguments.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dervet_hip.h"

namespace dvh {

hipError_t launch_bill(const dvh_bill_group& g, const dvh_packed& b, int first, double* bills, double* peaks,
                       int32_t* bad, hipStream_t s);
// opt_years is copied into the kernel's arguments: nothing of the host arrays is read after the call returns
hipError_t launch_valuation(const dvh_valuation& v, double* values, int32_t* valid, double* proforma, hipStream_t s);

}  // namespace dvh
