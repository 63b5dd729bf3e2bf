// Launchers of the economic-sizing kernels (dvh_value_sizing.hip), called by the entry points in
// dvh_api_value_sizing.cpp after dvh_value_sizing_validate.h has passed the arguments.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dervet_hip.h"

namespace dvh {

struct ValueCutArgs {
  dvh_battery_group g;
  const int64_t* desc;
  const int32_t* indices;
  const double* data;
  const double* c;
  const double* c0;
  const double* q;
  const double* l;
  const double* u;
  const double* x;
  const double* y;
  const int32_t* istats;
  int64_t total_n, total_m, total_nnz;
  int first;
  double* out;    // [G][DVH_VALUE_CUT_COLS]
  double* zwork;  // [G][T] when T is above the LDS size, else unused
};

hipError_t launch_value_cuts(const ValueCutArgs& a, hipStream_t s);
hipError_t launch_value_master(const dvh_value_master_args& a, hipStream_t s);

}  // namespace dvh
