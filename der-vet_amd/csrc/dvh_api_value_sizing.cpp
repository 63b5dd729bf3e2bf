// dvh_api_value_sizing.cpp -- the economic sizing's entry points (dvh_value_sizing.hip): dvh_value_cuts,
// dvh_value_master.  Both validate on the host (dvh_value_sizing_validate.h), then launch one kernel on the caller's
// stream: no wait.  The only device allocation is the cut pass's workspace for windows above the LDS size, the
// handle's v_zwork (dvh_handle.h): grown on demand and freed by dvh_destroy.
#include "dvh_handle.h"
#include "dvh_value_sizing.h"
#include "dvh_value_sizing_validate.h"

namespace {

constexpr int kLdsT = 768;  // value_cut_kernel keeps z in LDS up to here

}  // namespace

extern "C" int dvh_value_cuts(dvh_handle* h, const dvh_battery_group* group, const dvh_packed* batch, int32_t first,
                              double* cuts_out, void* stream) {
  if (!h) return DVH_ERR_ARG;
  int code = DVH_ERR_ARG;
  const std::string msg = dvh::validate_value_cuts(group, batch, first, cuts_out, &code);
  if (!msg.empty()) return fail(h, code, msg);
  if (group->G == 0) return DVH_OK;
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  DVH_HIP(h, hipSetDevice(h->device));
  dvh::ValueCutArgs a{};
  a.g = *group;
  a.desc = batch->desc;
  a.indices = batch->indices;
  a.data = batch->data;
  a.c = batch->c;
  a.c0 = batch->c0;
  a.q = batch->q;
  a.l = batch->l;
  a.u = batch->u;
  a.x = batch->x;
  a.y = batch->y;
  a.istats = batch->istats;
  a.total_n = batch->total_n;
  a.total_m = batch->total_m;
  a.total_nnz = batch->total_nnz;
  a.first = first;
  a.out = cuts_out;
  a.zwork = nullptr;
  if (group->T > kLdsT) {
    const size_t want = sizeof(double) * (size_t)group->G * (size_t)group->T;
    if (want > h->v_zwork.bytes) {
      // a launch in flight may still use the old buffer: wait for it before the buffer is replaced
      DVH_HIP(h, hipStreamSynchronize(s));
      DVH_HIP(h, h->v_zwork.ensure(want));
    }
    a.zwork = h->v_zwork.as<double>();
  }
  hipError_t e = dvh::launch_value_cuts(a, s);
  if (e != hipSuccess) return hip_fail(h, e, "value_cut_kernel");
  return DVH_OK;
}

extern "C" int dvh_value_master(dvh_handle* h, const dvh_value_master_args* args, void* stream) {
  if (!h) return DVH_ERR_ARG;
  const std::string msg = dvh::validate_value_master(args);
  if (!msg.empty()) return fail(h, DVH_ERR_ARG, msg);
  if (args->count == 0) return DVH_OK;
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  DVH_HIP(h, hipSetDevice(h->device));
  hipError_t e = dvh::launch_value_master(*args, s);
  if (e != hipSuccess) return hip_fail(h, e, "value_master_kernel");
  return DVH_OK;
}
