// dvh_degradation.hip -- battery cycle wear and the capacity update on the device (include/dervet_hip.h
// dvh_cycle_damage, dvh_degradation_update): the step between two window positions of a degradation-coupled sweep
// (dervet_hip/degradation.py DegradationSweep), so that the capacities stay in HBM from one position's solve to the
// next position's builder.
//
// One wave per SOE profile, up to four profiles per 256-thread workgroup.  The wave copies its T values coalesced
// into its own LDS strip of 8 (T + 1) bytes; lane 0 then walks the strip with the routines of dvh_rainflow.h -- the
// same source the host tests compile -- compacting the reversals in place and running the three-point stack on the
// compacted array.  Rainflow counting is a chain of T dependent steps per profile; the parallelism is across the
// profiles (a sweep has thousands), and one lane producing each sum in extraction order is what makes the result
// bit-identical to degradation.cycle_damage and run to run.  The cycle-life table sits in LDS in front of the strips.
// LDS is sized from T at launch: monthly windows (T = 744) run 24 waves per CU, an hourly year (T = 8,784) two
// profiles per workgroup, and from T = 10,176 one.
#include "dvh_rainflow.h"  // (first: it switches contraction off for the whole file)

#include "dvh_degradation_validate.h"
#include "dvh_internal.h"

namespace dvh {
namespace {

constexpr int kDegB = 256;
constexpr int kTab = rainflow::kMaxTable;
constexpr size_t kLdsCap = 160 * 1024;

struct DegArgs {
  // the profiles: rows of a plain array (desc == nullptr) or windows first .. of a packed batch
  const double* ene;
  int64_t row_stride;
  const int64_t* desc;
  const int32_t* istats;
  int64_t total_n;
  int first, ene_col;
  int S, T, n_table;
  const double* upper;
  const double* life;
  const double* e_rated;
  double* damage_out;           // plain rows only
  dvh_degradation_state st;     // batch windows only
  double days, eol;
};

__device__ inline size_t strip_len(int T) { return (size_t)T + 1; }

__global__ __launch_bounds__(kDegB) void rainflow_kernel(const DegArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, W = blockDim.x / kWave;
  const int s = blockIdx.x * W + wv;
  const int T = a.T;
  double* tab = lds;
  double* strip = lds + 2 * kTab + (size_t)wv * strip_len(T);
  for (int i = threadIdx.x; i < a.n_table; i += blockDim.x) {
    tab[i] = a.upper[i];
    tab[kTab + i] = a.life[i];
  }
  const bool have = s < a.S;
  bool valid = have;
  if (have) {
    const double* src;
    if (a.desc) {
      const int64_t w = (int64_t)a.first + s;
      const int64_t n = a.desc[8 * w], off = a.desc[8 * w + 6];
      // a profile that does not lie inside its window, or a window outside x, is never read
      const bool inside = (int64_t)a.ene_col + T <= n && off >= 0 && n >= 0 && off + n <= a.total_n;
      valid = inside && a.istats[2 * w] == DVH_OPTIMAL;
      src = a.ene + (inside ? off + a.ene_col : 0);
    } else {
      src = a.ene + (int64_t)s * a.row_stride;
    }
    if (valid && T >= 2)
      for (int j = lane; j < T; j += kWave) strip[j] = src[j];
  }
  __syncthreads();  // (every thread gets here: the table and the strips are written)
  if (!have || lane != 0) return;
  const double cyc =
      valid ? rainflow::cycle_damage_inplace(strip, T, a.e_rated[s], tab, tab + kTab, a.n_table) : 0.0;
  if (!a.desc) {
    a.damage_out[s] = cyc;
    return;
  }
  const dvh_degradation_state& st = a.st;
  rainflow::State b{st.e_rated[s], st.yearly[s], st.soh[s], st.replaceable[s] != 0,
                    st.degrade_perc[s], st.replacements[s], st.skipped[s]};
  const rainflow::Step o = rainflow::state_update(b, a.days, a.eol, valid, cyc);
  st.degrade_perc[s] = b.degrade_perc;
  st.replacements[s] = b.replacements;
  st.skipped[s] = b.skipped;
  st.capacity[s] = o.capacity;
  st.degradation[s] = o.degradation;
  st.reached[s] = o.reached;
}

// incl_cycle_degrade = 0: Degradation.update returns zeros and changes nothing; the capacity is written all the same,
// so that a caller can hand it to the next position's builder without asking which mode it is in
__global__ __launch_bounds__(kDegB) void degradation_off_kernel(const dvh_degradation_state st, int S) {
  const int s = blockIdx.x * kDegB + threadIdx.x;
  if (s >= S) return;
  st.degradation[s] = 0.0;
  st.reached[s] = 0;
  st.capacity[s] = rainflow::capacity_of(st.e_rated[s], st.degrade_perc[s]);
}

// waves (profiles) per workgroup: four while their strips fit the LDS, else two, else one; 0: T does not fit
int waves_for(int T, size_t* lds) {
  const size_t strip = sizeof(double) * ((size_t)T + 1), tab = sizeof(double) * 2 * kTab;
  for (int W = kDegB / kWave; W >= 1; W /= 2)
    if (tab + W * strip <= kLdsCap) {
      *lds = tab + W * strip;
      return W;
    }
  return 0;
}

hipError_t launch_rainflow(const DegArgs& a, hipStream_t s) {
  size_t lds = 0;
  const int W = waves_for(a.T, &lds);
  if (W == 0) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute((const void*)rainflow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rainflow_kernel, dim3((a.S + W - 1) / W), dim3(W * kWave), lds, s, a);
  return hipGetLastError();
}

}  // namespace
}  // namespace dvh

extern "C" int dvh_cycle_damage(dvh_handle* h, const double* ene, int64_t row_stride, int32_t S, int32_t T,
                                const double* e_rated, const double* upper, const double* life, int32_t n_table,
                                double* damage_out, void* stream) {
  if (!h) return DVH_ERR_ARG;
  const dvh::HandleView v = dvh::handle_view(h);
  const std::string msg = dvh::validate_cycle_damage(ene, row_stride, S, T, e_rated, upper, life, n_table, damage_out);
  if (!msg.empty()) return dvh::fail(v, DVH_ERR_ARG, msg);
  if (T > dvh::kRainflowMaxT)
    return dvh::fail(v, DVH_ERR_UNSUPPORTED, "cycle damage: T = " + std::to_string(T) + " steps do not fit a workgroup's "
                     "LDS (at most " + std::to_string(dvh::kRainflowMaxT) + ")");
  if (S == 0) return DVH_OK;
  DVH_VIEW_HIP(v, hipSetDevice(v.device));
  dvh::DegArgs a{};
  a.ene = ene;
  a.row_stride = row_stride;
  a.S = S;
  a.T = T;
  a.n_table = n_table;
  a.upper = upper;
  a.life = life;
  a.e_rated = e_rated;
  a.damage_out = damage_out;
  hipError_t e = dvh::launch_rainflow(a, stream ? (hipStream_t)stream : v.stream);
  if (e != hipSuccess) return dvh::fail(v, DVH_ERR_HIP, std::string("rainflow_kernel: ") + hipGetErrorString(e));
  return DVH_OK;
}

extern "C" int dvh_degradation_update(dvh_handle* h, const dvh_packed* batch, int32_t first, int32_t S, int32_t T,
                                      int32_t ene_col, double days, double eol_condition, const double* upper,
                                      const double* life, int32_t n_table, const dvh_degradation_state* state,
                                      void* stream) {
  if (!h) return DVH_ERR_ARG;
  const dvh::HandleView v = dvh::handle_view(h);
  const std::string msg =
      dvh::validate_degradation_update(batch, first, S, T, ene_col, days, eol_condition, upper, life, n_table, state);
  if (!msg.empty()) return dvh::fail(v, DVH_ERR_ARG, msg);
  if (T > dvh::kRainflowMaxT)
    return dvh::fail(v, DVH_ERR_UNSUPPORTED, "degradation update: T = " + std::to_string(T) + " steps do not fit a "
                     "workgroup's LDS (at most " + std::to_string(dvh::kRainflowMaxT) + ")");
  if (S == 0) return DVH_OK;
  DVH_VIEW_HIP(v, hipSetDevice(v.device));
  hipStream_t s = stream ? (hipStream_t)stream : v.stream;
  if (!state->incl_cycle_degrade) {
    hipLaunchKernelGGL(dvh::degradation_off_kernel, dim3((S + dvh::kDegB - 1) / dvh::kDegB), dim3(dvh::kDegB), 0, s,
                       *state, S);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dvh::fail(v, DVH_ERR_HIP, std::string("degradation_off_kernel: ") + hipGetErrorString(e));
    return DVH_OK;
  }
  dvh::DegArgs a{};
  a.ene = batch->x;
  a.desc = batch->desc;
  a.istats = batch->istats;
  a.total_n = batch->total_n;
  a.first = first;
  a.ene_col = ene_col;
  a.S = S;
  a.T = T;
  a.n_table = n_table;
  a.upper = upper;
  a.life = life;
  a.e_rated = state->e_rated;
  a.st = *state;
  a.days = days;
  a.eol = eol_condition;
  hipError_t e = dvh::launch_rainflow(a, s);
  if (e != hipSuccess) return dvh::fail(v, DVH_ERR_HIP, std::string("rainflow_kernel: ") + hipGetErrorString(e));
  return DVH_OK;
}
