// dvh_valuation.hip -- scenario valuation on the device (include/dervet_hip.h dvh_bill_windows,
// dvh_value_scenarios): what a solved window costs and what a scenario is worth, without the dispatch leaving HBM.
// The arithmetic is csrc/dvh_cba.h, the same source the host tests compile.
//
// bill_kernel: one 256-thread workgroup per window.  Lane l adds the terms of steps l, l + 256, .. in step order, each
// wave halves its partials with five xor shuffles, lane 0 of each wave leaves its sum in LDS and thread 0 adds the
// four in wave order: a fixed order, no floating-point atomics, the order cba::bill_window walks on the host.  The
// demand charge takes one pass over the demand-charge rows per tau column (J <= 16; the rows and the series they point
// at are L2-resident after the first pass), the peak a max reduction of the same shape.  A streaming kernel: per
// T = 744 window it reads ch, dis, base, orig and retail (~30 KB) once and writes 64 bytes.
//
// valuation_kernel: one thread per scenario, 64 per workgroup.  The yearly net value (Y + 1 <= 65 doubles, read again
// and again by the IRR bisection) lives in LDS at stride 64, so no thread indexes a private array: no scratch.
#include "dvh_cba.h"  // (first: it switches contraction off for the whole file)

#include "dvh_valuation.h"

namespace dvh {
namespace {

constexpr int kBillB = cba::kBillLanes;
constexpr int kLanes = cba::kWaveLanes;
constexpr int kBillW = kBillB / kLanes;
constexpr int kValB = 64;

struct BillArgs {
  dvh_bill_group g;
  const int64_t* desc;
  const double* x;
  const int32_t* istats;
  int64_t total_n;
  int first;
  double* bills;
  double* peaks;
  int32_t* bad;
};

__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kLanes);
  return v;
}
__device__ __forceinline__ double wave_tree_max(double v) {
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) v = cba::max2(v, __shfl_xor(v, o, kLanes));
  return v;
}

__global__ __launch_bounds__(kBillB) void bill_kernel(const BillArgs a) {
  __shared__ double red[kBillW][cba::kBillSums];
  __shared__ double wpk[2][kBillW];
  __shared__ double pk[2][cba::kBillMaxJ];
  const int g = blockIdx.x, lane = threadIdx.x & (kLanes - 1), wv = threadIdx.x / kLanes;
  const int64_t w = (int64_t)a.first + g;
  const int T = a.g.T, J = a.g.J;
  cba::BillIn in;
  in.T = T;
  in.J = J;
  in.mI = a.g.mI;
  in.dt = a.g.dt;
  in.has_pv = a.g.has_pv != 0;
  in.has_ice = a.g.has_ice != 0;
  in.has_ev = a.g.has_ev != 0;
  in.dcm_t = a.g.dcm_t;
  in.dcm_j = a.g.dcm_j;
  in.base = a.g.base + (int64_t)g * T;
  in.orig = a.g.orig ? a.g.orig + (int64_t)g * T : in.base;
  in.retail = a.g.retail ? a.g.retail + (int64_t)g * T : nullptr;
  in.da = a.g.da ? a.g.da + (int64_t)g * T : nullptr;
  in.demand = a.g.demand + (int64_t)g * J;
  in.om = a.g.om ? a.g.om[g] : 0.0;
  in.ice_cost = in.has_ice ? a.g.ice_cost[g] : 0.0;
  // a window that is not OPTIMAL, or whose columns do not lie inside it and it inside x, is never read
  const int64_t n = a.desc[8 * w], off = a.desc[8 * w + 6];
  const bool ok = n >= in.need() && n <= a.total_n && off >= 0 && off <= a.total_n - n && a.istats[2 * w] == DVH_OPTIMAL;
  in.x = ok ? a.x + off : nullptr;

  double s[cba::kBillSums];
  cba::lane_sums(in, threadIdx.x, kBillB, s);
#pragma unroll
  for (int u = 0; u < cba::kBillSums; ++u) {
    s[u] = wave_tree_sum(s[u]);
    if (lane == 0) red[wv][u] = s[u];
  }
  int flag = 0;
  for (int j = 0; j < J; ++j) {
    double m, mo;
    flag |= cba::lane_peaks(in, j, threadIdx.x, kBillB, &m, &mo);
    m = wave_tree_max(m);
    mo = wave_tree_max(mo);
    if (lane == 0) {
      wpk[0][wv] = m;
      wpk[1][wv] = mo;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      double r = wpk[threadIdx.x][0];
      for (int k = 1; k < kBillW; ++k) r = cba::max2(r, wpk[threadIdx.x][k]);
      pk[threadIdx.x][j] = r;
    }
    __syncthreads();
  }
  if (J == 0) {  // the rows are still range-checked
    double m, mo;
    flag |= cba::lane_peaks(in, -1, threadIdx.x, kBillB, &m, &mo);
  }
  flag = __syncthreads_or(flag);  // (also orders red and pk before thread 0 reads them)
  if (threadIdx.x != 0) return;
  double tot[cba::kBillSums];
#pragma unroll
  for (int u = 0; u < cba::kBillSums; ++u) {
    double r = red[0][u];
#pragma unroll
    for (int k = 1; k < kBillW; ++k) r += red[k][u];
    tot[u] = r;
  }
  cba::finish_bill(in, tot, pk[0], pk[1], a.bills + (int64_t)g * cba::kBillRows);
  if (a.peaks)
    for (int j = 0; j < J; ++j) a.peaks[(int64_t)g * J + j] = pk[0][j];
  a.bad[g] = (ok ? 0 : cba::kBadWindow) | (flag ? cba::kBadRow : 0);
}

struct ValArgs {
  dvh_valuation v;
  int32_t opt[cba::kMaxYears];
  double* values;
  int32_t* valid;
  double* proforma;
};

__global__ __launch_bounds__(kValB) void valuation_kernel(const ValArgs a) {
  extern __shared__ double net[];  // [Y + 1][kValB]
  __shared__ int32_t opt[cba::kMaxYears];
  __shared__ double growth[cba::kBillCols];
  if ((int)threadIdx.x < a.v.n_opt) opt[threadIdx.x] = a.opt[threadIdx.x];
  if (threadIdx.x < cba::kBillCols) growth[threadIdx.x] = a.v.growth[threadIdx.x];
  __syncthreads();
  const int s = blockIdx.x * kValB + threadIdx.x;
  if (s >= a.v.S) return;
  const int Y = a.v.Y, C = cba::kFixedCols + a.v.n_extra;
  cba::ValIn in;
  in.Y = Y;
  in.n_opt = a.v.n_opt;
  in.n_extra = a.v.n_extra;
  in.opt = opt;
  in.rate = a.v.rate;
  in.growth = growth;
  in.bills = a.v.bills;
  in.bad = a.v.bad;
  in.n_bills = a.v.n_bills;
  in.win_idx = a.v.win_idx;
  in.win_year = a.v.win_year;
  // the device copy of the row pointers is the one that is followed, so it is checked here too
  const int64_t e0 = a.v.win_ptr[s], e1 = a.v.win_ptr[s + 1];
  const bool range = e0 >= 0 && e0 <= e1 && e1 <= a.v.n_win;
  in.e0 = range ? e0 : 0;
  in.e1 = range ? e1 : 0;
  in.capex = a.v.capex[s];
  in.fixed_om = a.v.fixed_om[s];
  in.extra = a.v.extra;
  double* pf = a.proforma ? a.proforma + (int64_t)s * (Y + 1) * C : nullptr;
  const int valid = cba::value_scenario(in, net + threadIdx.x, kValB, a.values + (int64_t)s * cba::kValueCols, pf);
  a.valid[s] = (valid && range) ? 1 : 0;
}

}  // namespace

hipError_t launch_bill(const dvh_bill_group& g, const dvh_packed& b, int first, double* bills, double* peaks,
                       int32_t* bad, hipStream_t s) {
  BillArgs a{g, b.desc, b.x, b.istats, b.total_n, first, bills, peaks, bad};
  hipLaunchKernelGGL(bill_kernel, dim3(g.G), dim3(kBillB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_valuation(const dvh_valuation& v, double* values, int32_t* valid, double* proforma, hipStream_t s) {
  ValArgs a{};
  a.v = v;
  for (int o = 0; o < v.n_opt; ++o) a.opt[o] = v.opt_years[o];
  a.v.opt_years = nullptr;  // (host pointers: the kernel has the copy above and the device win_ptr)
  a.v.win_ptr_host = nullptr;
  a.values = values;
  a.valid = valid;
  a.proforma = proforma;
  const size_t lds = sizeof(double) * (size_t)(v.Y + 1) * kValB;
  hipLaunchKernelGGL(valuation_kernel, dim3((v.S + kValB - 1) / kValB), dim3(kValB), lds, s, a);
  return hipGetLastError();
}

}  // namespace dvh
