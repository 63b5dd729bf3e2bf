// dvh_value_sizing.hip -- economic sizing on the device (include/dervet_hip.h dvh_value_cuts, dvh_value_master): the
// optimality cut of every solved candidate window in the sizes (E, P), and per case the cutting-plane master over the
// cuts summed across its windows.  The arithmetic is csrc/dvh_value_cut.h, the same source the host tests compile.
//
// value_cut_kernel: one 256-thread workgroup per window.  K'y comes from the battery pattern's column structure, every
// CSR row checked against it first (vc::check_rows); the only vector the pass keeps is z_t, the demand-charge duals
// summed per step -- in LDS while the window fits the band tier (T <= 768), in the pass's workspace in HBM above that
// (the annual hourly window: T = 8,760).  r_j = c_j - (K'y)_j is consumed where it is formed.  Lane l adds the terms of
// steps l, l + 256, .. in order, each wave halves its partials with xor shuffles, thread 0 adds the four wave sums in
// wave order: no floating-point atomics, bit-identical run to run and to vc::window_cut on the host, and independent of
// the rest of the batch.  A streaming kernel: per T = 744 window it reads the LP's vectors and x, y (~110 KB) once.
//
// value_master_kernel: one wave per case.  Lanes 0 .. C - 1 each sum one candidate's window cuts in window order; lane 0
// appends them to the case's cut list in HBM, updates the incumbent and the bounds, solves the master
// (vc::master_solve, serial: <= 256 cuts, 3 x 3 solves) and writes the next round's candidates.
#include "dvh_value_cut.h"  // (first: it switches contraction off for the whole file)

#include "dvh_value_sizing.h"

namespace dvh {
namespace {

constexpr int kCutB = vc::kCutLanes;
constexpr int kLanes = vc::kWaveLanes;
constexpr int kCutW = kCutB / kLanes;
constexpr int kLdsT = 768;  // the band tier's largest window
constexpr int kMasterB = 64;

__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kLanes);
  return v;
}
__device__ __forceinline__ double wave_tree_max(double v) {
#pragma unroll
  for (int o = kLanes / 2; o > 0; o >>= 1) v = vc::max2(v, __shfl_xor(v, o, kLanes));
  return v;
}

__global__ __launch_bounds__(kCutB) void value_cut_kernel(const ValueCutArgs a) {
  __shared__ double zl[kLdsT];
  __shared__ double red[kCutW][vc::kCutSums];
  __shared__ double wmax[kCutW];
  __shared__ double wtau[kCutW];
  __shared__ double tausum[vc::kMaxJ];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & (kLanes - 1), wv = tid / kLanes;
  const int64_t w = (int64_t)a.first + g;
  const int T = a.g.T, J = a.g.J, mI = a.g.mI;
  double* out = a.out + (int64_t)g * vc::kCutCols;
  // the window must be the group's battery shape, inside the arrays: else it is never read
  const int64_t* d = a.desc + 8 * w;
  const int64_t n = 3 * (int64_t)T + J, m = (int64_t)T + 1 + mI, nnz = 4 * (int64_t)T + 3 * (int64_t)mI;
  int bad = 0;
  if (d[0] != n || d[1] != m || d[3] != nnz || d[5] < 0 || d[6] < 0 || d[7] < 0 || d[5] > a.total_nnz - nnz ||
      d[6] > a.total_n - n || d[7] > a.total_m - m)
    bad = vc::kBadShape;
  if (!bad && a.g.pch[g] != a.g.pdis[g]) bad = vc::kBadRating;
  vc::CutIn in;
  in.T = T;
  in.J = J;
  in.mI = mI;
  in.dcm_t = a.g.dcm_t;
  in.dcm_j = a.g.dcm_j;
  if (!bad) {
    in.ix = a.indices + d[5];
    in.dv = a.data + d[5];
    in.c = a.c + d[6];
    in.l = a.l + d[6];
    in.u = a.u + d[6];
    in.x = a.x + d[6];
    in.q = a.q + d[7];
    in.y = a.y + d[7];
    in.c0 = a.c0[w];
    in.E = a.g.E[g];
    in.P = a.g.pch[g];
    in.soc_target = a.g.soc_target[g];
    in.llsoc = a.g.llsoc[g];
    in.ulsoc = a.g.ulsoc[g];
    in.emax = a.g.has_emax ? a.g.emax + (int64_t)g * T : nullptr;
    bad = vc::check_rows(in, tid, kCutB);
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) vc::bad_cut(bad, out);
    return;
  }
  double* z = T <= kLdsT ? zl : a.zwork + (int64_t)g * T;
  for (int t = tid; t < T; t += kCutB) z[t] = 0.0;
  __syncthreads();
  // one pass per demand period: a step has at most one row in it (check_rows), so no two lanes add to one z_t
  for (int j = 0; j < J; ++j) {
    double s = vc::scatter_pass(in, j, tid, kCutB, z);
    s = wave_tree_sum(s);
    if (lane == 0) wtau[wv] = s;
    __syncthreads();  // (orders this pass's z before the next one's, too)
    if (tid == 0) {
      double r = wtau[0];
#pragma unroll
      for (int k = 1; k < kCutW; ++k) r += wtau[k];
      tausum[j] = r;
    }
    __syncthreads();
  }
  double s[vc::kCutSums], rinf;
  vc::lane_sums(in, z, tid, kCutB, s, &rinf);
#pragma unroll
  for (int u = 0; u < vc::kCutSums; ++u) {
    s[u] = wave_tree_sum(s[u]);
    if (lane == 0) red[wv][u] = s[u];
  }
  rinf = wave_tree_max(rinf);
  if (lane == 0) wmax[wv] = rinf;
  __syncthreads();
  if (tid != 0) return;
  double tot[vc::kCutSums];
#pragma unroll
  for (int u = 0; u < vc::kCutSums; ++u) {
    double r = red[0][u];
#pragma unroll
    for (int k = 1; k < kCutW; ++k) r += red[k][u];
    tot[u] = r;
  }
  double ri = wmax[0];
#pragma unroll
  for (int k = 1; k < kCutW; ++k) ri = vc::max2(ri, wmax[k]);
  vc::finish_cut(in, tot, ri, tausum, out);
  out[vc::cFlag] = 0.0;
  out[vc::cStatus] = (double)a.istats[2 * w];
  out[vc::cIters] = (double)a.istats[2 * w + 1];
  out[vc::cReserved] = 0.0;
}

__global__ __launch_bounds__(kMasterB) void value_master_kernel(const dvh_value_master_args a) {
  __shared__ double cand[DVH_VALUE_MAX_CAND][4];  // {sum a, sum gE, sum gP, sum pobj}
  __shared__ int cbad[DVH_VALUE_MAX_CAND][2];     // {first window status that is not OPTIMAL (or -1: a bad cut), iters}
  const int k = blockIdx.x, lane = threadIdx.x;
  const int C = a.n_cand, W = a.W;
  const int id = a.case_ids[k];
  if ((unsigned)id >= (unsigned)a.n_cases) return;  // (the ids are device memory: checked here)
  if (lane < C) {
    double sa = 0.0, sge = 0.0, sgp = 0.0, sp = 0.0;
    int st = 0, it = 0;
    for (int p = 0; p < W; ++p) {  // window order
      const double* wc = a.window_cuts + (((int64_t)p * a.count + k) * C + lane) * vc::kCutCols;
      const int flag = (int)wc[vc::cFlag], ws = (int)wc[vc::cStatus];
      if (st == 0 && flag != 0) st = -1;
      else if (st == 0 && ws != DVH_OPTIMAL) st = ws;
      it += (int)wc[vc::cIters];
      sa = p == 0 ? wc[vc::cA] : sa + wc[vc::cA];
      sge = p == 0 ? wc[vc::cGE] : sge + wc[vc::cGE];
      sgp = p == 0 ? wc[vc::cGP] : sgp + wc[vc::cGP];
      sp = p == 0 ? wc[vc::cPobj] : sp + wc[vc::cPobj];
    }
    cand[lane][0] = sa;
    cand[lane][1] = sge;
    cand[lane][2] = sgp;
    cand[lane][3] = sp;
    cbad[lane][0] = st;
    cbad[lane][1] = it;
  }
  __syncthreads();
  if (lane != 0) return;
  const dvh_value_spec& sp = a.spec[id];
  double* st = a.state + (int64_t)id * DVH_VALUE_STATE_COLS;
  int32_t* fl = a.flags + (int64_t)id * DVH_VALUE_FLAG_COLS;
  double* cuts = a.cuts + (int64_t)id * a.cut_cap * 3;
  if (fl[DVH_VF_DONE]) return;
  int ncut = fl[DVH_VF_NCUTS];
  fl[DVH_VF_ROUNDS] += 1;
  for (int j = 0; j < C; ++j) fl[DVH_VF_LP_ITERS] += cbad[j][1];
  // a candidate whose window is not OPTIMAL ends the case
  for (int j = 0; j < C; ++j)
    if (cbad[j][0] != 0) {
      fl[DVH_VF_DONE] = 1;
      fl[DVH_VF_STATUS] = DVH_VALUE_LP_FAILED;
      fl[DVH_VF_LP_STATUS] = cbad[j][0];
      return;
    }
  // the candidates' sizes are this round's entries of the builder's arrays
  for (int j = 0; j < C; ++j) {
    const double E = a.E_in[(int64_t)k * C + j], P = a.P_in[(int64_t)k * C + j];
    if (ncut < a.cut_cap) {
      cuts[3 * ncut] = cand[j][0];
      cuts[3 * ncut + 1] = cand[j][1];
      cuts[3 * ncut + 2] = cand[j][2];
      ++ncut;
    }
    const double F = ((sp.c_energy * E + sp.c_power * P) + sp.alpha * cand[j][3]) + sp.c_fixed;
    if (!(F >= st[DVH_VS_UPPER])) {  // (upper starts at +inf)
      st[DVH_VS_UPPER] = F;
      st[DVH_VS_INC_E] = E;
      st[DVH_VS_INC_P] = P;
      st[DVH_VS_INC_V] = cand[j][3];
    }
  }
  fl[DVH_VF_NCUTS] = ncut;
  vc::MasterIn mi;
  mi.n = ncut;
  mi.cut = cuts;
  mi.cE = sp.c_energy;
  mi.cP = sp.c_power;
  mi.alpha = sp.alpha;
  mi.Elo = sp.energy_min;
  mi.Ehi = sp.energy_max;
  mi.Plo = sp.power_min;
  mi.Phi = sp.power_max;
  double zs[4];
  const int ms = vc::master_solve(mi, zs);
  fl[DVH_VF_MASTER] = ms;
  if (ms != vc::kMasterOk) {
    fl[DVH_VF_DONE] = 1;
    fl[DVH_VF_STATUS] = DVH_VALUE_MASTER_FAILED;
    return;
  }
  const double lower = zs[3] + sp.c_fixed;
  if (lower > st[DVH_VS_LOWER]) st[DVH_VS_LOWER] = lower;
  st[DVH_VS_Z_E] = zs[0];
  st[DVH_VS_Z_P] = zs[1];
  st[DVH_VS_THETA] = zs[2];
  const double upper = st[DVH_VS_UPPER];
  if (upper - st[DVH_VS_LOWER] <= sp.gap_tol * (1.0 + fabs(upper))) {
    fl[DVH_VF_DONE] = 1;
    fl[DVH_VF_STATUS] = DVH_VALUE_SIZED;
    return;
  }
  if (fl[DVH_VF_ROUNDS] >= sp.max_rounds || ncut + a.n_next > a.cut_cap) {
    fl[DVH_VF_DONE] = 1;
    fl[DVH_VF_STATUS] = DVH_VALUE_ROUND_LIMIT;
    return;
  }
  // next round: the master optimum, then the points (j / Cn) of the way from the incumbent to it
  const int Cn = a.n_next;
  const double iE = st[DVH_VS_INC_E], iP = st[DVH_VS_INC_P];
  for (int j = 0; j < Cn; ++j) {
    double E = zs[0], P = zs[1];
    if (j > 0) {
      const double f = (double)j / (double)Cn;
      E = iE + f * (zs[0] - iE);
      P = iP + f * (zs[1] - iP);
    }
    a.E_out[(int64_t)k * Cn + j] = E;
    a.pch_out[(int64_t)k * Cn + j] = P;
    a.pdis_out[(int64_t)k * Cn + j] = P;
  }
}

}  // namespace

hipError_t launch_value_cuts(const ValueCutArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(value_cut_kernel, dim3(a.g.G), dim3(kCutB), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_value_master(const dvh_value_master_args& a, hipStream_t s) {
  hipLaunchKernelGGL(value_master_kernel, dim3(a.count), dim3(kMasterB), 0, s, a);
  return hipGetLastError();
}

}  // namespace dvh
