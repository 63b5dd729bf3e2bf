// dvh_band_shift.hip -- the band kernel's load-shift form (gfx950): battery windows with a controllable (load-shifting)
// load (dervet MicrogridDER/LoadControllable.py:215-251; dervet_hip/lp/builder.py battery_group ctrl_load).  Opt-in:
// dvh_set_kernel_path(h, 6) launches it over the ICE pass's refusals (dvh_cascade.cpp device_cascade).
//
// Same algorithm, scaling and check logic as the interconnection form of dvh_band_grid.hip (restated here: that
// translation unit's machine code is kept bit for bit), on
//   x = [ch(T), dis(T), ene(T), tau(J), pw(T), el(T)],  J <= 4
//   equality rows  the battery form's T + 1 (init row, T - 1 SOE recurrence rows, end row), then T + D load rows in
//                  any order, each step t with exactly one "load row" and at most one "day-start row":
//     load row       pw_t, el_t (+ el_{t+1}): the recurrence inside a day, or the day's last step (no el_{t+1})
//     day-start row  el_t alone
//                  each with its own coefficients and right-hand side (no sign or symmetry is assumed)
//   >= rows        DCM epigraph, at most once per step: ch_t, dis_t, tau_j (+ pw_t)
//   bounds         ch, dis, el >= 0 (lower bound exactly 0), tau free, pw with both of its bounds
// m_eq - 1 is not T here: T is read from the init row's single column index (2 T), then J = n - 5 T and
// D = m_eq - 2 T - 1.  The structure is verified on the device from the CSR pattern (any values, any entry order within a
// row), every entry of every row accounted for; anything else comes back with status kNeedsEll at once.  (The battery
// and ICE forms refuse these windows: under their reading T = m_eq - 1 the init row's column is not 2 T.)
//
// Mapping: 768 lanes per window, lane t owns step t -- five columns, four rows -- with the coefficients, iterates and
// anchors in VGPRs at the 168-VGPR budget of 3 waves per SIMD; the read-only data of the load block and of the DCM row
// (RO) in LDS.  The next step's ene and el and the previous step's SOE and load-row duals go through LDS, the tau columns
// are summed by wave 0 from per-lane partials.  One workgroup per listed window; a workgroup whose window's status is
// no longer kNeedsEll returns at once, so the launch can follow the ICE pass on the same list without a host round trip.
// dvh_options.kkt_predict is ignored; there is no box form, no persistent grid and no in-kernel Farkas test (certify = 1
// works through the after-pass).
#include <type_traits>

#include "dvh_device.h"

namespace dvh {
namespace {

constexpr int kShiftB = 768;  // lanes = steps per window (T <= kShiftB)
constexpr int kJMax = 4;      // tau (demand-period) columns per window
constexpr int kNeedsEll = -2;
constexpr int kNC = 5;  // columns per step: ch, dis, ene, pw, el
constexpr int kNR = 4;  // rows per step: SOE, DCM, load row, day-start row
// RO[u][B]: 0 c of pw, 1 / 2 lower / upper bound of pw, 3 upper bound of el, 4 q of the DCM row, 5 q of the load row,
// 6 q of the day-start row
constexpr int kNRO = 7;

// LDS layout, doubles then ints:
//   XE[B+1] XL[B+1] YS[B+1] YL[B+1] XT[kJMax] red[kNRed(NW+1)+4] TP[kJMax][B] XP[kNC][B] YP[kNR][B] RO[kNRO][B]
//   | ints: dcm[B] lrow[B] srow[B] flag[4]
// The ints hold the step -> row maps from the set-up to the write-back (the checks and the outputs read them).
__host__ __device__ constexpr size_t shift_lds_doubles(int B) {
  const int NW = B / kWave;
  return 4 * (size_t)(B + 1) + kJMax + (size_t)kNRed * (NW + 1) + 4 + (size_t)(kJMax + kNC + kNR + kNRO) * B;
}
__host__ __device__ constexpr size_t shift_lds_bytes(int B) {
  return align16(sizeof(double) * shift_lds_doubles(B)) + align16(sizeof(int32_t) * (3 * (size_t)B + 4));
}
static_assert(shift_lds_bytes(kShiftB) <= 160 * 1024, "one window per CU");

struct ColKktX {
  double rd2, cx, bt, rdx;
};
// KKT pieces of one column / one row, as dvh_band_grid.hip's (scale-free gap terms; the residuals and ||y|| unscaled
// with the single-precision factor fd and a 1-ulp reciprocal).  Out of line, so that the check does not raise the
// iteration loop's register allocation.
__device__ __noinline__ ColKktX shift_col_kkt(double kt, double cj, double loj, double hij, double xj, float fd) {
  const double id = (double)__builtin_amdgcn_rcpf(fd);
  const double rs = cj - kt;  // scaled reduced cost
  const bool fl = isfinite(loj), fh = isfinite(hij);
  const double lam = (fl && fh) ? rs : (fl ? fmax(rs, 0.0) : (fh ? fmin(rs, 0.0) : 0.0));
  const double rd = (rs - lam) * id;
  ColKktX r;
  r.rd2 = rd * rd;
  r.cx = cj * xj;
  r.bt = (fl ? loj * fmax(lam, 0.0) : 0.0) + (fh ? hij * fmin(lam, 0.0) : 0.0);
  r.rdx = fabs(rd) * fabs(xj * (double)fd);
  return r;
}
struct RowKkt {
  double rp2, y2;
};
__device__ __noinline__ RowKkt shift_row_kkt(double kv, double qi, double yi, float fd, int ge) {
  const double dr = (double)fd, idr = (double)__builtin_amdgcn_rcpf(fd);
  double r = (qi - kv) * idr;
  if (ge) r = fmax(r, 0.0);
  return {r * r, (yi * dr) * (yi * dr)};
}

template <int B>
__device__ __forceinline__ void shift_window(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, const int k_in,
                                             const int tid) {
  const int k = __builtin_amdgcn_readfirstlane(k_in);
  // only what the earlier passes refused (the launch follows them on the same list, before the list is formed again)
  if (__builtin_amdgcn_readfirstlane(b.istats[2 * k]) != kNeedsEll) return;
  constexpr int NW = B / kWave, NC = kNC, NR = kNR;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int kl_ = k - ch.first;
  const WinOff W = uniform_win(win_offsets(b, ch, k));
  const int n = W.n, m = W.m, meq = W.meq;
  const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* scal = w.scal + (int64_t)kl_ * kScal;
  auto bail = [&]() {  // stays kNeedsEll: the window continues down the cascade
    if (tid == 0) {
      b.istats[2 * k] = kNeedsEll;
      b.istats[2 * k + 1] = 0;
    }
  };
  const int32_t* gkp = b.indptr + W.row;
  const int32_t* gkc = b.indices + W.nz;
  if (n > kSmallMax || m > kSmallMax || meq < 4 || m < meq || W.nnz < 1) {
    bail();
    return;
  }
  // T from the init row: its single column is ene_0 = 2 T
  if (__builtin_amdgcn_readfirstlane(gkp[1] - gkp[0]) != 1) {
    bail();
    return;
  }
  const int c00 = __builtin_amdgcn_readfirstlane(gkc[gkp[0]]);
  const int T = c00 >> 1;
  const int J = n - 5 * T, D = meq - 2 * T - 1;
  if (c00 < 2 || (c00 & 1) || T > B || J < 0 || J > kJMax || D < 1 || D > T) {
    bail();
    return;
  }
  const int CPW = 3 * T + J, CE = 4 * T + J;  // first pw / el column
  // ---- LDS carve
  double* XE = reinterpret_cast<double*>(smem);  // x-bar (x+) of ene of lane l's step at [l]; [B] stays 0
  double* XL = XE + (B + 1);  // the same of el
  double* YS = XL + (B + 1);  // y (y+) of the init row at [0], of lane l's SOE row at [l + 1]
  double* YL = YS + (B + 1);  // y (y+) of lane l's load row at [l + 1]; [0] stays 0
  double* XT = YL + (B + 1);  // x-bar (x+) of the tau columns
  double* red = XT + kJMax;
  double* TP = red + kNRed * (NW + 1) + 4;  // [kJMax][B] per-lane partial K'y of the tau columns
  double* XP = TP + kJMax * B;              // [NC][B] T(z) of the lane's columns (check iterations)
  double* YP = XP + NC * B;                 // [NR][B] T(z) of the lane's rows
  double* RO = YP + NR * B;                 // [kNRO][B] read-only data (above)
  int32_t* dcm = reinterpret_cast<int32_t*>(smem + align16(sizeof(double) * shift_lds_doubles(B)));
  int32_t* lrow = dcm + B;   // the load row of each step
  int32_t* srow = lrow + B;  // the day-start row of each step
  int32_t* flag = srow + B;

  const double* gkv = b.data + W.nz;  // the window's own (unscaled) data
  const double* craw = b.c + W.on;
  const double* lraw = b.l + W.on;
  const double* uraw = b.u + W.on;
  const double* qraw = b.q + W.om;
  double* dcv = w.dc + W.wn;  // the factors this kernel computes (the outputs are unscaled with them)
  double* drv = w.dr + W.wm;
  double* xo_g = b.x + W.on;
  double* yo_g = b.y + W.om;

  // ---- structure check: every entry of every row accounted for, the step -> row maps
  {
    dcm[tid] = -1;
    lrow[tid] = -1;
    srow[tid] = -1;
    if (tid < 4) flag[tid] = 0;
    __syncthreads();
    int bad = 0, crossed = 0;
    for (int j = tid; j < J; j += B) bad |= !(lraw[3 * T + j] == -INFINITY && uraw[3 * T + j] == INFINITY);  // tau: free
    for (int r = tid; r <= T; r += B) {  // the battery's equality rows (row 0 was read above)
      if (r == 0) continue;
      const int p0 = gkp[r], len = gkp[r + 1] - p0;
      const int t = r - 1;
      if (len != (r < T ? 4 : 3)) {
        bad = 1;
        continue;
      }
      unsigned seen = 0;
      for (int e = 0; e < len; ++e) {
        const int c = gkc[p0 + e];
        const int kind = c == t ? 0 : c == T + t ? 1 : c == 2 * T + t ? 2 : (r < T && c == 2 * T + t + 1) ? 3 : 4;
        if (kind == 4 || ((seen >> kind) & 1u)) bad = 1;
        seen |= 1u << kind;
      }
      // the kernel keeps no lower bound for ch / dis / el; crossed bounds: infeasible as given
      bad |= lraw[t] != 0.0 || lraw[T + t] != 0.0 || lraw[CE + t] != 0.0;
      crossed |= lraw[t] > uraw[t] || lraw[T + t] > uraw[T + t] || lraw[2 * T + t] > uraw[2 * T + t] ||
                 lraw[CPW + t] > uraw[CPW + t] || lraw[CE + t] > uraw[CE + t];
    }
    for (int i = T + 1 + tid; i < meq; i += B) {  // the load's equality rows
      const int p0 = gkp[i], len = gkp[i + 1] - p0;
      if (len < 1 || len > 3) {
        bad = 1;
        continue;
      }
      if (len == 1) {  // day start: el_t alone
        const int c = gkc[p0];
        if (c < CE || c >= CE + T || atomicCAS(&srow[c - CE], -1, i) != -1) bad = 1;
        continue;
      }
      int tp = -1, rb = 0;
      for (int e = 0; e < len; ++e) {
        const int c = gkc[p0 + e];
        if (c >= CPW && c < CE) {
          rb |= tp >= 0;
          tp = c - CPW;
        }
      }
      if (rb || tp < 0) {
        bad = 1;
        continue;
      }
      unsigned seen = 0;
      for (int e = 0; e < len; ++e) {
        const int c = gkc[p0 + e];
        const int kind = c == CPW + tp ? 0 : c == CE + tp ? 1 : (len == 3 && tp + 1 < T && c == CE + tp + 1) ? 2 : 3;
        if (kind == 3 || ((seen >> kind) & 1u)) rb = 1;
        seen |= 1u << kind;
      }
      if (rb || atomicCAS(&lrow[tp], -1, i) != -1) bad = 1;
    }
    for (int i = meq + tid; i < m; i += B) {  // >= rows: DCM epigraph
      const int p0 = gkp[i], len = gkp[i + 1] - p0;
      if (len < 3 || len > 4) {
        bad = 1;
        continue;
      }
      int tc = -1, td = -1, tp = -1, jj = -1, rb = 0;
      for (int e = 0; e < len; ++e) {
        const int c = gkc[p0 + e];
        if (c < 0) {
          rb = 1;
        } else if (c < T) {
          rb |= tc >= 0;
          tc = c;
        } else if (c < 2 * T) {
          rb |= td >= 0;
          td = c - T;
        } else if (c >= 3 * T && c < CPW) {
          rb |= jj >= 0;
          jj = c - 3 * T;
        } else if (c >= CPW && c < CE) {
          rb |= tp >= 0;
          tp = c - CPW;
        } else {
          rb = 1;
        }
      }
      if (rb || tc < 0 || td != tc || jj < 0 || (tp >= 0 && tp != tc) || (len == 4 && tp < 0)) {
        bad = 1;
        continue;
      }
      if (atomicCAS(&dcm[tc], -1, i * 8 + jj) != -1) bad = 1;
    }
    if (bad) flag[0] = 1;
    if (crossed) flag[1] = 1;
    __syncthreads();
    // every step has its load row; with all T + D rows accounted for, the day-start rows are the D others
    if (tid < T && lrow[tid] < 0) flag[0] = 1;
    __syncthreads();
    const int f = __builtin_amdgcn_readfirstlane((flag[0] != 0 ? 1 : 0) | (flag[1] != 0 ? 2 : 0));
    if (f & 1) {
      bail();
      return;
    }
    if (f & 2) {  // crossed bounds, reported as setup_kernel reports them (no iterations)
      if (tid == 0) {
        scal[0] = 0.0;
        scal[6] = 3.0;
        b.istats[2 * k] = 1;  // DVH_PRIMAL_INFEASIBLE
        b.istats[2 * k + 1] = 0;
        for (int u = 0; u < 4; ++u) b.stats[4 * k + u] = u == 0 ? NAN : 0.0;
      }
      return;
    }
  }

  // ---- the lane's step t = tid: columns (v) ch, dis, ene, pw, el; rows (r) SOE, DCM, load row, day-start row
  const int t = tid;
  const bool val = t < T;
  double x[NC], xa[NC], cc[4], hi[3];  // cc[3]: c of el
  double loe = 0.0;  // lower bound of ene (pw's is in RO, the others are 0)
  double ks[4];      // SOE row: coefficients of ch_t, dis_t, ene_t, ene_{t+1}
  double kd[4];      // DCM row: coefficients of ch_t, dis_t, tau_j, pw_t
  double kl[3];      // load row: coefficients of pw_t, el_t, el_{t+1}
  double kst = 0.0;  // day-start row: coefficient of el_t
  double kp0 = 0.0;  // coefficient of ene_t in row t (the init row or the previous lane's SOE row)
  double kpl = 0.0;  // coefficient of el_t in the previous lane's load row
  double y[NR], ya[NR], q0 = 0.0;
  int jt = 0;
  auto ro = [&](int u) -> double& { return RO[u * B + tid]; };
#pragma unroll
  for (int v = 0; v < NC; ++v) x[v] = xa[v] = 0.0;
#pragma unroll
  for (int v = 0; v < 3; ++v) hi[v] = 0.0;
#pragma unroll
  for (int v = 0; v < 4; ++v) cc[v] = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) y[r] = ya[r] = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) ks[u] = kd[u] = 0.0;
  kl[0] = kl[1] = kl[2] = 0.0;
#pragma unroll
  for (int u = 0; u < kNRO; ++u) ro(u) = 0.0;
  // the row of the step's r-th row, or -1 where the step has none (LDS maps, kept to the write-back)
  auto row_of = [&](int r) -> int { return r == 0 ? (val ? t + 1 : -1) : r == 1 ? dcm[tid] : r == 2 ? lrow[tid] : srow[tid]; };
  // ---- the lane's coefficients (unscaled)
  if (val) {
    for (int p = gkp[t + 1]; p < gkp[t + 2]; ++p) {
      const int c = gkc[p];
      const double a = gkv[p];
      if (c == t) ks[0] = a;
      else if (c == T + t) ks[1] = a;
      else if (c == 2 * T + t) ks[2] = a;
      else ks[3] = a;
    }
    for (int p = gkp[t]; p < gkp[t + 1]; ++p)
      if (gkc[p] == 2 * T + t) kp0 = gkv[p];
    const int dv = dcm[tid];
    if (dv >= 0) {
      const int dr_ = dv >> 3;
      jt = dv & 7;
      for (int p = gkp[dr_]; p < gkp[dr_ + 1]; ++p) {
        const int c = gkc[p];
        const double a = gkv[p];
        if (c < T) kd[0] = a;
        else if (c < 2 * T) kd[1] = a;
        else if (c < CPW) kd[2] = a;
        else kd[3] = a;
      }
    }
    const int rl = lrow[tid], rs = srow[tid];
    for (int p = gkp[rl]; p < gkp[rl + 1]; ++p) {
      const int c = gkc[p];
      (c < CE ? kl[0] : c == CE + t ? kl[1] : kl[2]) = gkv[p];
    }
    if (rs >= 0) kst = gkv[gkp[rs]];
    if (t > 0) {
      const int rp = lrow[tid - 1];
      for (int p = gkp[rp]; p < gkp[rp + 1]; ++p)
        if (gkc[p] == CE + t) kpl = gkv[p];
    }
  }
  __syncthreads();  // (every lane has read its neighbour's lrow and its own dcm word)
  if (val) {
    if (dcm[tid] >= 0) dcm[tid] >>= 3;  // (from here on the row alone)
  } else {
    dcm[tid] = lrow[tid] = srow[tid] = -1;
  }
  // Special state in wave 0 (registers sp[], meaning by lane): lane j < J holds tau column j {x, xa, c, -, -, x+};
  // lane kInitLane holds the init row (row 0: ene_0 = target) {y, ya, y+, q, coefficient, -}.
  constexpr int kInitLane = kWave - 1;
  static_assert(kJMax < kInitLane, "tau lanes and the init-row lane are distinct");
  const bool tlane = wid == 0 && lane < J, ilane = wid == 0 && lane == kInitLane;
  double sp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  // ---- scaling: setup_kernel's preconditioning (o.ruiz_iters Ruiz inf-norm passes, then one Pock-Chambolle alpha = 1
  //      pass) restated on this structure as dvh_band_grid.hip restates it, every factor in the registers of the lane
  //      that owns the row / column.
  double fcv[NC], frv[NR], fsp = 1.0, kin0 = 0.0;  // kin0: the init row's coefficient (of ene_0)
#pragma unroll
  for (int v = 0; v < NC; ++v) fcv[v] = 1.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) frv[r] = 1.0;
  if (ilane) kin0 = gkv[gkp[0]];
  auto factor = [](double a) { return a > 0.0 ? __builtin_amdgcn_rsq(a) : 1.0; };
  auto exchange = [&]() {
    XE[tid] = fcv[2];
    XL[tid] = fcv[4];
    YS[tid + 1] = frv[0];
    YL[tid + 1] = frv[2];
    if (tid == 0) XE[B] = XL[B] = YL[0] = 1.0;  // (no step after the last lane's, none before the first: coefficient 0)
    if (tid < kJMax) XT[tid] = tlane ? fsp : 1.0;
    if (ilane) YS[0] = fsp;
  };
  for (int pass = 0; pass <= o.ruiz_iters; ++pass) {
    const bool pc = pass == o.ruiz_iters;
    auto acc = [pc](double a, double v) { return pc ? a + v : fmax(a, v); };
    exchange();
    __syncthreads();
    const double fen = XE[tid + 1], fel = XL[tid + 1], frp = YS[tid], flp = YL[tid], ftj = XT[jt];
    const double f0 = fcv[0], f1 = fcv[1], f2 = fcv[2], f3 = fcv[3], f4 = fcv[4];
    const double r0 = frv[0], r1 = frv[1], r2 = frv[2], r3 = frv[3];
    double nr[NR], nc[NC];
    nr[0] = acc(acc(acc(fabs(ks[0]) * r0 * f0, fabs(ks[1]) * r0 * f1), fabs(ks[2]) * r0 * f2), fabs(ks[3]) * r0 * fen);
    nr[1] = acc(acc(acc(fabs(kd[0]) * r1 * f0, fabs(kd[1]) * r1 * f1), fabs(kd[2]) * r1 * ftj), fabs(kd[3]) * r1 * f3);
    nr[2] = acc(acc(fabs(kl[0]) * r2 * f3, fabs(kl[1]) * r2 * f4), fabs(kl[2]) * r2 * fel);
    nr[3] = fabs(kst) * r3 * f4;
    nc[0] = acc(fabs(ks[0]) * r0 * f0, fabs(kd[0]) * r1 * f0);
    nc[1] = acc(fabs(ks[1]) * r0 * f1, fabs(kd[1]) * r1 * f1);
    nc[2] = acc(fabs(kp0) * frp * f2, fabs(ks[2]) * r0 * f2);
    nc[3] = acc(fabs(kd[3]) * r1 * f3, fabs(kl[0]) * r2 * f3);
    nc[4] = acc(acc(fabs(kpl) * flp * f4, fabs(kl[1]) * r2 * f4), fabs(kst) * r3 * f4);
    // tau columns: per-lane partials (the lane's DCM row, where it is of the period) -> wave 0
    for (int j = 0; j < J; ++j) TP[j * B + tid] = jt == j ? acc(0.0, fabs(kd[2]) * r1 * XT[j]) : 0.0;
    double nsp = 0.0;
    if (ilane) nsp = fabs(kin0) * fsp * XE[0];
    __syncthreads();
    if (wid == 0) {
      for (int j = 0; j < J; ++j) {
        double a = TP[j * B + lane];
#pragma unroll
        for (int r = 1; r < NW; ++r) a = acc(a, TP[j * B + r * kWave + lane]);
        a = uniform(pc ? wave_sum_dpp(a) : wave_max(a));
        if (lane == j) nsp = a;
      }
    }
#pragma unroll
    for (int v = 0; v < NC; ++v) fcv[v] *= factor(nc[v]);
#pragma unroll
    for (int r = 0; r < NR; ++r) frv[r] *= factor(nr[r]);
    if (tlane || ilane) fsp *= factor(nsp);
    __syncthreads();  // every read of this pass's XE / XL / YS / YL / XT / TP is done
  }
  {  // the KKT checks unscale with single-precision copies of the factors: a window whose factors leave
     // [2^-100, 2^100] goes on to the ELL / generic path, which keeps them in double
    auto oor = [](double f_) { return !(f_ >= 0x1p-100 && f_ <= 0x1p100); };
    bool out = oor(fsp);
#pragma unroll
    for (int v = 0; v < NC; ++v) out |= oor(fcv[v]);
#pragma unroll
    for (int r = 0; r < NR; ++r) out |= oor(frv[r]);
    if (__syncthreads_or(out)) {
      bail();
      return;
    }
  }
  exchange();
  __syncthreads();
  {  // scaled coefficients (K Dr) Dc, as setup_kernel forms them
    const double fen = XE[tid + 1], fel = XL[tid + 1], frp = YS[tid], flp = YL[tid], ftj = XT[jt];
    kp0 = kp0 * frp * fcv[2];
    kpl = kpl * flp * fcv[4];
    ks[0] = ks[0] * frv[0] * fcv[0];
    ks[1] = ks[1] * frv[0] * fcv[1];
    ks[2] = ks[2] * frv[0] * fcv[2];
    ks[3] = ks[3] * frv[0] * fen;
    kd[0] = kd[0] * frv[1] * fcv[0];
    kd[1] = kd[1] * frv[1] * fcv[1];
    kd[2] = kd[2] * frv[1] * ftj;
    kd[3] = kd[3] * frv[1] * fcv[3];
    kl[0] = kl[0] * frv[2] * fcv[3];
    kl[1] = kl[1] * frv[2] * fcv[4];
    kl[2] = kl[2] * frv[2] * fel;
    kst = kst * frv[3] * fcv[4];
    if (ilane) kin0 = kin0 * fsp * XE[0];
  }
  // ---- costs, bounds and right-hand sides, scaled (c Dc, l / Dc, u / Dc, q Dr); the factors for the outputs and
  //      the KKT checks; the norms for the primal weight and the relative KKT error
  double nrm[4] = {0.0, 0.0, 0.0, 0.0};  // ||c~||^2, ||q~||^2, ||c||^2, ||q||^2
  auto col = [&](int v) { return v < 3 ? v * T + t : v == 3 ? CPW + t : CE + t; };
  if (val) {
#pragma unroll
    for (int v = 0; v < NC; ++v) {
      const int j = col(v);
      const double d = fcv[v], cj = craw[j];
      const double csj = cj * d, lsj = lraw[j] / d, usj = uraw[j] / d;
      if (v < 3) {
        hi[v < 3 ? v : 0] = usj;
        cc[v < 3 ? v : 0] = csj;
      } else if (v == 3) {
        ro(0) = csj;
        ro(1) = lsj;
        ro(2) = usj;
      } else {
        cc[3] = csj;
        ro(3) = usj;
      }
      if (v == 2) loe = lsj;
      x[v] = xa[v] = fmin(fmax(o.warm ? xo_g[j] / d : 0.0, lsj), usj);
      nrm[0] += csj * csj;
      nrm[2] += cj * cj;
      dcv[j] = d;
      w.fc[W.wn + j] = (float)d;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = row_of(r);
      if (i < 0) continue;
      const double d = frv[r], qi = qraw[i], qsi = qi * d;
      if (r == 0)
        q0 = qsi;
      else
        ro(r + 3) = qsi;
      if (o.warm) y[r] = ya[r] = r == 1 ? fmax(yo_g[i] / d, 0.0) : yo_g[i] / d;
      nrm[1] += qsi * qsi;
      nrm[3] += qi * qi;
      drv[i] = d;
      w.fr[W.wm + i] = (float)d;
    }
  }
  if (tlane) {
    const int j = 3 * T + lane;
    const double cj = craw[j];
    sp[0] = sp[1] = sp[5] = o.warm ? xo_g[j] / fsp : 0.0;
    sp[2] = cj * fsp;
    nrm[0] += sp[2] * sp[2];
    nrm[2] += cj * cj;
    dcv[j] = fsp;
    w.fc[W.wn + j] = (float)fsp;
  }
  if (ilane) {
    const double qi = qraw[0];
    sp[3] = qi * fsp;
    sp[4] = kin0;
    if (o.warm) sp[0] = sp[1] = sp[2] = yo_g[0] / fsp;
    nrm[1] += sp[3] * sp[3];
    nrm[3] += qi * qi;
    drv[0] = fsp;
    w.fr[W.wm] = (float)fsp;
  }
  block_sum<B, 4>(nrm, red);
  const double ncs = sqrt(nrm[0]), nqs = sqrt(nrm[1]);
  const double pw0 = (ncs > 1e-10 && nqs > 1e-10) ? ncs / nqs : 1.0;  // setup_kernel's primal weight
  const int xta = lds_addr(XT + jt);
  // the check iterations' T(z) of the lane's columns / rows
  auto xpi = [&](int v) -> double& { return XP[v * B + tid]; };
  auto ypi = [&](int r) -> double& { return YP[r * B + tid]; };
  if (tid < kJMax) XT[tid] = 0.0;
  if (tid == 0) XE[B] = XL[B] = YS[B] = YL[B] = 0.0;
  XE[tid] = XL[tid] = YS[tid] = YL[tid] = 0.0;
  for (int u = tid; u < kJMax * B; u += B) TP[u] = 0.0;
#pragma unroll
  for (int v = 0; v < NC; ++v) xpi(v) = x[v];
#pragma unroll
  for (int r = 0; r < NR; ++r) ypi(r) = y[r];
  __syncthreads();

  // ---- SpMV pieces (fixed summation order)
  // K^T of the step's columns from its rows' values vr, vps = the value of row t (the previous SOE row) and vpl = the
  // value of the previous step's load row
  auto ktr = [&](const double (&vr)[NR], double vps, double vpl, double (&out)[NC]) {
    out[0] = fma(kd[0], vr[1], ks[0] * vr[0]);
    out[1] = fma(kd[1], vr[1], ks[1] * vr[0]);
    out[2] = fma(ks[2], vr[0], kp0 * vps);
    out[3] = fma(kl[0], vr[2], kd[3] * vr[1]);
    out[4] = fma(kst, vr[3], fma(kl[1], vr[2], kpl * vpl));
  };
  // K of the step's rows, own-column part (the next step's ene / el and the tau term are added by the caller)
  auto kown = [&](const double (&v)[NC], double (&os)[NR]) {
    os[0] = fma(ks[2], v[2], fma(ks[1], v[1], ks[0] * v[0]));
    os[1] = fma(kd[3], v[3], fma(kd[1], v[1], kd[0] * v[0]));
    os[2] = fma(kl[1], v[4], kl[0] * v[3]);
    os[3] = kst * v[4];
  };
  // the iteration's forms with the objective / right-hand side folded into the FMA chains (K^T y - c, K x - q)
  auto ktr_c = [&](const double (&vr)[NR], double vps, double vpl, double (&out)[NC]) {
    out[0] = fma(kd[0], vr[1], fma(ks[0], vr[0], -cc[0]));
    out[1] = fma(kd[1], vr[1], fma(ks[1], vr[0], -cc[1]));
    out[2] = fma(ks[2], vr[0], fma(kp0, vps, -cc[2]));
    out[3] = fma(kl[0], vr[2], fma(kd[3], vr[1], -ro(0)));
    out[4] = fma(kst, vr[3], fma(kl[1], vr[2], fma(kpl, vpl, -cc[3])));
  };
  auto kown_q = [&](const double (&v)[NC], double (&os)[NR]) {
    os[0] = fma(ks[2], v[2], fma(ks[1], v[1], fma(ks[0], v[0], -q0)));
    os[1] = fma(kd[3], v[3], fma(kd[1], v[1], fma(kd[0], v[0], -ro(4))));
    os[2] = fma(kl[1], v[4], fma(kl[0], v[3], -ro(5)));
    os[3] = fma(kst, v[4], -ro(6));
  };
  auto rhs = [&](int r) -> double { return r == 0 ? q0 : ro(r + 3); };
  // per-lane partial K'y of the tau columns from the DCM row's value vd
  auto tau_parts = [&](double vd) {
    for (int j = 0; j < J; ++j) TP[j * B + tid] = (jt == j ? kd[2] : 0.0) * vd;
  };
  // wave 0: lane j < J gets the sum over all lanes of TP[j][.] (fixed order; uniform per column)
  auto tau_kt = [&]() {
    double res = 0.0;
    for (int j = 0; j < J; ++j) {
      double a = 0.0;
#pragma unroll
      for (int r = 0; r < NW; ++r) a += TP[j * B + r * kWave + lane];
      a = uniform(wave_sum_dpp(a));
      if (lane == j) res = a;
    }
    return res;
  };

  // ---- ||Kt||_2 by power iteration (as the ELL kernel: v <- Kt'(Kt v), sigma^2 = |v_P| / |v_{P-1}|)
  double eta = o.step_safety;  // Pock-Chambolle bound ||K~|| <= 1, refined by the power iteration
  if (o.power_iters > 0) {
    const int P = o.power_iters;
    const double v0 = 1.0 / sqrt((double)n);
    double vc[NC];
#pragma unroll
    for (int v = 0; v < NC; ++v) vc[v] = val ? v0 : 0.0;
    double vtau = tlane ? v0 : 0.0;
    double nv[2] = {0.0, 0.0};
    double wr[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) wr[r] = 0.0;
    for (int pi = 0; pi <= P; ++pi) {
      if (pi > 0) {
        ktr(wr, YS[tid], YL[tid], vc);
        if (wid == 0) {
          const double kt = tau_kt();
          vtau = lane < J ? kt : 0.0;
        }
      }
      if (pi >= P - 1) {
        double a = vtau * vtau;
#pragma unroll
        for (int v = 0; v < NC; ++v) a = fma(vc[v], vc[v], a);
        nv[pi - (P - 1)] = a;
      }
      if (pi == P) break;
      XE[tid] = vc[2];
      XL[tid] = vc[4];
      if (tlane) XT[lane] = vtau;
      __syncthreads();
      kown(vc, wr);
      wr[0] = fma(ks[3], XE[tid + 1], wr[0]);
      wr[1] = fma(kd[2], lds_ld(xta), wr[1]);
      wr[2] = fma(kl[2], XL[tid + 1], wr[2]);
      YS[tid + 1] = wr[0];
      YL[tid + 1] = wr[2];
      if (ilane) YS[0] = sp[4] * XE[0];
      tau_parts(wr[1]);
      __syncthreads();
    }
    block_sum<B, 2>(nv, red);
    if (nv[0] > 0.0 && nv[1] > 0.0) eta = o.step_safety / sqrt(sqrt(nv[1] / nv[0]));
    YS[tid] = YL[tid] = 0.0;
    if (tid == 0) YS[B] = YL[B] = 0.0;
    for (int u = tid; u < kJMax * B; u += B) TP[u] = 0.0;
    __syncthreads();
  }
  if (o.warm) {  // y images of the starting point
    YS[tid + 1] = y[0];
    YL[tid + 1] = y[2];
    if (ilane) YS[0] = sp[0];
    tau_parts(y[1]);
    __syncthreads();
  }
  eta = uniform(eta);
  // a warm start's primal weight: the geometric mean of the data's and the starting point's own ||y~0|| / ||x~0||
  double pwi = pw0;
  if (o.warm) {
    double nv[2] = {0.0, 0.0};
#pragma unroll
    for (int v = 0; v < NC; ++v) nv[0] += x[v] * x[v];
#pragma unroll
    for (int r = 0; r < NR; ++r) nv[1] += y[r] * y[r];
    if (tlane) nv[0] += sp[0] * sp[0];
    if (ilane) nv[1] += sp[0] * sp[0];
    block_sum<B, 2>(nv, red);
    if (nv[0] > 1e-20 && nv[1] > 1e-20) pwi = sqrt(sqrt(nv[1] / nv[0]) * pw0);
  }
  double pw = uniform(pwi);
  const double cnorm = uniform(sqrt(nrm[2])), qnorm = uniform(sqrt(nrm[3])), c0 = uniform(b.c0[k]);
  int it = 0, kin = 0, status = kIterLimit;
  double r0 = -1.0, rprev = -1.0;
  double* fin = red + kNRed * NW;
  if (tid == 0)
    for (int u = 0; u < 4; ++u) fin[u] = NAN;
  const int chk = o.check_every > 0 ? o.check_every : 64;
  double tau = uniform(eta / pw), sigma = uniform(eta * pw);
  double sigma2n = uniform(-2.0 * sigma);  // the equality rows' fused dual step (non-check iterations)
  const int kkt_every = o.kkt_every > 0 ? o.kkt_every : 1;
  int ck = chk, kk_ = kkt_every;
  int kbase = 0;
  // the Halpern weights 1 / (k + 2) of the next kWave iterations, one correctly rounded quotient per lane
  auto hload = [&](int k0_) { return 1.0 / (k0_ + lane + 2.0); };
  double hw = hload(0);
  double mv0, mv1, mv2, mv3;

  auto iterate = [&](auto chk_tag) __attribute__((always_inline)) {
    constexpr bool CHECK = decltype(chk_tag)::value;
    if (kin - kbase >= kWave) {
      kbase = kin;
      hw = hload(kin);
    }
    const double cb = readlane_f64(hw, kin - kbase), ca = 1.0 - cb;
    mv0 = mv1 = mv2 = mv3 = 0.0;
    // ---------------- primal half-step (reflected Halpern, rho = 1)
    double kx[NR];  // own-lane part of K x-bar for the dual half-step
    {
      double kty[NC], xb[NC];
      ktr_c(y, YS[tid], YL[tid], kty);
#pragma unroll
      for (int v = 0; v < NC; ++v) {  // branch-free: padding steps have c = lo = hi = 0, stay at 0
        const double lo = v == 2 ? loe : v == 3 ? ro(1) : 0.0;
        const double up = v < 3 ? hi[v < 3 ? v : 0] : v == 3 ? ro(2) : ro(3);
        const double p1 = vmin(vmax(fma(tau, kty[v], x[v]), lo), up);
        xb[v] = fma(2.0, p1, -x[v]);
        if (CHECK) {
          const double d = x[v] - p1, da = p1 - xa[v];
          mv0 += d * d;
          mv1 += da * da;
          xpi(v) = p1;
        }
        x[v] = fma(ca, xb[v], cb * xa[v]);
      }
      XE[tid] = xb[2];
      XL[tid] = xb[4];
      kown_q(xb, kx);
      if (wid == 0 && J > 0) {  // the tau columns (free): lane j of wave 0
        const double kt = tau_kt();
        if (tlane) {
          const double xo = sp[0], xan = sp[1];
          const double p1 = fma(-tau, sp[2] - kt, xo);
          const double xbt = fma(2.0, p1, -xo);
          XT[lane] = xbt;
          sp[0] = fma(ca, xbt, cb * xan);
          if (CHECK) {
            const double d = xo - p1, da = p1 - xan;
            mv0 += d * d;
            mv1 += da * da;
            sp[5] = p1;
          }
        }
      }
    }
    lds_barrier();
    // ---------------- dual half-step (the SOE, load and day-start rows are equalities; the DCM row is >=: dual >= 0;
    //                  an absent row has zero coefficients and right-hand side, its dual stays 0)
    {
      const double xen = XE[tid + 1], xel = XL[tid + 1], xtv = lds_ld(xta);
      kx[0] = fma(ks[3], xen, kx[0]);
      kx[1] = fma(kd[2], xtv, kx[1]);
      kx[2] = fma(kl[2], xel, kx[2]);
      {
        const double p1 = vmax(fma(-sigma, kx[1], y[1]), 0.0);
        if (CHECK) {
          const double d = y[1] - p1, da = p1 - ya[1];
          mv2 += d * d;
          mv3 += da * da;
          ypi(1) = p1;
        }
        y[1] = fma(ca, fma(2.0, p1, -y[1]), cb * ya[1]);
      }
      tau_parts(y[1]);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (r == 1) continue;
        if (!CHECK) {  // no image needed: 2 (y - sigma Kx) - y = y - 2 sigma Kx
          y[r] = fma(ca, fma(sigma2n, kx[r], y[r]), cb * ya[r]);
        } else {
          const double p1 = fma(-sigma, kx[r], y[r]);
          const double d = y[r] - p1, da = p1 - ya[r];
          mv2 += d * d;
          mv3 += da * da;
          ypi(r) = p1;
          y[r] = fma(ca, fma(2.0, p1, -y[r]), cb * ya[r]);
        }
      }
      YS[tid + 1] = y[0];
      YL[tid + 1] = y[2];
      if (ilane) {  // init row: ene_0 = target
        const double y0 = sp[0], ya0 = sp[1];
        const double q1 = fma(sigma, sp[3] - sp[4] * XE[0], y0);
        if (CHECK) {
          const double d = y0 - q1, da = q1 - ya0;
          mv2 += d * d;
          mv3 += da * da;
          sp[2] = q1;
        }
        const double yn = fma(ca, fma(2.0, q1, -y0), cb * ya0);
        sp[0] = yn;
        YS[0] = yn;
      }
    }
    ++it;
    ++kin;
    lds_barrier();
  };

  using F = std::integral_constant<bool, false>;
  using Tt = std::integral_constant<bool, true>;
  while (it < o.max_iters) {
    if (--ck != 0) {
      iterate(F());
      continue;
    }
    ck = chk;
    iterate(Tt());
    // ---------------- check: fixed-point residual of z_k, restart test; every kkt_every-th check the relative
    // KKT error of T(z_k) in the unscaled space (as the other on-chip kernels)
    const bool last = it + chk > o.max_iters;
    const bool kkt = (--kk_ == 0) || last;
    if (kkt) kk_ = kkt_every;
    static_assert(kRdx == kNRed - 1, "the dual-residual term is the last reduced value");
    double acc[kNRed];
    acc[0] = mv0;
    acc[1] = mv1;
    acc[2] = mv2;
    acc[3] = mv3;
#pragma unroll
    for (int u = 4; u < kNRed; ++u) acc[u] = 0.0;
    if (kkt) {
      // images of T(z_k) in XE / XL / XT / YS / YL / TP (YS / YL / TP rewritten from z after the check)
      double xp[NC], yp[NR];
#pragma unroll
      for (int v = 0; v < NC; ++v) xp[v] = xpi(v);
#pragma unroll
      for (int r = 0; r < NR; ++r) yp[r] = ypi(r);
      XE[tid] = xp[2];
      XL[tid] = xp[4];
      YS[tid + 1] = yp[0];
      YL[tid + 1] = yp[2];
      if (ilane) YS[0] = sp[2];
      if (tlane) XT[lane] = sp[5];
      tau_parts(yp[1]);
      lds_barrier();
      auto col_kkt = [&](int j, double kt, double cj, double loj, double hij, double xj) {
        const ColKktX r = shift_col_kkt(kt, cj, loj, hij, xj, w.fc[W.wn + opaque(j)]);
        acc[5] += r.rd2;
        acc[6] += r.cx;
        acc[8] += r.bt;
        acc[kRdx] += r.rdx;
      };
      auto row_kkt = [&](int i, double kv, double qi, double yi, bool ge) {
        const RowKkt r = shift_row_kkt(kv, qi, yi, w.fr[W.wm + opaque(i)], ge);
        acc[4] += r.rp2;
        acc[7] += qi * yi;
        acc[9] += r.y2;
      };
      {
        double kt[NC];
        ktr(yp, YS[tid], YL[tid], kt);
        if (val) {
          col_kkt(t, kt[0], cc[0], 0.0, hi[0], xp[0]);
          col_kkt(T + t, kt[1], cc[1], 0.0, hi[1], xp[1]);
          col_kkt(2 * T + t, kt[2], cc[2], loe, hi[2], xp[2]);
          col_kkt(CPW + t, kt[3], ro(0), ro(1), ro(2), xp[3]);
          col_kkt(CE + t, kt[4], cc[3], 0.0, ro(3), xp[4]);
        }
      }
      if (wid == 0 && J > 0) {
        const double ktt = tau_kt();
        if (tlane) col_kkt(3 * T + lane, ktt, sp[2], -INFINITY, INFINITY, sp[5]);
      }
      {
        double kv[NR];
        kown(xp, kv);
        kv[0] = fma(ks[3], XE[tid + 1], kv[0]);
        kv[1] = fma(kd[2], lds_ld(xta), kv[1]);
        kv[2] = fma(kl[2], XL[tid + 1], kv[2]);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int i = row_of(r);
          if (i >= 0) row_kkt(i, kv[r], rhs(r), yp[r], r == 1);
        }
      }
      if (ilane) row_kkt(0, sp[4] * XE[0], sp[3], sp[2], false);
      block_sum1<B, kNRed, true>(acc, red);
    } else {
      double acc4[4] = {acc[0], acc[1], acc[2], acc[3]};
      block_sum1<B, 4, true>(acc4, red);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = acc4[u];
    }
    const double r = uniform(sqrt(pw * acc[0] + acc[2] / pw));
    if (kkt) {
      const double pobj = uniform(acc[6] + c0), dobj = uniform(acc[7] + acc[8] + c0);
      const double pres = uniform(sqrt(acc[4]) / (1.0 + qnorm));
      const double dres = uniform(sqrt(acc[5]) / (1.0 + cnorm));
      const double gap = uniform(fabs(pobj - dobj) / (1.0 + fabs(pobj) + fabs(dobj)));
      if (tid == 0) {
        fin[0] = pobj;
        fin[1] = pres;
        fin[2] = dres;
        fin[3] = gap;
      }
      if (kkt_done(o, pres, dres, gap, pobj, dobj, acc[4], acc[9], acc[kRdx])) {
        status = kOptimal;
        break;
      }
      if (!(isfinite(pobj) && isfinite(dobj))) {
        status = kNumerical;
        break;
      }
    }
    if (r0 < 0.0) r0 = r;
    const bool restart = (r <= o.b_suff * r0) || (r <= o.b_nec * r0 && rprev >= 0.0 && r > rprev) ||
                         ((double)kin >= o.b_art * (double)it);
    if (restart) {
      const double ddx = sqrt(acc[1]), ddy = sqrt(acc[3]);
      if (ddx > 1e-10 && ddy > 1e-10) pw = uniform(pw_update<false>(ddy / ddx, pw, o.theta));
      tau = uniform(eta / pw);
      sigma = uniform(eta * pw);
      sigma2n = uniform(-2.0 * sigma);
#pragma unroll
      for (int v = 0; v < NC; ++v) x[v] = xa[v] = xpi(v);
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) y[rr] = ya[rr] = ypi(rr);
      if (ilane) sp[0] = sp[1] = sp[2];
      if (tlane) sp[0] = sp[1] = sp[5];
      kin = 0;
      kbase = 0;
      hw = hload(0);
      r0 = r;
      rprev = -1.0;
    } else {
      rprev = r;
    }
    if (restart || kkt) {  // the y images must hold z again (after a restart z = T(z_k))
      YS[tid + 1] = y[0];
      YL[tid + 1] = y[2];
      if (ilane) YS[0] = sp[0];
      tau_parts(y[1]);
      lds_barrier();
    }
    // (a restart check that neither restarts nor checks KKT rewrote no shared value: the next iteration reads what the
    // check iteration wrote before its barriers, and `red` is next written two barriers later -- no barrier here)
  }
  // outputs: the last check's T(z_k), unscaled with the exact double factors
  if (val) {
#pragma unroll
    for (int v = 0; v < NC; ++v) {
      const int j = col(v);
      xo_g[j] = unscale_x(xpi(v), dcv[j], lraw[j], uraw[j]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = row_of(r);
      if (i >= 0) yo_g[i] = ypi(r) * drv[i];
    }
  }
  if (tlane) xo_g[3 * T + lane] = unscale_x(sp[5], dcv[3 * T + lane], lraw[3 * T + lane], uraw[3 * T + lane]);
  if (ilane) yo_g[0] = sp[2] * drv[0];
  if (tid == 0) {
    b.istats[2 * k] = status;
    b.istats[2 * k + 1] = it;
    for (int u = 0; u < 4; ++u) b.stats[4 * k + u] = fin[u];
  }
}

struct ShiftArgs {
  Batch b;
  Work w;
  Chunk ch;
  Opts o;
  const int32_t* list;  // global window indices, or null: the chunk
};
template <int B>
__global__ __launch_bounds__(B, 3) void pdhg_band_shift_kernel(const ShiftArgs args) {
  const int i = blockIdx.x;
  shift_window<B>(args.b, args.w, args.ch, args.o, args.list ? args.list[i] : args.ch.first + i, threadIdx.x);
}

}  // namespace

hipError_t launch_pdhg_band_shift(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                                  const int32_t* list, int nlist, int* variant_out) {
  constexpr int B = kShiftB;
  const size_t lds = shift_lds_bytes(B);
  hipError_t e = hipFuncSetAttribute((const void*)pdhg_band_shift_kernel<B>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  const int count = list ? nlist : ch.count;
  if (count <= 0) return hipSuccess;
  const ShiftArgs args{b, w, ch, o, list};
  hipLaunchKernelGGL((pdhg_band_shift_kernel<B>), dim3(count), dim3(B), lds, s, args);
  if (variant_out) *variant_out = 9000000 + 300 + B / kWave;
  return hipGetLastError();
}

}  // namespace dvh
