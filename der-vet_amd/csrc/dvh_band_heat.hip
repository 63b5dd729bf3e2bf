// dvh_band_heat.hip -- the band kernel's heat form (gfx950): battery windows with one combined-heat-and-power unit
// (dervet MicrogridDER/CombinedHeatPower.py:85-97, CombustionTurbine.py:79-88, RotatingGeneratorSizing.py:110-136, the
// thermal balance of MicrogridPOI.py:215-258; dervet_hip/lp/builder.py battery_group chp).  Opt-in:
// dvh_set_kernel_path(h, 7) launches it over the ICE pass's refusals (dvh_cascade.cpp device_cascade) and over the
// heat-sized windows above the on-chip limit of the other kernels (dvh_solve.cpp solve_packed).
//
// Same algorithm, scaling, restart and check logic as the load-shift form of dvh_band_shift.hip (restated here: that
// translation unit's machine code is kept bit for bit), on
//   x = [ch(T), dis(T), ene(T), tau(J), elec(T), on(T), steam(T), hotwater(T)],  J <= 4
//   equality rows  the battery form's T + 1 (init row, T - 1 SOE recurrence rows, end row), then T heat rows in any
//                  order, one per step: elec_t, steam_t, hotwater_t, right-hand side 0
//   >= rows        in any order: the DCM epigraph, at most once per step: ch_t, dis_t, tau_j (+ elec_t); per step two
//                  generator rows (elec_t, on_t) and one ratio row (steam_t, hotwater_t), right-hand sides 0
//   bounds         ch, dis >= 0 (lower bound exactly 0), ene with both bounds, tau free, 0 <= elec (no upper bound),
//                  0 <= on <= a finite positive number, steam and hotwater with their lower bounds (no upper bound)
//   costs          any, but on's is 0
// m_eq - 1 is not T here: T is read from the init row's single column index (2 T), then J = n - 7 T and m_eq must be
// 2 T + 1.  The structure is verified on the device from the CSR pattern (any values, any entry order within a row),
// every entry of every row accounted for; the data the kernel keeps no slot for (the right-hand sides of the heat,
// generator and ratio rows, on's cost and lower bound, elec's lower bound) are verified to be zero.  Anything else
// comes back with status kNeedsEll at once.  (The battery and ICE forms refuse these windows: under their reading
// T = m_eq - 1 the init row's column is not 2 T; the load-shift form finds n - 5 T > 4 or D = m_eq - 2 T - 1 < 1; the
// interconnection form reads T' = m_eq - 1 = 2 T too: n - 3 T' = T + J > 4 from T = 4 on, and below that its row scan
// fails at the init row.)  The two generator rows of a step have the same pattern and are treated
// alike; which of them is the step's first is decided by their coefficients, so that the arithmetic does not depend on
// the order the rows come in.
//
// Mapping: 768 lanes per window, lane t owns step t -- seven columns, six rows.  Against the load-shift form's budget
// (160 KB of LDS, 168 VGPRs at 3 waves per SIMD) the lane is two columns and two rows heavier, so the data are placed
// differently: the coefficients, iterates and anchors stay in VGPRs; every cost, bound and right-hand side of the lane
// (RO, 15 values) sits in LDS; the tau partials are one value per lane, summed by wave 0 per period from the step ->
// period map that stays in LDS; and the check iterations' T(z) images, written once per check_every iterations and read
// back only by the lane that wrote them, live in the window's slices of the workspace (Work::vbuf / wbuf) instead of
// LDS.  The next step's ene and the previous step's SOE dual go through LDS.  One workgroup per listed window; with
// `gate` a workgroup whose window's status is no longer kNeedsEll returns at once, so the launch can follow the ICE pass
// on the same list without a host round trip.  dvh_options.kkt_predict is ignored; there is no box form, no persistent
// grid and no in-kernel Farkas test (certify = 1 works through the after-pass).
#include <type_traits>

#include "dvh_device.h"

namespace dvh {
namespace {

constexpr int kHeatB = 768;  // lanes = steps per window (T <= kHeatB)
constexpr int kJMax = 4;     // tau (demand-period) columns per window
constexpr int kNeedsEll = -2;
constexpr int kNC = 7;  // columns per step: ch, dis, ene, elec, on, steam, hotwater
constexpr int kNR = 6;  // rows per step: SOE, DCM, heat, first / second generator row, ratio
// RO[u][B]: 0 .. 5 c of ch, dis, ene, elec, steam, hotwater; 6 / 7 upper bound of ch / dis; 8 / 9 lower / upper bound of
// ene; 10 upper bound of on; 11 / 12 lower bound of steam / hotwater; 13 q of the SOE row; 14 q of the DCM row
constexpr int kNRO = 15;

// LDS layout, doubles then ints:
//   XE[B+1] YS[B+1] XT[kJMax] red[kNRed(NW+1)+4] TP[B] RO[kNRO][B] | ints: dcm[B] hrow[B] ga[B] gb[B] rrow[B] flag[4]
// The ints hold the step -> row maps from the set-up to the write-back (the checks and the outputs read them); dcm
// keeps row * 8 + period (wave 0's tau sums read the period).
__host__ __device__ constexpr size_t heat_lds_doubles(int B) {
  const int NW = B / kWave;
  return 2 * (size_t)(B + 1) + kJMax + (size_t)kNRed * (NW + 1) + 4 + (size_t)(1 + kNRO) * B;
}
__host__ __device__ constexpr size_t heat_lds_bytes(int B) {
  return align16(sizeof(double) * heat_lds_doubles(B)) + align16(sizeof(int32_t) * (5 * (size_t)B + 4));
}
static_assert(heat_lds_bytes(kHeatB) <= 160 * 1024, "one window per CU");

struct ColKktX {
  double rd2, cx, bt, rdx;
};
// KKT pieces of one column / one row, as dvh_band_shift.hip's (scale-free gap terms; the residuals and ||y|| unscaled
// with the single-precision factor fd and a 1-ulp reciprocal).  Out of line, so that the check does not raise the
// iteration loop's register allocation.
__device__ __noinline__ ColKktX heat_col_kkt(double kt, double cj, double loj, double hij, double xj, float fd) {
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
__device__ __noinline__ RowKkt heat_row_kkt(double kv, double qi, double yi, float fd, int ge) {
  const double dr = (double)fd, idr = (double)__builtin_amdgcn_rcpf(fd);
  double r = (qi - kv) * idr;
  if (ge) r = fmax(r, 0.0);
  return {r * r, (yi * dr) * (yi * dr)};
}

template <int B>
__device__ __forceinline__ void heat_window(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, const int k_in,
                                            const int gate, const int tid) {
  const int k = __builtin_amdgcn_readfirstlane(k_in);
  // only what the earlier passes refused (the launch follows them on the same list, before the list is formed again)
  if (gate && __builtin_amdgcn_readfirstlane(b.istats[2 * k]) != kNeedsEll) return;
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
  // (the largest window of the form, T = B: n = 7 B + kJMax, m = 6 B + 1 -- above kSmallMax, so no such test here)
  if (n > NC * B + kJMax || m > NR * B + 1 || meq < 5 || m < meq || W.nnz < 1) {
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
  const int J = n - NC * T;
  if (c00 < 4 || (c00 & 1) || T > B || J < 0 || J > kJMax || meq != 2 * T + 1 || m - meq < 3 * T || m - meq > 4 * T) {
    bail();
    return;
  }
  const int CE = 3 * T + J, CO = CE + T, CS = CE + 2 * T, CH = CE + 3 * T;  // first elec / on / steam / hotwater column
  // ---- LDS carve
  double* XE = reinterpret_cast<double*>(smem);  // x-bar (x+) of ene of lane l's step at [l]; [B] stays 0
  double* YS = XE + (B + 1);  // y (y+) of the init row at [0], of lane l's SOE row at [l + 1]
  double* XT = YS + (B + 1);  // x-bar (x+) of the tau columns
  double* red = XT + kJMax;
  double* TP = red + kNRed * (NW + 1) + 4;  // [B] the lane's term of K'y of its tau column
  double* RO = TP + B;                      // [kNRO][B] read-only data (above)
  int32_t* dcm = reinterpret_cast<int32_t*>(smem + align16(sizeof(double) * heat_lds_doubles(B)));
  int32_t* hrow = dcm + B;   // the heat row of each step
  int32_t* ga = hrow + B;    // the first generator row of each step
  int32_t* gb = ga + B;      // the second
  int32_t* rrow = gb + B;    // the ratio row
  int32_t* flag = rrow + B;

  const double* gkv = b.data + W.nz;  // the window's own (unscaled) data
  const double* craw = b.c + W.on;
  const double* lraw = b.l + W.on;
  const double* uraw = b.u + W.on;
  const double* qraw = b.q + W.om;
  double* dcv = w.dc + W.wn;  // the factors this kernel computes (the outputs are unscaled with them)
  double* drv = w.dr + W.wm;
  double* xo_g = b.x + W.on;
  double* yo_g = b.y + W.om;
  double* xim = w.vbuf + W.wn;  // the check iterations' T(z): columns by column index, rows by row index
  double* yim = w.wbuf + W.wm;

  // ---- structure check: every entry of every row accounted for, the step -> row maps
  {
    dcm[tid] = -1;
    hrow[tid] = -1;
    ga[tid] = -1;
    gb[tid] = -1;
    rrow[tid] = -1;
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
      // the kernel keeps no lower bound for ch / dis / elec / on, no upper bound for elec / steam / hotwater and no
      // cost for on; on's upper bound is a finite positive number
      bad |= lraw[t] != 0.0 || lraw[T + t] != 0.0 || lraw[CE + t] != 0.0 || lraw[CO + t] != 0.0;
      bad |= uraw[CE + t] != INFINITY || uraw[CS + t] != INFINITY || uraw[CH + t] != INFINITY;
      bad |= !(uraw[CO + t] > 0.0 && uraw[CO + t] < INFINITY) || craw[CO + t] != 0.0;
      bad |= !(lraw[CS + t] < INFINITY) || !(lraw[CH + t] < INFINITY);
      // crossed bounds: infeasible as given
      crossed |= lraw[t] > uraw[t] || lraw[T + t] > uraw[T + t] || lraw[2 * T + t] > uraw[2 * T + t];
    }
    for (int i = T + 1 + tid; i < meq; i += B) {  // the heat rows: elec_t, steam_t, hotwater_t, right-hand side 0
      const int p0 = gkp[i], len = gkp[i + 1] - p0;
      if (len != 3 || qraw[i] != 0.0) {
        bad = 1;
        continue;
      }
      int te = -1, ts = -1, th = -1, rb = 0;
      for (int e = 0; e < len; ++e) {
        const int c = gkc[p0 + e];
        if (c >= CE && c < CO) {
          rb |= te >= 0;
          te = c - CE;
        } else if (c >= CS && c < CH) {
          rb |= ts >= 0;
          ts = c - CS;
        } else if (c >= CH && c < CH + T) {
          rb |= th >= 0;
          th = c - CH;
        } else {
          rb = 1;
        }
      }
      if (rb || te < 0 || ts != te || th != te || atomicCAS(&hrow[te], -1, i) != -1) bad = 1;
    }
    for (int i = meq + tid; i < m; i += B) {  // >= rows: DCM epigraph, generator rows, ratio rows
      const int p0 = gkp[i], len = gkp[i + 1] - p0;
      if (len < 2 || len > 4) {
        bad = 1;
        continue;
      }
      if (len == 2) {  // (elec_t, on_t) or (steam_t, hotwater_t), right-hand side 0
        const int c0 = gkc[p0], c1 = gkc[p0 + 1];
        const int lo = c0 < c1 ? c0 : c1, hi = c0 < c1 ? c1 : c0;
        if (qraw[i] != 0.0) {
          bad = 1;
        } else if (lo >= CE && lo < CO && hi == lo + T) {
          const int t = lo - CE;
          if (atomicCAS(&ga[t], -1, i) != -1 && atomicCAS(&gb[t], -1, i) != -1) bad = 1;
        } else if (lo >= CS && lo < CH && hi == lo + T) {
          if (atomicCAS(&rrow[lo - CS], -1, i) != -1) bad = 1;
        } else {
          bad = 1;
        }
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
        } else if (c >= 3 * T && c < CE) {
          rb |= jj >= 0;
          jj = c - 3 * T;
        } else if (c >= CE && c < CO) {
          rb |= tp >= 0;
          tp = c - CE;
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
    // every step has its heat row, its two generator rows and its ratio row
    if (tid < T && (hrow[tid] < 0 || ga[tid] < 0 || gb[tid] < 0 || rrow[tid] < 0)) flag[0] = 1;
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

  // ---- the lane's step t = tid: columns (v) ch, dis, ene, elec, on, steam, hotwater; rows (r) SOE, DCM, heat, first /
  //      second generator row, ratio
  const int t = tid;
  const bool val = t < T;
  double x[NC], xa[NC];
  double ks[4];      // SOE row: coefficients of ch_t, dis_t, ene_t, ene_{t+1}
  double kd[4];      // DCM row: coefficients of ch_t, dis_t, tau_j, elec_t
  double kh[3];      // heat row: coefficients of steam_t, hotwater_t, elec_t
  double kg[4];      // generator rows: coefficients of elec_t, on_t of the first, of the second
  double kr[2];      // ratio row: coefficients of steam_t, hotwater_t
  double kp0 = 0.0;  // coefficient of ene_t in row t (the init row or the previous lane's SOE row)
  double y[NR], ya[NR];
  int jt = 0;
  auto ro = [&](int u) -> double& { return RO[u * B + tid]; };
#pragma unroll
  for (int v = 0; v < NC; ++v) x[v] = xa[v] = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) y[r] = ya[r] = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) ks[u] = kd[u] = kg[u] = 0.0;
  kh[0] = kh[1] = kh[2] = kr[0] = kr[1] = 0.0;
#pragma unroll
  for (int u = 0; u < kNRO; ++u) ro(u) = 0.0;
  // (the two generator rows of a step in row order)
  if (val && ga[tid] > gb[tid]) {
    const int a_ = ga[tid];
    ga[tid] = gb[tid];
    gb[tid] = a_;
  }
  // the row of the step's r-th row, or -1 where the step has none (LDS maps, kept to the write-back)
  auto row_of = [&](int r) -> int {
    return r == 0 ? (val ? t + 1 : -1)
                  : r == 1 ? (dcm[tid] >= 0 ? dcm[tid] >> 3 : -1) : r == 2 ? hrow[tid] : r == 3 ? ga[tid] : r == 4 ? gb[tid] : rrow[tid];
  };
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
        else if (c < CE) kd[2] = a;
        else kd[3] = a;
      }
    }
    const int rh = hrow[tid], r3 = ga[tid], r4 = gb[tid], r5 = rrow[tid];
    for (int p = gkp[rh]; p < gkp[rh + 1]; ++p) {
      const int c = gkc[p];
      (c < CO ? kh[2] : c < CH ? kh[0] : kh[1]) = gkv[p];
    }
    for (int p = gkp[r3]; p < gkp[r3 + 1]; ++p) (gkc[p] < CO ? kg[0] : kg[1]) = gkv[p];
    for (int p = gkp[r4]; p < gkp[r4 + 1]; ++p) (gkc[p] < CO ? kg[2] : kg[3]) = gkv[p];
    // the step's first generator row: the one with the larger coefficient of on_t, then of elec_t (the two rows are
    // treated alike; the rule only makes the arithmetic independent of the order the rows come in)
    if (kg[1] < kg[3] || (kg[1] == kg[3] && kg[0] < kg[2])) {
      const double a0 = kg[0], a1 = kg[1];
      kg[0] = kg[2];
      kg[1] = kg[3];
      kg[2] = a0;
      kg[3] = a1;
      ga[tid] = r4;
      gb[tid] = r3;
    }
    for (int p = gkp[r5]; p < gkp[r5 + 1]; ++p) (gkc[p] < CH ? kr[0] : kr[1]) = gkv[p];
  } else {
    dcm[tid] = hrow[tid] = ga[tid] = gb[tid] = rrow[tid] = -1;
  }
  // Special state in wave 0 (registers sp[], meaning by lane): lane j < J holds tau column j {x, xa, c, -, -, x+};
  // lane kInitLane holds the init row (row 0: ene_0 = target) {y, ya, y+, q, coefficient, -}.
  constexpr int kInitLane = kWave - 1;
  static_assert(kJMax < kInitLane, "tau lanes and the init-row lane are distinct");
  const bool tlane = wid == 0 && lane < J, ilane = wid == 0 && lane == kInitLane;
  double sp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  // wave 0: lane j < J gets op-reduced TP[.] over the lanes of period j (fixed order; uniform per column); SUM: a sum,
  // else a maximum of non-negative terms.  A lane without a DCM row has the map word -1 (period 7: none) and TP 0.
  auto tau_reduce = [&](auto sum_tag) {
    constexpr bool SUM = decltype(sum_tag)::value;
    double a[kJMax] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < NW; ++r) {
      const double v = TP[r * kWave + lane];
      const int jj = dcm[r * kWave + lane] & 7;
#pragma unroll
      for (int j = 0; j < kJMax; ++j) {
        const double vj = jj == j ? v : 0.0;
        a[j] = SUM ? a[j] + vj : fmax(a[j], vj);
      }
    }
    double res = 0.0;
#pragma unroll
    for (int j = 0; j < kJMax; ++j) {
      if (j < J) {
        const double s = uniform(SUM ? wave_sum_dpp(a[j]) : wave_max(a[j]));
        if (lane == j) res = s;
      }
    }
    return res;
  };
  using F = std::integral_constant<bool, false>;
  using Tt = std::integral_constant<bool, true>;

  // ---- scaling: setup_kernel's preconditioning (o.ruiz_iters Ruiz inf-norm passes, then one Pock-Chambolle alpha = 1
  //      pass) restated on this structure as dvh_band_shift.hip restates it, every factor in the registers of the lane
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
    YS[tid + 1] = frv[0];
    if (tid == 0) XE[B] = 1.0;  // (no step after the last lane's: coefficient 0)
    if (tid < kJMax) XT[tid] = tlane ? fsp : 1.0;
    if (ilane) YS[0] = fsp;
  };
  __syncthreads();  // (the maps are final: wave 0 reads every lane's dcm word)
  for (int pass = 0; pass <= o.ruiz_iters; ++pass) {
    const bool pc = pass == o.ruiz_iters;
    auto acc = [pc](double a, double v) { return pc ? a + v : fmax(a, v); };
    exchange();
    __syncthreads();
    const double fen = XE[tid + 1], frp = YS[tid], ftj = XT[jt];
    const double f0 = fcv[0], f1 = fcv[1], f2 = fcv[2], f3 = fcv[3], f4 = fcv[4], f5 = fcv[5], f6 = fcv[6];
    const double r0 = frv[0], r1 = frv[1], r2 = frv[2], r3 = frv[3], r4 = frv[4], r5 = frv[5];
    double nr[NR], nc[NC];
    nr[0] = acc(acc(acc(fabs(ks[0]) * r0 * f0, fabs(ks[1]) * r0 * f1), fabs(ks[2]) * r0 * f2), fabs(ks[3]) * r0 * fen);
    nr[1] = acc(acc(acc(fabs(kd[0]) * r1 * f0, fabs(kd[1]) * r1 * f1), fabs(kd[2]) * r1 * ftj), fabs(kd[3]) * r1 * f3);
    nr[2] = acc(acc(fabs(kh[0]) * r2 * f5, fabs(kh[1]) * r2 * f6), fabs(kh[2]) * r2 * f3);
    nr[3] = acc(fabs(kg[0]) * r3 * f3, fabs(kg[1]) * r3 * f4);
    nr[4] = acc(fabs(kg[2]) * r4 * f3, fabs(kg[3]) * r4 * f4);
    nr[5] = acc(fabs(kr[0]) * r5 * f5, fabs(kr[1]) * r5 * f6);
    nc[0] = acc(fabs(ks[0]) * r0 * f0, fabs(kd[0]) * r1 * f0);
    nc[1] = acc(fabs(ks[1]) * r0 * f1, fabs(kd[1]) * r1 * f1);
    nc[2] = acc(fabs(kp0) * frp * f2, fabs(ks[2]) * r0 * f2);
    nc[3] = acc(acc(acc(fabs(kd[3]) * r1 * f3, fabs(kh[2]) * r2 * f3), fabs(kg[0]) * r3 * f3), fabs(kg[2]) * r4 * f3);
    nc[4] = acc(fabs(kg[1]) * r3 * f4, fabs(kg[3]) * r4 * f4);
    nc[5] = acc(fabs(kh[0]) * r2 * f5, fabs(kr[0]) * r5 * f5);
    nc[6] = acc(fabs(kh[1]) * r2 * f6, fabs(kr[1]) * r5 * f6);
    // tau columns: the lane's term (its DCM row's entry) -> wave 0
    TP[tid] = fabs(kd[2]) * r1 * ftj;
    double nsp = 0.0;
    if (ilane) nsp = fabs(kin0) * fsp * XE[0];
    __syncthreads();
    if (wid == 0 && J > 0) {
      const double a = pc ? tau_reduce(Tt()) : tau_reduce(F());
      if (lane < J) nsp = a;
    }
#pragma unroll
    for (int v = 0; v < NC; ++v) fcv[v] *= factor(nc[v]);
#pragma unroll
    for (int r = 0; r < NR; ++r) frv[r] *= factor(nr[r]);
    if (tlane || ilane) fsp *= factor(nsp);
    __syncthreads();  // every read of this pass's XE / YS / XT / TP is done
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
    const double fen = XE[tid + 1], frp = YS[tid], ftj = XT[jt];
    kp0 = kp0 * frp * fcv[2];
    ks[0] = ks[0] * frv[0] * fcv[0];
    ks[1] = ks[1] * frv[0] * fcv[1];
    ks[2] = ks[2] * frv[0] * fcv[2];
    ks[3] = ks[3] * frv[0] * fen;
    kd[0] = kd[0] * frv[1] * fcv[0];
    kd[1] = kd[1] * frv[1] * fcv[1];
    kd[2] = kd[2] * frv[1] * ftj;
    kd[3] = kd[3] * frv[1] * fcv[3];
    kh[0] = kh[0] * frv[2] * fcv[5];
    kh[1] = kh[1] * frv[2] * fcv[6];
    kh[2] = kh[2] * frv[2] * fcv[3];
    kg[0] = kg[0] * frv[3] * fcv[3];
    kg[1] = kg[1] * frv[3] * fcv[4];
    kg[2] = kg[2] * frv[4] * fcv[3];
    kg[3] = kg[3] * frv[4] * fcv[4];
    kr[0] = kr[0] * frv[5] * fcv[5];
    kr[1] = kr[1] * frv[5] * fcv[6];
    if (ilane) kin0 = kin0 * fsp * XE[0];
  }
  // ---- costs, bounds and right-hand sides, scaled (c Dc, l / Dc, u / Dc, q Dr); the factors for the outputs and
  //      the KKT checks; the norms for the primal weight and the relative KKT error
  double nrm[4] = {0.0, 0.0, 0.0, 0.0};  // ||c~||^2, ||q~||^2, ||c||^2, ||q||^2
  auto col = [&](int v) { return v < 3 ? v * T + t : CE + (v - 3) * T + t; };
  if (val) {
#pragma unroll
    for (int v = 0; v < NC; ++v) {
      const int j = col(v);
      const double d = fcv[v], cj = craw[j];
      const double csj = cj * d, lsj = lraw[j] / d, usj = uraw[j] / d;
      if (v < 4) ro(v) = csj;
      if (v > 4) ro(v - 1) = csj;  // (on's cost is 0: verified)
      if (v < 2) ro(6 + v) = usj;
      if (v == 2) {
        ro(8) = lsj;
        ro(9) = usj;
      }
      if (v == 4) ro(10) = usj;
      if (v > 4) ro(6 + v) = lsj;
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
      if (r < 2) ro(13 + r) = qsi;  // (the other rows' right-hand sides are 0: verified)
      if (o.warm) y[r] = ya[r] = (r == 0 || r == 2) ? yo_g[i] / d : fmax(yo_g[i] / d, 0.0);
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
  // the check iterations' T(z) of the lane's columns / rows: written and read by this lane alone (a lane past T, a
  // step without a DCM row: nothing is kept, the value is 0 throughout)
  auto xim_st = [&](int v, double a) {
    if (val) xim[opaque(col(v))] = a;
  };
  auto xim_ld = [&](int v) -> double { return val ? xim[opaque(col(v))] : 0.0; };
  auto yim_st = [&](int r, double a) {
    const int i = row_of(r);
    if (i >= 0) yim[opaque(i)] = a;
  };
  auto yim_ld = [&](int r) -> double {
    const int i = row_of(r);
    return i >= 0 ? yim[opaque(i)] : 0.0;
  };
  if (tid < kJMax) XT[tid] = 0.0;
  if (tid == 0) XE[B] = YS[B] = 0.0;
  XE[tid] = YS[tid] = 0.0;
  TP[tid] = 0.0;
#pragma unroll
  for (int v = 0; v < NC; ++v) xim_st(v, x[v]);
#pragma unroll
  for (int r = 0; r < NR; ++r) yim_st(r, y[r]);
  __syncthreads();

  // ---- SpMV pieces (fixed summation order)
  // K^T of the step's columns from its rows' values vr and vps = the value of row t (the previous SOE row)
  auto ktr = [&](const double (&vr)[NR], double vps, double (&out)[NC]) {
    out[0] = fma(kd[0], vr[1], ks[0] * vr[0]);
    out[1] = fma(kd[1], vr[1], ks[1] * vr[0]);
    out[2] = fma(ks[2], vr[0], kp0 * vps);
    out[3] = fma(kg[2], vr[4], fma(kg[0], vr[3], fma(kh[2], vr[2], kd[3] * vr[1])));
    out[4] = fma(kg[3], vr[4], kg[1] * vr[3]);
    out[5] = fma(kr[0], vr[5], kh[0] * vr[2]);
    out[6] = fma(kr[1], vr[5], kh[1] * vr[2]);
  };
  // K of the step's rows, own-column part (the next step's ene and the tau term are added by the caller)
  auto kown = [&](const double (&v)[NC], double (&os)[NR]) {
    os[0] = fma(ks[2], v[2], fma(ks[1], v[1], ks[0] * v[0]));
    os[1] = fma(kd[3], v[3], fma(kd[1], v[1], kd[0] * v[0]));
    os[2] = fma(kh[2], v[3], fma(kh[1], v[6], kh[0] * v[5]));
    os[3] = fma(kg[1], v[4], kg[0] * v[3]);
    os[4] = fma(kg[3], v[4], kg[2] * v[3]);
    os[5] = fma(kr[1], v[6], kr[0] * v[5]);
  };
  // the iteration's forms with the objective / right-hand side folded into the FMA chains (K^T y - c, K x - q)
  auto ktr_c = [&](const double (&vr)[NR], double vps, double (&out)[NC]) {
    out[0] = fma(kd[0], vr[1], fma(ks[0], vr[0], -ro(0)));
    out[1] = fma(kd[1], vr[1], fma(ks[1], vr[0], -ro(1)));
    out[2] = fma(ks[2], vr[0], fma(kp0, vps, -ro(2)));
    out[3] = fma(kg[2], vr[4], fma(kg[0], vr[3], fma(kh[2], vr[2], fma(kd[3], vr[1], -ro(3)))));
    out[4] = fma(kg[3], vr[4], kg[1] * vr[3]);
    out[5] = fma(kr[0], vr[5], fma(kh[0], vr[2], -ro(4)));
    out[6] = fma(kr[1], vr[5], fma(kh[1], vr[2], -ro(5)));
  };
  auto kown_q = [&](const double (&v)[NC], double (&os)[NR]) {
    os[0] = fma(ks[2], v[2], fma(ks[1], v[1], fma(ks[0], v[0], -ro(13))));
    os[1] = fma(kd[3], v[3], fma(kd[1], v[1], fma(kd[0], v[0], -ro(14))));
    os[2] = fma(kh[2], v[3], fma(kh[1], v[6], kh[0] * v[5]));
    os[3] = fma(kg[1], v[4], kg[0] * v[3]);
    os[4] = fma(kg[3], v[4], kg[2] * v[3]);
    os[5] = fma(kr[1], v[6], kr[0] * v[5]);
  };
  // the lane's term of K'y of its tau column from the DCM row's value vd
  auto tau_parts = [&](double vd) { TP[tid] = kd[2] * vd; };
  auto tau_kt = [&]() { return tau_reduce(Tt()); };

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
        ktr(wr, YS[tid], vc);
        if (wid == 0 && J > 0) {
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
      if (tlane) XT[lane] = vtau;
      __syncthreads();
      kown(vc, wr);
      wr[0] = fma(ks[3], XE[tid + 1], wr[0]);
      wr[1] = fma(kd[2], lds_ld(xta), wr[1]);
      YS[tid + 1] = wr[0];
      if (ilane) YS[0] = sp[4] * XE[0];
      tau_parts(wr[1]);
      __syncthreads();
    }
    block_sum<B, 2>(nv, red);
    if (nv[0] > 0.0 && nv[1] > 0.0) eta = o.step_safety / sqrt(sqrt(nv[1] / nv[0]));
    YS[tid] = 0.0;
    if (tid == 0) YS[B] = 0.0;
    TP[tid] = 0.0;
    __syncthreads();
  }
  if (o.warm) {  // y images of the starting point
    YS[tid + 1] = y[0];
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
      ktr_c(y, YS[tid], kty);
#pragma unroll
      for (int v = 0; v < NC; ++v) {  // branch-free: padding steps have c = lo = hi = 0 where a bound is kept, stay at 0
        double p1 = fma(tau, kty[v], x[v]);
        p1 = vmax(p1, v == 2 ? ro(8) : v == 5 ? ro(11) : v == 6 ? ro(12) : 0.0);
        if (v < 3 || v == 4) p1 = vmin(p1, v < 2 ? ro(6 + v) : v == 2 ? ro(9) : ro(10));
        xb[v] = fma(2.0, p1, -x[v]);
        if (CHECK) {
          const double d = x[v] - p1, da = p1 - xa[v];
          mv0 += d * d;
          mv1 += da * da;
          xim_st(v, p1);
        }
        x[v] = fma(ca, xb[v], cb * xa[v]);
      }
      XE[tid] = xb[2];
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
    // ---------------- dual half-step (the SOE and heat rows are equalities; the DCM, generator and ratio rows are >=:
    //                  dual >= 0; an absent row has zero coefficients and right-hand side, its dual stays 0)
    {
      const double xen = XE[tid + 1], xtv = lds_ld(xta);
      kx[0] = fma(ks[3], xen, kx[0]);
      kx[1] = fma(kd[2], xtv, kx[1]);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (r == 0 || r == 2) continue;
        const double p1 = vmax(fma(-sigma, kx[r], y[r]), 0.0);
        if (CHECK) {
          const double d = y[r] - p1, da = p1 - ya[r];
          mv2 += d * d;
          mv3 += da * da;
          yim_st(r, p1);
        }
        y[r] = fma(ca, fma(2.0, p1, -y[r]), cb * ya[r]);
        if (r == 1) tau_parts(y[1]);
      }
#pragma unroll
      for (int r = 0; r < NR; r += 2) {
        if (r > 2) continue;
        if (!CHECK) {  // no image needed: 2 (y - sigma Kx) - y = y - 2 sigma Kx
          y[r] = fma(ca, fma(sigma2n, kx[r], y[r]), cb * ya[r]);
        } else {
          const double p1 = fma(-sigma, kx[r], y[r]);
          const double d = y[r] - p1, da = p1 - ya[r];
          mv2 += d * d;
          mv3 += da * da;
          yim_st(r, p1);
          y[r] = fma(ca, fma(2.0, p1, -y[r]), cb * ya[r]);
        }
      }
      YS[tid + 1] = y[0];
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
      // images of T(z_k) in XE / XT / YS / TP (YS / TP rewritten from z after the check)
      double xp[NC], yp[NR];
#pragma unroll
      for (int v = 0; v < NC; ++v) xp[v] = xim_ld(v);
#pragma unroll
      for (int r = 0; r < NR; ++r) yp[r] = yim_ld(r);
      XE[tid] = xp[2];
      YS[tid + 1] = yp[0];
      if (ilane) YS[0] = sp[2];
      if (tlane) XT[lane] = sp[5];
      tau_parts(yp[1]);
      lds_barrier();
      auto col_kkt = [&](int j, double kt, double cj, double loj, double hij, double xj) {
        const ColKktX r = heat_col_kkt(kt, cj, loj, hij, xj, w.fc[W.wn + opaque(j)]);
        acc[5] += r.rd2;
        acc[6] += r.cx;
        acc[8] += r.bt;
        acc[kRdx] += r.rdx;
      };
      auto row_kkt = [&](int i, double kv, double qi, double yi, bool ge) {
        const RowKkt r = heat_row_kkt(kv, qi, yi, w.fr[W.wm + opaque(i)], ge);
        acc[4] += r.rp2;
        acc[7] += qi * yi;
        acc[9] += r.y2;
      };
      {
        double kt[NC];
        ktr(yp, YS[tid], kt);
        if (val) {
          col_kkt(col(0), kt[0], ro(0), 0.0, ro(6), xp[0]);
          col_kkt(col(1), kt[1], ro(1), 0.0, ro(7), xp[1]);
          col_kkt(col(2), kt[2], ro(2), ro(8), ro(9), xp[2]);
          col_kkt(col(3), kt[3], ro(3), 0.0, INFINITY, xp[3]);
          col_kkt(col(4), kt[4], 0.0, 0.0, ro(10), xp[4]);
          col_kkt(col(5), kt[5], ro(4), ro(11), INFINITY, xp[5]);
          col_kkt(col(6), kt[6], ro(5), ro(12), INFINITY, xp[6]);
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
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int i = row_of(r);
          if (i >= 0) row_kkt(i, kv[r], r < 2 ? ro(13 + r) : 0.0, yp[r], r != 0 && r != 2);
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
      for (int v = 0; v < NC; ++v) x[v] = xa[v] = xim_ld(v);
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) y[rr] = ya[rr] = yim_ld(rr);
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
      xo_g[j] = unscale_x(xim_ld(v), dcv[j], lraw[j], uraw[j]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int i = row_of(r);
      if (i >= 0) yo_g[i] = yim_ld(r) * drv[i];
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

struct HeatArgs {
  Batch b;
  Work w;
  Chunk ch;
  Opts o;
  const int32_t* list;  // global window indices, or null: the chunk
  int gate;             // only the windows whose status is kNeedsEll
};
template <int B>
__global__ __launch_bounds__(B, 3) void pdhg_band_heat_kernel(const HeatArgs args) {
  const int i = blockIdx.x;
  heat_window<B>(args.b, args.w, args.ch, args.o, args.list ? args.list[i] : args.ch.first + i, args.gate, threadIdx.x);
}

}  // namespace

bool band_heat_sized(int64_t n, int64_t m, int64_t meq) {
  const int64_t T = (meq - 1) / 2, J = n - kNC * T;
  return meq >= 5 && (meq & 1) && T <= kHeatB && J >= 0 && J <= kJMax && m - meq >= 3 * T && m - meq <= 4 * T;
}

hipError_t launch_pdhg_band_heat(const Batch& b, const Work& w, const Chunk& ch, const Opts& o, hipStream_t s,
                                 const int32_t* list, int nlist, int* variant_out, bool gate) {
  constexpr int B = kHeatB;
  const size_t lds = heat_lds_bytes(B);
  hipError_t e = hipFuncSetAttribute((const void*)pdhg_band_heat_kernel<B>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds);
  if (e != hipSuccess) return e;
  const int count = list ? nlist : ch.count;
  if (count <= 0) return hipSuccess;
  const HeatArgs args{b, w, ch, o, list, gate ? 1 : 0};
  hipLaunchKernelGGL((pdhg_band_heat_kernel<B>), dim3(count), dim3(B), lds, s, args);
  if (variant_out) *variant_out = 9000000 + 400 + B / kWave;
  return hipGetLastError();
}

}  // namespace dvh
