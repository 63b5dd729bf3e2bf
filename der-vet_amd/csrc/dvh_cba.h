// Scenario valuation arithmetic, shared by the device kernels (csrc/dvh_valuation.hip) and the host build the tests
// compile (tests/native/cba_host.cpp): a solved window's bill (retail energy charge, demand charge, DA energy cost,
// variable O&M, ICE fuel, and the "original" bill of the site load alone), and a scenario's pro forma, present values,
// payback and IRR (dervet/CBA.py:215-233, 299-346, 479-523 as far as the Usecase 2 goldens pin them;
// dervet_hip/valuation.py is the numpy form of the same operations).
//
// Every floating-point operation is one IEEE operation in the order written here: the translation units that include
// this header are compiled without contraction (the pragma below, -ffp-contract=off), so that (retail_t dt) net_t is a
// product and then a sum on the host and on the device alike.  Powers are repeated products, never pow().
//
// The bill's sums are formed the way a 256-thread workgroup forms them -- lane l adds the terms t = l, l + 256, ..
// in step order, each wave halves its 64 partials five times (l += l + 32, + 16, ..), the four wave sums are added in
// wave order -- and bill_window() below walks that order serially, so host and device agree bit for bit.
//
// Several opt years (UNPINNED: storagevet's Financial is absent and every golden has one): a year that is not an opt
// year takes the nearest earlier opt year's value times (1 + g)^(years since); years before the first opt year are
// de-escalated from it.  With one opt year this is exactly the golden pro forma rows.
//
// No runtime calls but log(): included by g++ (tests) and hipcc (device), hence DVH_HD.
#pragma once
#include <math.h>

#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#ifndef DVH_HD
#if defined(__HIPCC__)
#define DVH_HD __host__ __device__
#else
#define DVH_HD
#endif
#endif

namespace dvh {
namespace cba {

constexpr int kBillRows = 8;      // DVH_BILL_ROWS
constexpr int kBillMaxJ = 16;     // DVH_BILL_MAX_J
constexpr int kBillLanes = 256;   // threads of a bill workgroup
constexpr int kWaveLanes = 64;
constexpr int kMaxYears = 64;     // DVH_CBA_MAX_YEARS
constexpr int kMaxExtra = 16;     // DVH_CBA_MAX_EXTRA
constexpr int kBillCols = 5;      // bill-derived pro forma columns (each with a growth rate)
constexpr int kFixedCols = 7;     // DVH_CBA_FIXED_COLS: capex, the five bill columns, fixed O&M
constexpr int kValueCols = 7;     // DVH_VALUE_COLS

// bill rows
enum { kRetail = 0, kDemand, kDA, kVarOM, kFuel, kOrigRetail, kOrigDemand, kOrigDA };
// lane sums of a bill
enum { sRetail = 0, sDA, sDis, sElec, sOrigRetail, sOrigDA, kBillSums };
// value columns
enum { vNpv = 0, vPvCost, vPvBenefit, vBcRatio, vPayback, vDiscPayback, vIrr };
// window flags
constexpr int kBadWindow = 1;  // status not OPTIMAL or a needed column outside x: dispatch rows NaN
constexpr int kBadRow = 2;     // a demand-charge row naming no step or no tau column: the row is skipped

DVH_HD inline double qnan() { return __builtin_nan(""); }
DVH_HD inline double neg_inf() { return -__builtin_inf(); }
DVH_HD inline double max2(double a, double b) { return b > a ? b : a; }

// One window's inputs, the series pointers at its own first step.  x: the window's solution [ch, dis, ene, tau, pv?,
// elec?, on?] or [ch, dis, ene, tau, ev_ch, ev_ene], or nullptr when it must not be read (a bad window: original rows only).
struct BillIn {
  int T, J, mI;
  double dt;
  int has_pv, has_ice;
  const int32_t* dcm_t;
  const int32_t* dcm_j;
  const double* base;
  const double* orig;    // never null (the caller substitutes base)
  const double* retail;  // or null
  const double* da;      // or null
  const double* demand;  // [J]
  double om, ice_cost;
  const double* x;
  int has_ev = 0;  // an EV block (ev_ch, ev_ene) after tau; not combined with has_pv / has_ice
  DVH_HD int ipv() const { return 3 * T + J; }
  DVH_HD int ielec() const { return 3 * T + J + (has_pv ? T : 0); }
  // columns the bill reads: a window whose n is below this is bad
  DVH_HD int64_t need() const {
    return 3 * (int64_t)T + J + (has_pv ? T : 0) + (has_ice ? 2 * (int64_t)T : 0) + (has_ev ? 2 * (int64_t)T : 0);
  }
};

// net_t = ((base_t + ch_t) - dis_t) - pv_t - elec_t, or ((base_t + ch_t) - dis_t) + ev_ch_t: adds and subtracts only,
// in this order (in.x != nullptr)
DVH_HD inline double net_load(const BillIn& in, int t) {
  double v = (in.base[t] + in.x[t]) - in.x[in.T + t];
  if (in.has_pv) v = v - in.x[in.ipv() + t];
  if (in.has_ice) v = v - in.x[in.ielec() + t];
  if (in.has_ev) v = v + in.x[in.ipv() + t];
  return v;
}

// Lane `lane` of `lanes`: its partial sums over the steps t = lane, lane + lanes, ..
DVH_HD inline void lane_sums(const BillIn& in, int lane, int lanes, double* s) {
  for (int u = 0; u < kBillSums; ++u) s[u] = 0.0;
  for (int t = lane; t < in.T; t += lanes) {
    const double o = in.orig[t];
    if (in.retail) s[sOrigRetail] += (in.retail[t] * in.dt) * o;
    if (in.da) s[sOrigDA] += (in.da[t] * in.dt) * o;
    if (!in.x) continue;
    const double net = net_load(in, t);
    if (in.retail) s[sRetail] += (in.retail[t] * in.dt) * net;
    if (in.da) s[sDA] += (in.da[t] * in.dt) * net;
    s[sDis] += in.x[in.T + t];
    if (in.has_ice) s[sElec] += in.x[in.ielec() + t];
  }
}

// Lane `lane`: the largest net load / original load over its share of the demand-charge rows of tau column j
// (-inf: none); returns kBadRow when it met a row naming no step or no column (skipped), else 0.
DVH_HD inline int lane_peaks(const BillIn& in, int j, int lane, int lanes, double* peak, double* opeak) {
  double m = neg_inf(), mo = neg_inf();
  int flag = 0;
  for (int i = lane; i < in.mI; i += lanes) {
    const int jj = in.dcm_j[i], t = in.dcm_t[i];
    if (jj < 0 || jj >= in.J || t < 0 || t >= in.T) {
      flag = kBadRow;
      continue;
    }
    if (jj != j) continue;
    mo = max2(mo, in.orig[t]);
    if (in.x) m = max2(m, net_load(in, t));
  }
  *peak = m;
  *opeak = mo;
  return flag;
}

// The rows from the reduced sums and peaks (peaks[j], opeaks[j]: -inf for a column without rows, which then bills
// nothing).  A bad window (in.x == nullptr) gets NaN in its dispatch rows and keeps its original rows.
DVH_HD inline void finish_bill(const BillIn& in, const double* s, double* peaks, const double* opeaks, double* out) {
  double dem = 0.0, odem = 0.0;
  for (int j = 0; j < in.J; ++j) {
    const double po = opeaks[j] == neg_inf() ? 0.0 : opeaks[j];
    odem += in.demand[j] * po;
    if (in.x) {
      const double p = peaks[j] == neg_inf() ? 0.0 : peaks[j];
      peaks[j] = p;
      dem += in.demand[j] * p;
    } else {
      peaks[j] = qnan();
    }
  }
  out[kOrigRetail] = s[sOrigRetail];
  out[kOrigDemand] = odem;
  out[kOrigDA] = s[sOrigDA];
  if (in.x) {
    out[kRetail] = s[sRetail];
    out[kDemand] = dem;
    out[kDA] = s[sDA];
    out[kVarOM] = (in.om / 1000.0 * in.dt) * s[sDis];
    out[kFuel] = in.has_ice ? in.ice_cost * s[sElec] : 0.0;
  } else {
    out[kRetail] = out[kDemand] = out[kDA] = out[kVarOM] = out[kFuel] = qnan();
  }
}

// v[0 .. 256): the workgroup's sum order (see the head of this file); v is overwritten
inline double block_sum(double* v) {
  for (int w = 0; w < kBillLanes / kWaveLanes; ++w)
    for (int o = kWaveLanes / 2; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l) v[w * kWaveLanes + l] += v[w * kWaveLanes + l + o];
  double r = v[0];
  for (int w = 1; w < kBillLanes / kWaveLanes; ++w) r += v[w * kWaveLanes];
  return r;
}

// One window on the host, in the workgroup's order.  out [kBillRows], peaks [J] (scratch when the caller wants none);
// returns the window's flags (kBadWindow when the caller passed x = nullptr).
inline int bill_window(const BillIn& in, double* out, double* peaks) {
  double part[kBillSums][kBillLanes], s[kBillSums], opeaks[kBillMaxJ];
  for (int l = 0; l < kBillLanes; ++l) {
    double ls[kBillSums];
    lane_sums(in, l, kBillLanes, ls);
    for (int u = 0; u < kBillSums; ++u) part[u][l] = ls[u];
  }
  for (int u = 0; u < kBillSums; ++u) s[u] = block_sum(part[u]);
  int flag = in.x ? 0 : kBadWindow;
  for (int j = 0; j < in.J; ++j) {
    double m = neg_inf(), mo = neg_inf();
    for (int l = 0; l < kBillLanes; ++l) {
      double pl, po;
      flag |= lane_peaks(in, j, l, kBillLanes, &pl, &po);
      m = max2(m, pl);
      mo = max2(mo, po);
    }
    peaks[j] = m;
    opeaks[j] = mo;
  }
  if (in.J == 0) {  // the rows are still range-checked
    double pl, po;
    for (int l = 0; l < kBillLanes; ++l) flag |= lane_peaks(in, -1, l, kBillLanes, &pl, &po);
  }
  finish_bill(in, s, peaks, opeaks, out);
  return flag;
}

// ---- scenario valuation

// One scenario's inputs.  bills [n_bills][kBillRows], bad [n_bills] or nullptr; the scenario's windows are the CSR
// entries e0 .. e1 - 1 (already range-checked by the caller), win_idx their bill rows, win_year their pro forma year
// (0 = the first year after the CAPEX row).  opt: the opt years, ascending, each below Y.
struct ValIn {
  int Y, n_opt, n_extra;
  const int32_t* opt;
  double rate;
  const double* growth;  // [kBillCols] %/yr: avoided energy, avoided demand, DA value, variable O&M, fuel
  const double* bills;
  const int32_t* bad;
  int64_t n_bills;
  const int32_t* win_idx;
  const int32_t* win_year;
  int64_t e0, e1;
  double capex, fixed_om;
  const double* extra;  // [n_extra][Y + 1]
};

DVH_HD inline double pw(double b, int k) {
  double r = 1.0;
  for (int i = 0; i < k; ++i) r *= b;
  return r;
}

// bill column b of bill row r as the pro forma carries it: a benefit is original - with-DER, a cost is negative
DVH_HD inline double bill_term(const double* r, int b) {
  switch (b) {
    case 0: return r[kOrigRetail] - r[kRetail];
    case 1: return r[kOrigDemand] - r[kDemand];
    case 2: return r[kOrigDA] - r[kDA];
    case 3: return -r[kVarOM];
    default: return -r[kFuel];
  }
}

// column b summed over the windows of opt year `year`, in CSR order
DVH_HD inline double opt_year_value(const ValIn& a, int b, int year) {
  double v = 0.0;
  for (int64_t e = a.e0; e < a.e1; ++e) {
    const int64_t idx = a.win_idx[e];
    if (a.win_year[e] != year || idx < 0 || idx >= a.n_bills) continue;
    v += bill_term(a.bills + idx * kBillRows, b);
  }
  return v;
}

// NPV's sign at x = 1 + rate: Horner in 1 / x over the yearly net (net[k * ns], k = 0 .. Y)
DVH_HD inline double npv_at(const double* net, int ns, int Y, double x) {
  double acc = net[(int64_t)Y * ns];
  for (int k = Y - 1; k >= 0; --k) acc = acc / x + net[(int64_t)k * ns];
  return acc;
}

DVH_HD inline double bisect_irr(const double* net, int ns, int Y, double lo, double flo, double hi) {
  while (hi - lo > 1e-13) {
    const double mid = 0.5 * (lo + hi);
    if (!(mid > lo && mid < hi)) break;
    const double fm = npv_at(net, ns, Y, mid);
    if (fm == 0.0) return mid - 1.0;
    if ((fm < 0.0) == (flo < 0.0)) {
      lo = mid;
      flo = fm;
    } else {
      hi = mid;
    }
  }
  return 0.5 * (lo + hi) - 1.0;
}

// np.irr's meaning: the real rate above -1 at which the NPV is 0, nearest to rate 0.  Brackets on the fixed grid
// x = 1 + rate = (17/16)^i, i = -128 .. 128 (rates -0.9996 .. 2,345), searched outward from x = 1 (the upper interval
// of a pair first), then bisection to |d rate| <= 1e-13.  NaN when no interval of the grid brackets a sign change.
DVH_HD inline double irr(const double* net, int ns, int Y) {
  constexpr double kStep = 1.0625;
  constexpr int kGrid = 128;
  const double f1 = npv_at(net, ns, Y, 1.0);
  if (f1 == 0.0) return 0.0;
  if (f1 != f1) return qnan();
  double xu = 1.0, fu = f1, xd = 1.0, fd = f1;
  for (int i = 0; i < kGrid; ++i) {
    const double xn = xu * kStep, fn = npv_at(net, ns, Y, xn);
    if (fn == 0.0) return xn - 1.0;
    if (fn != fn) return qnan();
    if ((fn < 0.0) != (fu < 0.0)) return bisect_irr(net, ns, Y, xu, fu, xn);
    xu = xn;
    fu = fn;
    const double xm = xd / kStep, fm = npv_at(net, ns, Y, xm);
    if (fm == 0.0) return xm - 1.0;
    if (fm != fm) return qnan();
    if ((fm < 0.0) != (fd < 0.0)) return bisect_irr(net, ns, Y, xm, fm, xd);
    xd = xm;
    fd = fm;
  }
  return qnan();
}

struct Split {
  double cost, benefit;
  // a column's present value: negative to cost, positive to benefit (the golden cost_benefit rows)
  DVH_HD inline void add(double pv) {
    if (pv != pv) {
      cost = benefit = pv;
    } else if (pv < 0.0) {
      cost += -pv;
    } else if (pv > 0.0) {
      benefit += pv;
    }
  }
};

// One scenario.  net: Y + 1 doubles of work space at stride ns (the yearly net value, left there); out [kValueCols];
// pf: nullptr or the pro forma [Y + 1][kFixedCols + n_extra].  Returns the validity flag: 0 when a window of the
// scenario is flagged, names no bill row or no opt year, or when an opt year has no window.
DVH_HD inline int value_scenario(const ValIn& a, double* net, int ns, double* out, double* pf) {
  const int Y = a.Y, C = kFixedCols + a.n_extra;
  const double x1 = 1.0 + a.rate;
  int valid = 1;
  for (int64_t e = a.e0; e < a.e1; ++e) {
    const int64_t idx = a.win_idx[e];
    if (idx < 0 || idx >= a.n_bills) {
      valid = 0;
      continue;
    }
    if (a.bad && a.bad[idx] != 0) valid = 0;
    bool listed = false;
    for (int o = 0; o < a.n_opt; ++o) listed |= a.opt[o] == a.win_year[e];
    if (!listed) valid = 0;
  }
  for (int o = 0; o < a.n_opt; ++o) {
    bool any = false;
    for (int64_t e = a.e0; e < a.e1; ++e) any |= a.win_year[e] == a.opt[o];
    if (!any) valid = 0;
  }
  Split sp{0.0, 0.0};
  // capital cost: the CAPEX row only
  net[0] = -a.capex;
  for (int k = 1; k <= Y; ++k) net[(int64_t)k * ns] = 0.0;
  if (pf) {
    pf[0] = -a.capex;
    for (int k = 1; k <= Y; ++k) pf[(int64_t)k * C] = 0.0;
  }
  sp.add(-a.capex);
  // the bill columns: opt years from the windows, the others escalated
  for (int b = 0; b < kBillCols; ++b) {
    const double g1 = 1.0 + a.growth[b] / 100.0;
    double pv = 0.0, disc = 1.0, V = 0.0;
    int o = -1;
    if (pf) pf[1 + b] = 0.0;
    for (int y = 0; y < Y; ++y) {
      int on = o < 0 ? 0 : o;
      while (on + 1 < a.n_opt && a.opt[on + 1] <= y) ++on;
      if (on != o) {
        o = on;
        V = opt_year_value(a, b, a.opt[o]);
      }
      const int d = y - a.opt[o];
      const double v = d >= 0 ? V * pw(g1, d) : V / pw(g1, -d);
      disc *= x1;
      pv += v / disc;
      net[(int64_t)(y + 1) * ns] += v;
      if (pf) pf[(int64_t)(y + 1) * C + 1 + b] = v;
    }
    sp.add(pv);
  }
  {  // fixed O&M: every year, unescalated
    double pv = 0.0, disc = 1.0;
    if (pf) pf[kFixedCols - 1] = 0.0;
    for (int k = 1; k <= Y; ++k) {
      const double v = -a.fixed_om;
      disc *= x1;
      pv += v / disc;
      net[(int64_t)k * ns] += v;
      if (pf) pf[(int64_t)k * C + kFixedCols - 1] = v;
    }
    sp.add(pv);
  }
  for (int j = 0; j < a.n_extra; ++j) {  // the caller's columns, verbatim
    double pv = 0.0, disc = 1.0;
    for (int k = 0; k <= Y; ++k) {
      const double v = a.extra[(int64_t)j * (Y + 1) + k];
      if (k > 0) disc *= x1;
      pv += v / disc;
      net[(int64_t)k * ns] += v;
      if (pf) pf[(int64_t)k * C + kFixedCols + j] = v;
    }
    sp.add(pv);
  }
  double npv = 0.0, disc = 1.0;
  for (int k = 0; k <= Y; ++k) {
    if (k > 0) disc *= x1;
    npv += net[(int64_t)k * ns] / disc;
  }
  out[vNpv] = npv;
  out[vPvCost] = sp.cost;
  out[vPvBenefit] = sp.benefit;
  // CBA.benefit_cost_ratio: benefit / cost, NaN when np.isclose(cost, 0)
  out[vBcRatio] = (sp.cost <= 1e-8 && sp.cost >= -1e-8) ? qnan() : sp.benefit / sp.cost;
  const double capex = -net[0], net1 = net[ns];
  double pb = qnan(), dpb = qnan();
  if (net1 > 0.0) {  // (a first year that earns nothing never pays the capital back)
    pb = capex / net1;
    if (a.rate == 0.0) {
      dpb = pb;
    } else {
      const double arg = 1.0 - capex * a.rate / net1;
      if (arg > 0.0) dpb = ::log(1.0 / arg) / ::log(x1);
    }
  }
  out[vPayback] = pb;
  out[vDiscPayback] = dpb;
  out[vIrr] = irr(net, ns, Y);
  return valid;
}

}  // namespace cba
}  // namespace dvh
