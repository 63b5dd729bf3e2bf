// Host build of csrc/dvh_cba.h, the arithmetic the valuation kernels run (csrc/dvh_valuation.hip).
//
// As a shared object (tests/test_valuation_native.py, g++ -O2 -ffp-contract=off): cba_bill_group and cba_value run
// the routines over numpy arrays, compared with dervet_hip/valuation.py's host form.
// As a program (-DCBA_MAIN, built with -fsanitize=address,undefined -fno-sanitize-recover=all): the same routines over
// heap buffers of exactly the sizes the entry points document, so that a read or write past one is a report, then the
// entry points' argument validation (csrc/dvh_valuation_validate.h) over malformed calls; every refusal is printed as
// "<case> err=<message>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dvh_cba.h"
#include "dvh_valuation_validate.h"

using namespace dvh;

extern "C" void cba_bill_group(int T, int J, int G, int mI, double dt, int has_pv, int has_ice, const int32_t* dcm_t,
                               const int32_t* dcm_j, const double* base, const double* orig, const double* retail,
                               const double* da, const double* demand, const double* om, const double* ice_cost,
                               const double* x, int64_t n, const int32_t* status, double* bills, double* peaks,
                               int32_t* bad) {
  for (int g = 0; g < G; ++g) {
    cba::BillIn in;
    in.T = T;
    in.J = J;
    in.mI = mI;
    in.dt = dt;
    in.has_pv = has_pv;
    in.has_ice = has_ice;
    in.dcm_t = dcm_t;
    in.dcm_j = dcm_j;
    in.base = base + (int64_t)g * T;
    in.orig = orig ? orig + (int64_t)g * T : in.base;
    in.retail = retail ? retail + (int64_t)g * T : nullptr;
    in.da = da ? da + (int64_t)g * T : nullptr;
    in.demand = demand + (int64_t)g * J;
    in.om = om ? om[g] : 0.0;
    in.ice_cost = has_ice ? ice_cost[g] : 0.0;
    const bool ok = n >= in.need() && (!status || status[g] == 0);
    in.x = ok ? x + (int64_t)g * n : nullptr;
    double pk[cba::kBillMaxJ];
    bad[g] = cba::bill_window(in, bills + (int64_t)g * cba::kBillRows, pk);
    for (int j = 0; j < J; ++j) peaks[(int64_t)g * J + j] = pk[j];
  }
}

extern "C" void cba_value(int S, int Y, int n_opt, int n_extra, const int32_t* opt, double rate, const double* growth,
                          const double* bills, const int32_t* bad, int64_t n_bills, const int64_t* win_ptr,
                          const int32_t* win_idx, const int32_t* win_year, const double* capex, const double* fixed_om,
                          const double* extra, double* values, int32_t* valid, double* pf) {
  const int C = cba::kFixedCols + n_extra;
  std::vector<double> net(Y + 1);
  for (int s = 0; s < S; ++s) {
    cba::ValIn in{Y,     n_opt,   n_extra,  opt,        rate,           growth,   bills,       bad,
                  n_bills, win_idx, win_year, win_ptr[s], win_ptr[s + 1], capex[s], fixed_om[s], extra};
    valid[s] = cba::value_scenario(in, net.data(), 1, values + (int64_t)s * cba::kValueCols,
                                   pf ? pf + (int64_t)s * (Y + 1) * C : nullptr);
  }
}

#ifdef CBA_MAIN
static int failures = 0;

static void refused(const char* name, const std::string& msg) {
  std::printf("%s err=%s\n", name, msg.c_str());
  if (msg.empty()) ++failures;
}
static void accepted(const char* name, const std::string& msg) {
  if (!msg.empty()) {
    std::printf("%s unexpectedly refused: %s\n", name, msg.c_str());
    ++failures;
  }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uni(double lo, double hi) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}
template <class T>
static T* heap(size_t n) {
  return new T[n ? n : 1];
}

// one group with every block, heap buffers of exactly the documented sizes
static void run_bills(int T, int J, int G, int has_pv, int has_ice) {
  std::vector<int32_t> rt, rj;
  for (int j = 0; j < J; ++j)
    for (int t = j; t < T; t += j + 1) {  // overlapping masks
      rt.push_back(t);
      rj.push_back(j);
    }
  const int mI = (int)rt.size();
  const int64_t n = 3 * (int64_t)T + J + (has_pv ? T : 0) + (has_ice ? 2 * T : 0);
  int32_t *dt_ = heap<int32_t>(mI), *dj = heap<int32_t>(mI), *status = heap<int32_t>(G), *bad = heap<int32_t>(G);
  for (int i = 0; i < mI; ++i) {
    dt_[i] = rt[i];
    dj[i] = rj[i];
  }
  double *base = heap<double>((size_t)G * T), *orig = heap<double>((size_t)G * T), *retail = heap<double>((size_t)G * T),
         *da = heap<double>((size_t)G * T), *demand = heap<double>((size_t)G * J), *om = heap<double>(G),
         *ice = heap<double>(G), *x = heap<double>((size_t)G * n), *bills = heap<double>((size_t)G * cba::kBillRows),
         *peaks = heap<double>((size_t)G * J);
  for (int64_t i = 0; i < (int64_t)G * T; ++i) {
    base[i] = uni(-50, 200);
    orig[i] = uni(100, 300);
    retail[i] = uni(0.05, 0.3);
    da[i] = uni(0.01, 0.1);
  }
  for (int i = 0; i < G * J; ++i) demand[i] = uni(5, 20);
  for (int g = 0; g < G; ++g) {
    om[g] = uni(0, 5);
    ice[g] = uni(0.1, 0.4);
    status[g] = g % 3 == 1 ? 3 : 0;
  }
  for (int64_t i = 0; i < G * n; ++i) x[i] = uni(0, 40);
  cba_bill_group(T, J, G, mI, 0.25, has_pv, has_ice, dt_, dj, base, orig, retail, da, demand, om, ice, x, n, status,
                 bills, peaks, bad);
  for (int g = 0; g < G; ++g) {
    const double* r = bills + (int64_t)g * cba::kBillRows;
    const bool isbad = status[g] != 0;
    if (bad[g] != (isbad ? 1 : 0)) ++failures;
    if ((r[cba::kRetail] != r[cba::kRetail]) != isbad) ++failures;
    if (!(r[cba::kOrigRetail] > 0.0) || (J > 0 && !(r[cba::kOrigDemand] > 0.0))) ++failures;
  }
  // a window one column short of what the layout needs is bad, and is not read: x of G * (n - 1)
  double* xs = heap<double>((size_t)G * (n - 1));
  for (int64_t i = 0; i < G * (n - 1); ++i) xs[i] = 1.0;
  cba_bill_group(T, J, G, mI, 0.25, has_pv, has_ice, dt_, dj, base, nullptr, retail, nullptr, demand, nullptr, ice, xs,
                 n - 1, nullptr, bills, peaks, bad);
  for (int g = 0; g < G; ++g)
    if (bad[g] != 1) ++failures;
  delete[] xs;
  delete[] dt_;
  delete[] dj;
  delete[] status;
  delete[] bad;
  delete[] base;
  delete[] orig;
  delete[] retail;
  delete[] da;
  delete[] demand;
  delete[] om;
  delete[] ice;
  delete[] x;
  delete[] bills;
  delete[] peaks;
}

static void run_values(int S, int Y, int n_extra, int per) {
  const int n_opt = Y >= 4 ? 2 : 1;
  int32_t* opt = heap<int32_t>(n_opt);
  opt[0] = Y >= 4 ? 1 : 0;
  if (n_opt == 2) opt[1] = 3;
  const int64_t nw = (int64_t)S * per * n_opt, nb = nw + 1;
  int64_t* ptr = heap<int64_t>(S + 1);
  int32_t *idx = heap<int32_t>(nw), *yr = heap<int32_t>(nw), *bad = heap<int32_t>(nb), *valid = heap<int32_t>(S);
  double *bills = heap<double>((size_t)nb * cba::kBillRows), *capex = heap<double>(S), *fom = heap<double>(S),
         *extra = heap<double>((size_t)n_extra * (Y + 1)), *values = heap<double>((size_t)S * cba::kValueCols),
         *pf = heap<double>((size_t)S * (Y + 1) * (cba::kFixedCols + n_extra));
  double growth[cba::kBillCols] = {2.2, 2.2, 0.0, 3.0, -1.0};
  for (int64_t i = 0; i < nb * cba::kBillRows; ++i) bills[i] = uni(100, 5000);
  for (int64_t i = 0; i < nb; ++i) bad[i] = 0;
  for (int s = 0; s <= S; ++s) ptr[s] = (int64_t)s * per * n_opt;
  for (int64_t e = 0; e < nw; ++e) {
    idx[e] = (int32_t)((e * 7) % nb);  // scattered
    yr[e] = opt[(e % (per * n_opt)) / per];
  }
  for (int s = 0; s < S; ++s) {
    capex[s] = s % 5 == 4 ? 0.0 : uni(1e3, 1e6);
    fom[s] = uni(0, 1e3);
  }
  for (int i = 0; i < n_extra * (Y + 1); ++i) extra[i] = uni(-100, 300);
  if (nb > 3) bad[3] = 1;
  cba_value(S, Y, n_opt, n_extra, opt, 0.06, growth, bills, bad, nb, ptr, idx, yr, capex, fom, extra, values, valid, pf);
  for (int s = 0; s < S; ++s)
    if (!(values[(int64_t)s * cba::kValueCols + cba::vNpv] == values[(int64_t)s * cba::kValueCols + cba::vNpv])) ++failures;
  cba_value(S, Y, n_opt, n_extra, opt, 0.0, growth, bills, nullptr, nb, ptr, idx, yr, capex, fom, extra, values, valid,
            nullptr);
  delete[] opt;
  delete[] ptr;
  delete[] idx;
  delete[] yr;
  delete[] bad;
  delete[] valid;
  delete[] bills;
  delete[] capex;
  delete[] fom;
  delete[] extra;
  delete[] values;
  delete[] pf;
}

int main() {
  for (int T : {1, 2, 63, 64, 65, 255, 256, 257, 744})
    for (int J : {0, 1, 3}) run_bills(T, J, 3, J == 1, J == 3 || T == 65);
  run_bills(24, cba::kBillMaxJ, 2, 1, 1);
  for (int Y : {1, 21, 64}) run_values(Y == 21 ? 65 : 3, Y, Y == 21 ? 3 : 0, 12);
  run_values(2, cba::kMaxYears, cba::kMaxExtra, 1);

  // the argument validation (what the entry points run before a launch); the pointers are never dereferenced
  double d = 0.0;
  int32_t i32 = 0;
  int64_t i64 = 0;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  dvh_packed b;
  std::memset(&b, 0, sizeof b);
  b.count = 5;
  b.total_n = 5 * 37;
  b.desc = &i64;
  b.x = &d;
  b.istats = &i32;
  dvh_bill_group g;
  std::memset(&g, 0, sizeof g);
  g.T = 12;
  g.J = 1;
  g.G = 5;
  g.mI = 12;
  g.dt = 1.0;
  g.dcm_t = g.dcm_j = &i32;
  g.base = g.demand = &d;
  accepted("bill_ok", validate_bill_windows(&g, &b, 0, &d, &i32));
  {
    dvh_bill_group e = g;
    e.G = 0;
    accepted("bill_empty", validate_bill_windows(&e, &b, 5, nullptr, nullptr));
  }
  refused("bill_null_group", validate_bill_windows(nullptr, &b, 0, &d, &i32));
  refused("bill_null_batch", validate_bill_windows(&g, nullptr, 0, &d, &i32));
  refused("bill_null_bills", validate_bill_windows(&g, &b, 0, nullptr, &i32));
  refused("bill_null_bad", validate_bill_windows(&g, &b, 0, &d, nullptr));
  refused("bill_negative_first", validate_bill_windows(&g, &b, -1, &d, &i32));
  refused("bill_past_batch", validate_bill_windows(&g, &b, 1, &d, &i32));
#define BILL_WITH(name, stmt)                                  \
  {                                                            \
    dvh_bill_group e = g;                                      \
    dvh_packed b2 = b;                                         \
    stmt;                                                      \
    refused(name, validate_bill_windows(&e, &b2, 0, &d, &i32)); \
  }
  BILL_WITH("bill_negative_G", e.G = -1)
  BILL_WITH("bill_first_overflow", e.G = 2147483647)
  BILL_WITH("bill_T0", e.T = 0)
  BILL_WITH("bill_negative_J", e.J = -1)
  BILL_WITH("bill_negative_mI", e.mI = -3)
  BILL_WITH("bill_dt0", e.dt = 0.0)
  BILL_WITH("bill_dt_nan", e.dt = nan)
  BILL_WITH("bill_null_base", e.base = nullptr)
  BILL_WITH("bill_null_rows", e.dcm_t = nullptr)
  BILL_WITH("bill_null_demand", e.demand = nullptr)
  BILL_WITH("bill_null_ice_cost", e.has_ice = 1)
  BILL_WITH("bill_null_x", b2.x = nullptr)
  BILL_WITH("bill_null_desc", b2.desc = nullptr)
  BILL_WITH("bill_null_istats", b2.istats = nullptr)

  int32_t opt[2] = {0, 2};
  int64_t ptr[4] = {0, 2, 4, 6};
  dvh_valuation v;
  std::memset(&v, 0, sizeof v);
  v.S = 3;
  v.Y = 4;
  v.n_opt = 2;
  v.n_extra = 1;
  v.n_win = 6;
  v.n_bills = 6;
  v.opt_years = opt;
  v.win_ptr_host = ptr;
  v.win_ptr = &i64;
  v.win_idx = v.win_year = &i32;
  v.bills = v.capex = v.fixed_om = v.extra = &d;
  v.rate = 0.06;
  accepted("value_ok", validate_value_scenarios(&v, &d, &i32));
  refused("value_null", validate_value_scenarios(nullptr, &d, &i32));
  refused("value_null_values", validate_value_scenarios(&v, nullptr, &i32));
  refused("value_null_valid", validate_value_scenarios(&v, &d, nullptr));
#define VALUE_WITH(name, stmt)                              \
  {                                                         \
    dvh_valuation e = v;                                    \
    int32_t o2[2] = {0, 2};                                 \
    int64_t p2[4] = {0, 2, 4, 6};                           \
    e.opt_years = o2;                                       \
    e.win_ptr_host = p2;                                    \
    stmt;                                                   \
    refused(name, validate_value_scenarios(&e, &d, &i32));  \
  }
  VALUE_WITH("value_negative_S", e.S = -1)
  VALUE_WITH("value_Y0", e.Y = 0)
  VALUE_WITH("value_Y_long", e.Y = DVH_CBA_MAX_YEARS + 1)
  VALUE_WITH("value_extra_long", e.n_extra = DVH_CBA_MAX_EXTRA + 1)
  VALUE_WITH("value_no_opt", e.n_opt = 0)
  VALUE_WITH("value_null_opt", e.opt_years = nullptr)
  VALUE_WITH("value_opt_past_Y", o2[1] = 4)
  VALUE_WITH("value_opt_negative", o2[0] = -1)
  VALUE_WITH("value_opt_descending", o2[1] = 0)
  VALUE_WITH("value_rate_minus_one", e.rate = -1.0)
  VALUE_WITH("value_rate_nan", e.rate = nan)
  VALUE_WITH("value_rate_inf", e.rate = inf)
  VALUE_WITH("value_growth_nan", e.growth[2] = nan)
  VALUE_WITH("value_ptr_null", e.win_ptr_host = nullptr)
  VALUE_WITH("value_ptr_start", p2[0] = 1)
  VALUE_WITH("value_ptr_not_monotone", p2[2] = 1)
  VALUE_WITH("value_ptr_short", p2[3] = 5)
  VALUE_WITH("value_ptr_long", e.n_win = 5)
  VALUE_WITH("value_null_device_ptr", e.win_ptr = nullptr)
  VALUE_WITH("value_null_capex", e.capex = nullptr)
  VALUE_WITH("value_null_idx", e.win_idx = nullptr)
  VALUE_WITH("value_null_bills", e.bills = nullptr)
  VALUE_WITH("value_null_extra", e.extra = nullptr)
  std::printf("failures=%d\ndone\n", failures);
  return failures ? 1 : 0;
}
#endif
