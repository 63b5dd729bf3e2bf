// Stand-alone driver of the economic-sizing arithmetic (der-vet_amd/csrc/dvh_value_cut.h) and of the entry points'
// argument validation (dvh_value_sizing_validate.h) under AddressSanitizer / UBSan
// (tests/test_value_sizing_native.py):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I der-vet_amd/csrc value_cut_sanitize.cpp
// Builds seeded battery windows of several shapes in exactly-sized heap arrays, cuts them, solves seeded masters, and
// feeds the validators malformed arguments.  Prints one line per check and "failures=N", then "done".
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "dvh_value_cut.h"
#include "dvh_value_sizing_validate.h"

using namespace dvh;

namespace {

int failures = 0;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uni() {  // xorshift64*, (0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return ((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-12;
}

void check(const char* name, bool ok) {
  std::printf("%s %s\n", name, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

// one window of the battery pattern, T steps, J periods that split the steps evenly, every step in one period
void cut_window(int T, int J, bool with_emax, bool break_pattern) {
  const int mI = J ? T : 0, n = 3 * T + J, m = T + 1 + mI, nnz = 4 * T + 3 * mI;
  std::vector<int32_t> dcm_t(mI), dcm_j(mI), ix(nnz);
  std::vector<double> dv(nnz), c(n), l(n), u(n), q(m), x(n), y(m), emax(T), z(T);
  const double dt = 1.0, eta = 0.9, sdr = 0.001, E = 100.0 * uni(), P = 30.0 * uni();
  ix[0] = 2 * T;
  dv[0] = 1.0;
  const int fin = 1 + 4 * (T - 1);
  for (int t = 0; t < T - 1; ++t) {
    const int p = 1 + 4 * t;
    ix[p] = t; ix[p + 1] = T + t; ix[p + 2] = 2 * T + t; ix[p + 3] = 2 * T + t + 1;
    dv[p] = -dt * eta; dv[p + 1] = dt; dv[p + 2] = -(1.0 - dt * sdr); dv[p + 3] = 1.0;
  }
  ix[fin] = T - 1; ix[fin + 1] = 2 * T - 1; ix[fin + 2] = 3 * T - 1;
  dv[fin] = dt * eta; dv[fin + 1] = -dt; dv[fin + 2] = 1.0 - dt * sdr;
  for (int i = 0; i < mI; ++i) {
    const int p = fin + 3 + 3 * i;
    dcm_t[i] = i;
    dcm_j[i] = (int)((int64_t)i * J / T);
    ix[p] = i; ix[p + 1] = T + i; ix[p + 2] = 3 * T + dcm_j[i];
    dv[p] = -1.0; dv[p + 1] = 1.0; dv[p + 2] = 1.0;
  }
  if (break_pattern && mI > 1) { dcm_t[1] = dcm_t[0]; ix[fin + 3 + 3] = dcm_t[0]; ix[fin + 3 + 4] = T + dcm_t[0]; }
  for (int j = 0; j < n; ++j) {
    c[j] = j < 2 * T ? uni() - 0.5 : (j < 3 * T ? 0.0 : 10.0 * uni());
    l[j] = j < 3 * T ? 0.0 : -std::numeric_limits<double>::infinity();
    u[j] = j < 2 * T ? P : (j < 3 * T ? E : std::numeric_limits<double>::infinity());
    x[j] = uni();
  }
  for (int t = 0; t < T; ++t) emax[t] = E * (0.5 + uni());
  for (int i = 0; i < m; ++i) { q[i] = uni(); y[i] = uni() - 0.3; }
  vc::CutIn in;
  in.T = T; in.J = J; in.mI = mI;
  in.dcm_t = dcm_t.data(); in.dcm_j = dcm_j.data(); in.ix = ix.data(); in.dv = dv.data();
  in.c = c.data(); in.l = l.data(); in.u = u.data(); in.q = q.data(); in.x = x.data(); in.y = y.data();
  in.c0 = 3.0; in.E = E; in.P = P; in.soc_target = 0.5; in.llsoc = 0.0; in.ulsoc = 1.0;
  in.emax = with_emax ? emax.data() : nullptr;
  double out[vc::kCutCols];
  vc::window_cut(in, z.data(), out);
  char name[96];
  std::snprintf(name, sizeof name, "cut_T%d_J%d_emax%d_broken%d", T, J, (int)with_emax, (int)break_pattern);
  const bool bad = break_pattern && mI > 1;
  check(name, bad ? (out[vc::cFlag] == vc::kBadPattern && out[vc::cA] != out[vc::cA])
                  : (out[vc::cFlag] == 0.0 && vc::finite(out[vc::cA]) && out[vc::cGP] <= 0.0));
}

void master(int n, bool duplicates) {
  std::vector<double> cut(3 * (size_t)n);
  for (int k = 0; k < n; ++k) {
    const int src = duplicates && k > 0 && k % 2 ? k - 1 : k;
    if (src != k) {
      for (int u = 0; u < 3; ++u) cut[3 * k + u] = cut[3 * src + u];
      continue;
    }
    cut[3 * k] = 100.0 * uni();
    cut[3 * k + 1] = -2.0 * uni();
    cut[3 * k + 2] = -3.0 * uni();
  }
  vc::MasterIn in;
  in.n = n; in.cut = cut.data(); in.cE = 0.5; in.cP = 0.8; in.alpha = 2.0;
  in.Elo = 0.0; in.Ehi = 50.0; in.Plo = 0.0; in.Phi = 20.0;
  double out[4];
  const int rc = vc::master_solve(in, out);
  bool ok = rc == vc::kMasterOk && out[0] >= 0.0 && out[0] <= 50.0 && out[1] >= 0.0 && out[1] <= 20.0;
  for (int k = 0; ok && k < n; ++k)
    ok = out[2] >= cut[3 * k] + cut[3 * k + 1] * out[0] + cut[3 * k + 2] * out[1] - 1e-9 * (1.0 + std::fabs(out[2]));
  char name[64];
  std::snprintf(name, sizeof name, "master_n%d_dup%d", n, (int)duplicates);
  check(name, ok);
}

void refuse(const char* name, const std::string& msg, int code, int want) {
  std::printf("%s rc=%d err=%s\n", name, msg.empty() ? 0 : code, msg.c_str());
  if (msg.size() < 8 || code != want) ++failures;
}

// (the message first: the validator sets the code it goes with)
void refuse_cuts(const char* name, const dvh_battery_group* g, const dvh_packed* b, int32_t first, const void* out,
                 int want) {
  int code = 0;
  const std::string msg = validate_value_cuts(g, b, first, out, &code);
  refuse(name, msg, code, want);
}

}  // namespace

int main() {
  for (int T : {1, 2, 25, 192, 257, 769})
    for (int J : {0, 1, 4}) {
      cut_window(T, J, false, false);
      cut_window(T, J, true, false);
    }
  cut_window(25, 1, false, true);
  for (int n : {1, 2, 3, 64, 256}) {
    master(n, false);
    master(n, true);
  }
  // ---- the validators
  dvh_battery_group g{};
  dvh_packed b{};
  double dummy = 0.0;
  g.T = 4; g.G = 1;
  b.count = 1;
  refuse_cuts("cuts_null_group", nullptr, &b, 0, &dummy, DVH_ERR_ARG);
  refuse_cuts("cuts_null_batch", &g, nullptr, 0, &dummy, DVH_ERR_ARG);
  refuse_cuts("cuts_null_out", &g, &b, 0, nullptr, DVH_ERR_ARG);
  refuse_cuts("cuts_null_arrays", &g, &b, 0, &dummy, DVH_ERR_ARG);
  refuse_cuts("cuts_negative_first", &g, &b, -1, &dummy, DVH_ERR_ARG);
  refuse_cuts("cuts_past_batch", &g, &b, 1, &dummy, DVH_ERR_ARG);
  g.T = 0;
  refuse_cuts("cuts_zero_steps", &g, &b, 0, &dummy, DVH_ERR_ARG);
  g.T = 4;
  g.has_ice = 1;
  refuse_cuts("cuts_ice", &g, &b, 0, &dummy, DVH_ERR_UNSUPPORTED);
  g.has_ice = 0;
  g.has_emin = 1;
  refuse_cuts("cuts_emin", &g, &b, 0, &dummy, DVH_ERR_UNSUPPORTED);
  g.has_emin = 0;
  g.J = DVH_VALUE_MAX_J + 1;
  refuse_cuts("cuts_many_periods", &g, &b, 0, &dummy, DVH_ERR_UNSUPPORTED);

  dvh_value_spec good{};
  good.size_energy = good.size_power = 1;
  good.c_energy = 250.0; good.c_power = 800.0; good.alpha = 14.0;
  good.energy_max = 1e4; good.power_max = 1e3; good.gap_tol = 1e-6; good.max_rounds = 40;
  check("spec_good", validate_value_spec(good, 0).empty());
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  auto spec = [&](const char* name, auto edit) {
    dvh_value_spec s = good;
    edit(s);
    refuse(name, validate_value_spec(s, 0), DVH_ERR_ARG, DVH_ERR_ARG);
  };
  spec("spec_nothing_sized", [](dvh_value_spec& s) { s.size_energy = s.size_power = 0; });
  spec("spec_free_energy", [&](dvh_value_spec& s) { s.energy_max = inf; });
  spec("spec_free_power", [&](dvh_value_spec& s) { s.power_max = inf; });
  spec("spec_zero_energy_cost", [](dvh_value_spec& s) { s.c_energy = 0.0; });
  spec("spec_negative_power_cost", [](dvh_value_spec& s) { s.c_power = -1.0; });
  spec("spec_nan_alpha", [&](dvh_value_spec& s) { s.alpha = nan; });
  spec("spec_zero_gap", [](dvh_value_spec& s) { s.gap_tol = 0.0; });
  spec("spec_no_rounds", [](dvh_value_spec& s) { s.max_rounds = 0; });
  spec("spec_crossed_box", [](dvh_value_spec& s) { s.energy_min = 2e4; });
  spec("spec_fixed_power_with_box", [](dvh_value_spec& s) { s.size_power = 0; });

  dvh_value_master_args a{};
  refuse("master_null", validate_value_master(nullptr), DVH_ERR_ARG, DVH_ERR_ARG);
  a.count = 1; a.n_cases = 1; a.W = 1; a.n_cand = 1; a.n_next = 1; a.cut_cap = 64;
  refuse("master_null_arrays", validate_value_master(&a), DVH_ERR_ARG, DVH_ERR_ARG);
  a.n_cand = DVH_VALUE_MAX_CAND + 1;
  refuse("master_many_candidates", validate_value_master(&a), DVH_ERR_ARG, DVH_ERR_ARG);
  a.n_cand = 1;
  a.cut_cap = DVH_VALUE_MAX_CUTS + 1;
  refuse("master_cut_capacity", validate_value_master(&a), DVH_ERR_ARG, DVH_ERR_ARG);
  a.cut_cap = 64;
  a.count = 2;
  refuse("master_count", validate_value_master(&a), DVH_ERR_ARG, DVH_ERR_ARG);
  a.count = 1;
  a.W = 0;
  refuse("master_no_windows", validate_value_master(&a), DVH_ERR_ARG, DVH_ERR_ARG);
  std::printf("failures=%d\ndone\n", failures);
  return failures ? 1 : 0;
}
