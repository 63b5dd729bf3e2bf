// Host sanitizer driver of the reliability sizing entry points (include/dervet_hip.h: dvh_outage_first_uncovered,
// dvh_sizing_windows, dvh_size_reliability, dvh_last_sizing_ms).  Built with -fsanitize=address,undefined from
// der-vet_amd/csrc/dvh_sizing.cpp and dvh_sizing_validate.cpp (tests/test_sizing_sanitize.py) and run on the CPU: it
// drives the argument validation with a null handle and with malformed cases, specs and starts.  Every call must come
// back DVH_ERR_ARG with a message before anything touches a device, so the handle is a stand-in that carries only what
// dvh_sizing.cpp reads of one (dvh::handle_view), and the launchers and the solve it would reach are stubs that abort.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../der-vet_amd/csrc/dvh_internal.h"
#include "../../include/dervet_hip.h"

struct dvh_handle {
  dvh_options opts{};
  std::string err;
  dvh::SizingState* sizing = nullptr;
};

namespace dvh {
HandleView handle_view(dvh_handle* h) { return HandleView{0, nullptr, &h->opts, &h->err, &h->sizing}; }
static hipError_t unreachable(const char* what) {
  std::printf("FATAL: %s reached: validation let a malformed call through\n", what);
  std::abort();
}
hipError_t launch_outage_first_uncovered(const OutageCase*, int, int, int32_t*, int32_t*, hipStream_t) {
  return unreachable("launch_outage_first_uncovered");
}
hipError_t launch_build_sizing(const SizingLP*, int, const int64_t*, int32_t*, int32_t*, double*, double*, double*,
                               double*, double*, double*, hipStream_t) {
  return unreachable("launch_build_sizing");
}
hipError_t launch_gather_sizes(const int64_t*, const double*, const int32_t*, int, double*, hipStream_t) {
  return unreachable("launch_gather_sizes");
}
}  // namespace dvh
extern "C" int dvh_solve_packed_device(dvh_handle*, const dvh_packed*, void*) {
  dvh::unreachable("dvh_solve_packed_device");
  return DVH_ERR_HIP;
}

static dvh_handle H;
static int failures = 0;

static void report(const char* name, int rc, bool with_handle) {
  std::printf("%s rc=%d err=%s\n", name, rc, with_handle ? H.err.c_str() : "-");
  if (rc != DVH_ERR_ARG || (with_handle && H.err.empty())) ++failures;
  H.err.clear();
}

int main() {
  const int N = 48;
  std::vector<double> cl(N, 500.0), shed(24, 80.0);
  dvh_outage_case good{};
  good.n_steps = N;
  good.max_outage = 24;
  good.dt = 1.0;
  good.critical_load = cl.data();
  good.load_shed_pct = shed.data();
  good.rte = 0.85;
  dvh_sizing_spec spec{};
  spec.target_hours = 4.0;
  spec.size_energy = spec.size_power = 1;
  spec.ccost_kw = 100.0;
  spec.ccost_kwh = 800.0;
  spec.energy_max = spec.power_max = INFINITY;
  spec.ulsoc = 1.0;
  spec.soc_init = 1.0;
  spec.n_seed = 10;
  spec.max_rounds = 256;
  int32_t steps = 4, first = 0, nunc = 0, starts[3] = {0, 5, 47}, ns = 3;
  dvh_result res{};
  dvh_sizing_result sres{};
  double ms = 0.0;

  // ---- null handle: a code, no crash
  report("null_handle_scan", dvh_outage_first_uncovered(nullptr, &good, 1, &steps, &first, &nunc), false);
  report("null_handle_windows", dvh_sizing_windows(nullptr, &good, &spec, 1, starts, &ns, &res), false);
  report("null_handle_loop", dvh_size_reliability(nullptr, &good, &spec, 1, &sres), false);
  report("null_handle_ms", dvh_last_sizing_ms(nullptr, &ms, nullptr), false);
  report("null_ms", dvh_last_sizing_ms(&H, nullptr, nullptr), false);
  if (dvh_last_sizing_ms(&H, &ms, nullptr) != DVH_OK || ms != 0.0) ++failures;  // nothing ran yet
  // empty batches are fine and touch nothing
  if (dvh_outage_first_uncovered(&H, nullptr, 0, nullptr, nullptr, nullptr) != DVH_OK) ++failures;
  if (dvh_sizing_windows(&H, nullptr, nullptr, 0, nullptr, nullptr, nullptr) != DVH_OK) ++failures;
  if (dvh_size_reliability(&H, nullptr, nullptr, 0, nullptr) != DVH_OK) ++failures;

  // ---- the scan
  report("scan_null_cases", dvh_outage_first_uncovered(&H, nullptr, 1, &steps, &first, &nunc), true);
  report("scan_negative_count", dvh_outage_first_uncovered(&H, &good, -1, &steps, &first, &nunc), true);
  report("scan_null_steps", dvh_outage_first_uncovered(&H, &good, 1, nullptr, &first, &nunc), true);
  report("scan_null_out", dvh_outage_first_uncovered(&H, &good, 1, &steps, nullptr, &nunc), true);
  {
    int32_t bad = 0;
    report("scan_zero_steps", dvh_outage_first_uncovered(&H, &good, 1, &bad, &first, &nunc), true);
    bad = 25;
    report("scan_steps_beyond_window", dvh_outage_first_uncovered(&H, &good, 1, &bad, &first, &nunc), true);
    dvh_outage_case c = good;
    c.n_steps = 0;
    report("scan_no_steps", dvh_outage_first_uncovered(&H, &c, 1, &steps, &first, &nunc), true);
    c = good;
    c.critical_load = nullptr;
    report("scan_null_series", dvh_outage_first_uncovered(&H, &c, 1, &steps, &first, &nunc), true);
    c = good;
    c.dt = 0.0;
    report("scan_zero_dt", dvh_outage_first_uncovered(&H, &c, 1, &steps, &first, &nunc), true);
    c.dt = NAN;
    report("scan_nan_dt", dvh_outage_first_uncovered(&H, &c, 1, &steps, &first, &nunc), true);
    c = good;
    c.rte = 0.0;
    report("scan_zero_rte", dvh_outage_first_uncovered(&H, &c, 1, &steps, &first, &nunc), true);
    c = good;
    c.max_outage = 0;
    report("scan_zero_window", dvh_outage_first_uncovered(&H, &c, 1, &steps, &first, &nunc), true);
  }

  // ---- the loop's specs
  auto loop = [&](const char* name, const dvh_sizing_spec& s) {
    report(name, dvh_size_reliability(&H, &good, &s, 1, &sres), true);
  };
  report("loop_null_specs", dvh_size_reliability(&H, &good, nullptr, 1, &sres), true);
  report("loop_null_out", dvh_size_reliability(&H, &good, &spec, 1, nullptr), true);
  report("loop_negative_count", dvh_size_reliability(&H, &good, &spec, -3, &sres), true);
  {
    std::vector<double> nanload(cl);
    nanload[7] = NAN;
    dvh_outage_case c = good;
    c.critical_load = nanload.data();
    report("loop_nan_load", dvh_size_reliability(&H, &c, &spec, 1, &sres), true);
  }
  {
    dvh_sizing_spec s = spec;
    s.size_energy = s.size_power = 0;
    loop("loop_nothing_sized", s);
    s = spec;
    s.ccost_kwh = 0.0;
    loop("loop_free_energy", s);
    s = spec;
    s.ccost_kw = -1.0;
    loop("loop_negative_power_cost", s);
    s = spec;
    s.ccost = NAN;
    loop("loop_nan_cost", s);
    s = spec;
    s.target_hours = 0.0;
    loop("loop_zero_target", s);
    s.target_hours = NAN;
    loop("loop_nan_target", s);
    s.target_hours = 1e300;
    loop("loop_huge_target", s);
    s.target_hours = 25.0;
    loop("loop_target_beyond_window", s);
    s = spec;
    s.energy_min = 10.0;
    s.energy_max = 5.0;
    loop("loop_crossed_energy_bounds", s);
    s = spec;
    s.power_min = -1.0;
    loop("loop_negative_power_min", s);
    s = spec;
    s.size_power = 0;
    s.power = NAN;
    loop("loop_nan_fixed_power", s);
    s = spec;
    s.llsoc = 0.9;
    s.ulsoc = 0.5;
    loop("loop_crossed_soc", s);
    s = spec;
    s.n_seed = 0;
    loop("loop_no_seed", s);
    s = spec;
    s.max_rounds = 0;
    loop("loop_no_rounds", s);
    s.max_rounds = 1 << 20;
    loop("loop_too_many_rounds", s);
  }

  // ---- given starts
  report("windows_null_starts", dvh_sizing_windows(&H, &good, &spec, 1, nullptr, &ns, &res), true);
  report("windows_null_counts", dvh_sizing_windows(&H, &good, &spec, 1, starts, nullptr, &res), true);
  report("windows_null_out", dvh_sizing_windows(&H, &good, &spec, 1, starts, &ns, nullptr), true);
  {
    int32_t zero = 0, bad[3] = {0, -1, 5}, past[3] = {0, 5, 48};
    report("windows_no_starts", dvh_sizing_windows(&H, &good, &spec, 1, starts, &zero, &res), true);
    report("windows_negative_start", dvh_sizing_windows(&H, &good, &spec, 1, bad, &ns, &res), true);
    report("windows_start_past_series", dvh_sizing_windows(&H, &good, &spec, 1, past, &ns, &res), true);
    dvh_sizing_spec s = spec;
    s.ccost_kwh = 0.0;
    report("windows_bad_spec", dvh_sizing_windows(&H, &good, &s, 1, starts, &ns, &res), true);
  }
  std::printf("failures=%d\n%s\n", failures, failures ? "FAILED" : "done");
  return failures ? 1 : 0;
}
