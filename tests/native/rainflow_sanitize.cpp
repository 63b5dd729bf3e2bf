// Stand-alone run of csrc/dvh_rainflow.h and csrc/dvh_degradation_validate.h under AddressSanitizer / UBSan
// (tests/test_rainflow_native.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all).
//
//   rainflow_sanitize <in> <out>
// in:  doubles {n_table, upper[n_table], life[n_table], rows, then per row: T, e_rated, x[T]}
// out: the rows' damages (doubles), each counted in a heap buffer of exactly T values, so that a read or write past
//      the profile is a report.  Then the state update runs over a few batteries and the argument validation over
//      malformed calls; every refusal is printed as "<case> err=<message>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "dvh_degradation_validate.h"
#include "dvh_rainflow.h"

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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> in;
  double buf[512];
  for (size_t k; (k = std::fread(buf, sizeof(double), 512, f)) > 0;) in.insert(in.end(), buf, buf + k);
  std::fclose(f);
  size_t p = 0;
  const int n_table = (int)in.at(p++);
  std::vector<double> upper(in.begin() + p, in.begin() + p + n_table);
  p += n_table;
  std::vector<double> life(in.begin() + p, in.begin() + p + n_table);
  p += n_table;
  const int rows = (int)in.at(p++);
  std::vector<double> out;
  for (int r = 0; r < rows; ++r) {
    const int T = (int)in.at(p++);
    const double e = in.at(p++);
    double* v = new double[T > 0 ? T : 1];  // exactly the profile (one slot when it is empty)
    for (int j = 0; j < T; ++j) v[j] = in.at(p++);
    out.push_back(dvh::rainflow::cycle_damage_inplace(v, T, e, upper.data(), life.data(), n_table));
    delete[] v;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);

  // the state update: wear a battery past its state of health, replaceable or not, with an invalid window between
  for (int rep = 0; rep < 2; ++rep) {
    dvh::rainflow::State s{1000.0, 2.0, 0.8, rep, 0.0, 0, 0};
    for (int k = 0; k < 400; ++k) {
      const dvh::rainflow::Step o = dvh::rainflow::state_update(s, 30.5, 80.0, k % 7 != 3, 0.004);
      if (!(o.capacity >= 0.0 && o.capacity <= 1000.0)) ++failures;
    }
    if (s.skipped != 57 || (rep == 1) != (s.replacements > 0)) ++failures;
  }

  // the argument validation (what the entry points run before a launch); the pointers are never dereferenced
  double d = 0.0;
  int32_t i32 = 0;
  int64_t i64 = 0;
  const void* ok = &d;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  accepted("damage_ok", dvh::validate_cycle_damage(ok, 10, 3, 10, ok, ok, ok, 11, ok));
  accepted("damage_empty", dvh::validate_cycle_damage(nullptr, 0, 0, 0, nullptr, ok, ok, 1, nullptr));
  accepted("damage_T0", dvh::validate_cycle_damage(nullptr, 0, 4, 0, ok, ok, ok, 1, ok));
  refused("damage_negative_S", dvh::validate_cycle_damage(ok, 10, -1, 10, ok, ok, ok, 11, ok));
  refused("damage_negative_T", dvh::validate_cycle_damage(ok, 10, 3, -2, ok, ok, ok, 11, ok));
  refused("damage_short_stride", dvh::validate_cycle_damage(ok, 9, 3, 10, ok, ok, ok, 11, ok));
  refused("damage_null_ene", dvh::validate_cycle_damage(nullptr, 10, 3, 10, ok, ok, ok, 11, ok));
  refused("damage_null_rated", dvh::validate_cycle_damage(ok, 10, 3, 10, nullptr, ok, ok, 11, ok));
  refused("damage_null_out", dvh::validate_cycle_damage(ok, 10, 3, 10, ok, ok, ok, 11, nullptr));
  refused("damage_null_upper", dvh::validate_cycle_damage(ok, 10, 3, 10, ok, nullptr, ok, 11, ok));
  refused("damage_null_life", dvh::validate_cycle_damage(ok, 10, 3, 10, ok, ok, nullptr, 11, ok));
  refused("damage_empty_table", dvh::validate_cycle_damage(ok, 10, 3, 10, ok, ok, ok, 0, ok));
  refused("damage_long_table", dvh::validate_cycle_damage(ok, 10, 3, 10, ok, ok, ok, DVH_RAINFLOW_MAX_TABLE + 1, ok));

  dvh_packed b;
  std::memset(&b, 0, sizeof b);
  b.count = 5;
  b.total_n = 5 * 37;
  b.desc = &i64;
  b.x = &d;
  b.istats = &i32;
  dvh_degradation_state st;
  std::memset(&st, 0, sizeof st);
  st.incl_cycle_degrade = 1;
  st.e_rated = st.yearly = st.soh = &d;
  st.replaceable = &i32;
  st.degrade_perc = st.capacity = st.degradation = &d;
  st.replacements = st.skipped = &i64;
  st.reached = &i32;
  accepted("update_ok", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  accepted("update_part", dvh::validate_degradation_update(&b, 2, 3, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_null_batch", dvh::validate_degradation_update(nullptr, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_null_state", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, nullptr));
  refused("update_negative_S", dvh::validate_degradation_update(&b, 0, -5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_negative_T", dvh::validate_degradation_update(&b, 0, 5, -1, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_negative_col", dvh::validate_degradation_update(&b, 0, 5, 12, -24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_negative_first", dvh::validate_degradation_update(&b, -1, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_past_batch", dvh::validate_degradation_update(&b, 1, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_first_overflow",
          dvh::validate_degradation_update(&b, 2147483647, 2147483647, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_past_columns", dvh::validate_degradation_update(&b, 0, 5, 12, 180, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_col_overflow",
          dvh::validate_degradation_update(&b, 0, 5, 2147483647, 2147483647, 0.5, 80.0, ok, ok, 11, &st));
  refused("update_nan_days", dvh::validate_degradation_update(&b, 0, 5, 12, 24, nan, 80.0, ok, ok, 11, &st));
  refused("update_inf_days", dvh::validate_degradation_update(&b, 0, 5, 12, 24, inf, 80.0, ok, ok, 11, &st));
  refused("update_nan_eol", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, nan, ok, ok, 11, &st));
  refused("update_long_table", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 65, &st));
  refused("update_null_table", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, 80.0, nullptr, ok, 11, &st));
  {
    dvh_packed b2 = b;
    b2.x = nullptr;
    refused("update_null_x", dvh::validate_degradation_update(&b2, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
    b2 = b;
    b2.istats = nullptr;
    refused("update_null_istats", dvh::validate_degradation_update(&b2, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &st));
    dvh_degradation_state s2 = st;
    s2.capacity = nullptr;
    refused("update_null_capacity", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &s2));
    s2 = st;
    s2.skipped = nullptr;
    refused("update_null_skipped", dvh::validate_degradation_update(&b, 0, 5, 12, 24, 0.5, 80.0, ok, ok, 11, &s2));
  }
  std::printf("failures=%d\ndone\n", failures);
  return failures ? 1 : 0;
}
