// Host build of csrc/dvh_rainflow.h for tests/test_rainflow_native.py (g++ -O2 -ffp-contract=off): the routines the
// device lane runs in dvh_degradation.hip, behind a C interface for ctypes.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "dvh_rainflow.h"

using namespace dvh::rainflow;

extern "C" {

// damage[s] of row s of x[S][stride] (its first T entries), rated energy e[s]; the rows are not modified
void rainflow_damage_rows(const double* x, int S, int T, long long stride, const double* e, const double* upper,
                          const double* life, int n_table, double* damage) {
  std::vector<double> v((std::size_t)(T > 0 ? T : 0));
  for (int s = 0; s < S; ++s) {
    for (int j = 0; j < T; ++j) v[j] = x[(std::size_t)s * stride + j];
    damage[s] = cycle_damage_inplace(v.data(), T, e[s], upper, life, n_table);
  }
}

// the reversal values of x[0 .. T) (T >= 2) to out[0 .. T); returns their number
int rainflow_reversals(const double* x, int T, double* out) {
  for (int j = 0; j < T; ++j) out[j] = x[j];
  return reversals_inplace(out, T);
}

int rainflow_life_index(const double* upper, int n_table, double depth) { return life_index(upper, n_table, depth); }

// Degradation.update for S batteries: state arrays in / out, valid / cyc per battery
void degradation_step(int S, const double* e_rated, const double* yearly, const double* soh, const int32_t* replaceable,
                      double* degrade_perc, int64_t* replacements, int64_t* skipped, double days, double eol,
                      const int32_t* valid, const double* cyc, double* degradation, double* capacity,
                      int32_t* reached) {
  for (int s = 0; s < S; ++s) {
    State b{e_rated[s], yearly[s], soh[s], replaceable[s] != 0, degrade_perc[s], replacements[s], skipped[s]};
    const Step o = state_update(b, days, eol, valid[s], cyc[s]);
    degrade_perc[s] = b.degrade_perc;
    replacements[s] = b.replacements;
    skipped[s] = b.skipped;
    degradation[s] = o.degradation;
    capacity[s] = o.capacity;
    reached[s] = o.reached;
  }
}

}  // extern "C"
