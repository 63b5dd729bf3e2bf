// Battery cycle wear on one SOE profile, restated so that a device lane computes exactly the bits
// dervet_hip/degradation.py computes on the host: the reversal rule and the three-point rainflow stack of
// oracle/rainflow_ref.py (ASTM E1049-85 section 5.4.4 in the form of the `rainflow` package), the cycle-life table
// lookup and damage sum of degradation.cycle_damage, and the per-battery state update of Degradation.update.
// tests/test_rainflow_native.py checks the host build of this header against both, tests/test_gpu_rainflow.py the
// device build (csrc/dvh_degradation.hip).
//
// Every floating-point operation is one IEEE operation in the order the Python writes it; the translation units that
// include this header are compiled without contraction (the pragma below; g++ builds pass -ffp-contract=off): the
// reversal test is the product d_last * d < 0 as such, and 1.0 - degrade_perc feeds a product that must not fuse.
//
// No runtime calls: included by g++ (tests) and hipcc (device), hence DVH_HD.
#pragma once
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define DVH_HD __host__ __device__
#else
#define DVH_HD
#endif

namespace dvh {
namespace rainflow {

constexpr int kMaxTable = 64;  // cycle-life table rows an entry point accepts

// a < b as numpy sorts doubles (NaN after everything): np.searchsorted's comparison
DVH_HD inline bool np_less(double a, double b) { return a < b || (b != b && a == a); }

// min(np.searchsorted(upper, depth, side="left"), n_table - 1): the first row whose upper limit is >= depth
DVH_HD inline int life_index(const double* upper, int n_table, double depth) {
  int lo = 0, hi = n_table;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (np_less(upper[mid], depth))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n_table - 1 ? lo : n_table - 1;
}

// Running damage sum of one profile: cycles are added in extraction order, one true division each.
struct Damage {
  const double* upper;
  const double* life;
  int n_table;
  double e_rated;
  double sum;
  DVH_HD inline void add(double rng, double count) {
    const double depth = rng / e_rated;
    sum += count / life[life_index(upper, n_table, depth)];
  }
};

// The reversal points of v[0 .. T) (T >= 2), compacted in order to v[0 .. R); returns R >= 2.  The first point, every
// point at which the direction changes (index 1 is the first candidate even when v[1] == v[0]; later runs of equal
// values collapse onto their first point), the last point.  The write index never passes the read index.
DVH_HD inline int reversals_inplace(double* v, int T) {
  double cur = v[1];
  double d_last = v[1] - v[0];
  int w = 1;
  for (int j = 2; j < T; ++j) {
    const double xn = v[j];
    if (xn == cur) continue;
    const double d = xn - cur;
    const double p = d_last * d;  // the product itself: it may underflow to -0, which is not < 0
    if (p < 0.0) v[w++] = cur;
    d_last = d;
    cur = xn;
  }
  v[w++] = v[T - 1];
  return w;
}

// The three-point stack over the reversals r[0 .. R), in place: the live stack r[base .. top) never overtakes the
// read index i.  A range Y that contains the stack's first point is a half cycle (the first point is dropped), any
// other a full cycle (its two points are removed); what is left at the end are half cycles, in order.
template <class Acc>
DVH_HD inline void count_inplace(double* r, int R, Acc& acc) {
  int base = 0, top = 0;
  for (int i = 0; i < R; ++i) {
    const double p = r[i];
    r[top++] = p;
    while (top - base >= 3) {
      const double X = __builtin_fabs(r[top - 1] - r[top - 2]);
      const double Y = __builtin_fabs(r[top - 2] - r[top - 3]);
      if (!(X >= Y)) break;
      if (top - base == 3) {
        acc.add(Y, 0.5);
        ++base;
      } else {
        acc.add(Y, 1.0);
        r[top - 3] = r[top - 1];
        top -= 2;
      }
    }
  }
  for (int k = base; k + 1 < top; ++k) acc.add(__builtin_fabs(r[k + 1] - r[k]), 0.5);
}

// degradation.cycle_damage of one row: v[0 .. T) is used as the work array (overwritten).  T < 2: no cycles.
DVH_HD inline double cycle_damage_inplace(double* v, int T, double e_rated, const double* upper, const double* life,
                                          int n_table) {
  if (T < 2) return 0.0;
  Damage acc{upper, life, n_table, e_rated, 0.0};
  const int R = reversals_inplace(v, T);
  count_inplace(v, R, acc);
  return acc.sum;
}

// Effective energy capacity, Degradation.capacity(): np.maximum(e_rated * (1 - degrade_perc), 0) (a NaN stays NaN).
DVH_HD inline double capacity_of(double e_rated, double degrade_perc) {
  const double c = e_rated * (1.0 - degrade_perc);
  return (c >= 0.0 || c != c) ? c : 0.0;
}

// One battery's state (Degradation's arrays, one element each).
struct State {
  double e_rated, yearly, soh;  // soh: fraction of the rated energy (Degradation.soh)
  int replaceable;
  double degrade_perc;
  int64_t replacements, skipped;
};
struct Step {
  double degradation;  // this window's degradation (update's return value)
  double capacity;     // the capacity the next window is built with (after a replacement: rated)
  int reached;         // the battery reached its state of health in this window (before any replacement)
};

// Degradation.update for one battery after a window of `days` days.  valid: the window's dispatch is usable and
// `cyc` is its cycle damage; otherwise the battery takes the calendar loss only and is counted in skipped.
DVH_HD inline Step state_update(State& s, double days, double eol, int valid, double cyc) {
  double d = s.yearly / 100.0 * (days / 365.0);
  if (valid)
    d = d + cyc * (1.0 - eol / 100.0);
  else
    s.skipped += 1;
  s.degrade_perc += d;
  Step out;
  out.degradation = d;
  out.reached = capacity_of(s.e_rated, s.degrade_perc) <= s.e_rated * s.soh;
  if (out.reached && s.replaceable) {
    s.degrade_perc = 0.0;
    s.replacements += 1;
  }
  out.capacity = capacity_of(s.e_rated, s.degrade_perc);
  return out;
}

}  // namespace rainflow
}  // namespace dvh
