"""SOE-like profiles that exercise every branch of the rainflow counter (shared by tests/test_rainflow_native.py, the
sanitized stand-alone run and tests/test_gpu_rainflow.py), and the scalar oracle they are compared with."""
import numpy as np

from oracle import rainflow_ref


def oracle_damage(series, e_rated, upper, life):
    """oracle/rainflow_ref.cycles + the table lookup, as tests/test_degradation.py::_oracle_damage."""
    d = 0.0
    for r, c in rainflow_ref.cycles(series):
        idx = min(int(np.searchsorted(upper, r / e_rated, side="left")), len(upper) - 1)
        d += c / life[idx]
    return d


def shapes(upper):
    """[(name, profile, rated energy)], profiles of different lengths."""
    rng = np.random.default_rng(11)
    out = [("astm", [-2, 1, -3, 5, -1, 3, -4, 4, -2], 10.0),
           ("T0", [], 7.0), ("T1", [3.0], 7.0), ("T2_up", [1.0, 4.0], 7.0), ("T2_down", [4.0, 1.0], 7.0),
           ("T3_peak", [1.0, 4.0, 2.0], 7.0), ("T3_ramp", [1.0, 2.0, 4.0], 7.0), ("T3_flat_then", [2.0, 2.0, 5.0], 7.0),
           ("five_five", [5.0, 5.0], 10.0),
           ("flat", [1000.0] * 20, 4000.0),
           # x[1] == x[0]: index 1 is still the first "last" point, with d_last = 0
           ("plateau_start", [2, 2, 2, 5, 1, 4, 0, 3], 10.0),
           ("plateau_start_down", [2, 2, 1, 5, 1, 4], 10.0),
           ("plateau_middle", [0, 3, 3, 3, 1, 1, 4, 4, 2, 5], 10.0),
           ("plateau_end", [0, 4, 1, 3, 3, 3], 10.0),
           ("plateau_on_turn", [0, 4, 4, 1, 1, 3, 3, 0], 10.0),
           ("sawtooth", [0.0, 10.0] * 15, 12.0),
           ("sawtooth_growing", [((-1) ** k) * k for k in range(30)], 40.0),
           ("sawtooth_shrinking", [((-1) ** k) * (30 - k) for k in range(30)], 40.0),
           ("ramp", list(range(25)), 30.0),
           ("ramp_down", list(range(25, 0, -1)), 30.0),
           # few levels: X == Y ties take the >= branch, half cycles at depth 3 over and over
           ("quantised", (rng.integers(0, 4, 200) * 100.0).tolist(), 350.0),
           ("quantised_2", (rng.integers(0, 3, 97) * 0.5).tolist(), 1.0),
           # d_last * d underflows to -0, which is not < 0: no turning point although the signs differ
           ("underflow", [0.0, 1e-200, 0.0, 1e-200, 0.0, 1.0, 0.0], 1.0),
           ("above_table", [0.0, 2.0 * float(upper[-1])], 1.0)]
    for i in (0, 3, len(upper) - 1):  # a depth exactly on a table limit (side="left": that row), and just above it
        out.append((f"on_limit_{i}", [0.0, float(upper[i])], 1.0))
        out.append((f"over_limit_{i}", [0.0, float(np.nextafter(upper[i], np.inf))], 1.0))
    return [(n, np.asarray(x, np.float64), float(e)) for n, x, e in out]


def walks(S=40, T=300, seed=5):
    """Random walks with plateaus, a flat row and a sawtooth, per-row rated energy (tests/test_degradation.py's)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(size=(S, T)), axis=1) * 50 + 2000
    x[:, 50:60] = x[:, 49:50]
    x[3] = 1000.0
    x[min(7, S - 1), ::2] += 300.0
    return x, rng.uniform(3000, 6000, S)


def stacked_one_length(upper):
    """The shapes of at least two points as rows of ONE [S, Tmax] array, each continued with its last value (a final
    plateau: the counter sees the same reversals), and their rated energies."""
    sh = [(x, e) for _, x, e in shapes(upper) if len(x) >= 2]
    Tmax = max(len(x) for x, _ in sh)
    return np.stack([np.concatenate([x, np.full(Tmax - len(x), x[-1])]) for x, _ in sh]), np.array([e for _, e in sh])


def stacked(upper):
    """The shapes as rows of one [S, Tmax] array with their lengths (shorter rows padded with NaN, never read) and
    rated energies: rows of one length go to the device in one call."""
    sh = shapes(upper)
    Tmax = max(len(x) for _, x, _ in sh)
    X = np.full((len(sh), Tmax), np.nan)
    for i, (_, x, _) in enumerate(sh):
        X[i, :len(x)] = x
    return X, np.array([len(x) for _, x, _ in sh]), np.array([e for _, _, e in sh]), [n for n, _, _ in sh]
