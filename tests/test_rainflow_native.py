"""The device wear update's arithmetic on the CPU: csrc/dvh_rainflow.h (the routines one lane of dvh_degradation.hip
runs) compiled by g++ through tests/native/rainflow_host.cpp.  Cycle damage is bit-equal to
degradation.cycle_damage and to the scalar oracle (oracle/rainflow_ref.py + the table lookup) on every branch of the
counter, the state update equals Degradation.update field for field, and a stand-alone program drives the same
routines and the entry points' argument validation under AddressSanitizer / UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rainflow_cases
from dervet_hip import degradation
from oracle import rainflow_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "der-vet_amd", "csrc")
UPPER, LIFE = degradation.cycle_life_table()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rainflow") / "rainflow_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC,
                    os.path.join(HERE, "native", "rainflow_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.rainflow_damage_rows.restype = None
    lib.rainflow_damage_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong] + \
        [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    lib.rainflow_reversals.restype = ctypes.c_int
    lib.rainflow_reversals.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.rainflow_life_index.restype = ctypes.c_int
    lib.rainflow_life_index.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    lib.degradation_step.restype = None
    lib.degradation_step.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 7 + [ctypes.c_double, ctypes.c_double] + \
        [ctypes.c_void_p] * 5
    return lib


def native_damage(lib, x, e, upper=UPPER, life=LIFE):
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, np.float64)))
    S, T = x.shape
    e = np.ascontiguousarray(np.broadcast_to(np.asarray(e, np.float64), (S,)))
    keep = x.copy()
    out = np.full(S, np.nan)
    lib.rainflow_damage_rows(_p(x), S, T, max(T, 1), _p(e), _p(upper), _p(life), len(upper), _p(out))
    assert np.array_equal(x, keep, equal_nan=True)
    return out


@pytest.mark.parametrize("name,x,e", rainflow_cases.shapes(UPPER), ids=[s[0] for s in rainflow_cases.shapes(UPPER)])
def test_damage_equals_vectorised_and_scalar_oracle(host, name, x, e):
    got = native_damage(host, x[None, :], e)[0]
    assert got == degradation.cycle_damage(x[None, :], e, UPPER, LIFE)[0]
    assert got == rainflow_cases.oracle_damage(x, e, UPPER, LIFE)
    if len(x) >= 2:  # the reversal values themselves
        r = np.empty(len(x))
        n = host.rainflow_reversals(_p(np.ascontiguousarray(x)), len(x), _p(r))
        assert np.array_equal(r[:n], x[rainflow_ref.reversals(x)])


def test_shapes_reach_the_branches_they_are_named_for():
    """The list is only worth its names if the rows do what they say (checked on the oracle)."""
    sh = {n: (x, e) for n, x, e in rainflow_cases.shapes(UPPER)}
    assert rainflow_ref.count_cycles(sh["astm"][0]) == [(3, 0.5), (4, 1.5), (6, 0.5), (8, 1.0), (9, 0.5)]
    assert rainflow_ref.cycles(sh["T0"][0]) == [] and rainflow_ref.cycles(sh["T1"][0]) == []
    assert rainflow_ref.cycles(sh["flat"][0]) == [(0.0, 0.5)]
    assert rainflow_ref.reversals(sh["underflow"][0]) == [0, 4, 5, 6]   # the tiny turns 1, 2, 3 are not turning points
    assert rainflow_ref.reversals(sh["plateau_start"][0])[:2] == [0, 3]
    q = rainflow_ref.cycles(sh["quantised"][0])
    assert sum(1 for _, c in q if c == 0.5) > 5 and sum(1 for _, c in q if c == 1.0) > 5
    for i in (0, 3, len(UPPER) - 1):
        assert sh[f"on_limit_{i}"][0][1] / 1.0 == UPPER[i]


def test_table_lookup_is_searchsorted_left(host):
    up = np.ascontiguousarray(UPPER)
    depths = np.concatenate([UPPER, np.nextafter(UPPER, np.inf), np.nextafter(UPPER, -np.inf),
                             [0.0, -1.0, 5.0, np.inf, np.nan, -np.inf]])
    for d in depths:
        want = min(int(np.searchsorted(UPPER, d, side="left")), len(UPPER) - 1)
        assert host.rainflow_life_index(_p(up), len(up), float(d)) == want, d
    one = np.array([0.5])
    for d in (0.1, 0.5, 0.9):
        assert host.rainflow_life_index(_p(one), 1, d) == 0


def test_random_walks_with_per_row_energy(host):
    x, E = rainflow_cases.walks()
    got = native_damage(host, x, E)
    assert np.array_equal(got, degradation.cycle_damage(x, E, UPPER, LIFE))
    for i in range(len(x)):
        assert got[i] == rainflow_cases.oracle_damage(x[i], E[i], UPPER, LIFE), i


def test_rows_are_read_through_the_stride(host):
    x, E = rainflow_cases.walks(S=5, T=64)
    out = np.empty(5)
    host.rainflow_damage_rows(_p(x), 5, 41, 64, _p(E), _p(UPPER), _p(LIFE), len(UPPER), _p(out))
    assert np.array_equal(out, degradation.cycle_damage(x[:, :41], E, UPPER, LIFE))


def _native_update(lib, st, days, eol, valid, cyc):
    S = len(st["e_rated"])
    d, cap, reached = np.empty(S), np.empty(S), np.empty(S, np.int32)
    lib.degradation_step(S, _p(st["e_rated"]), _p(st["yearly"]), _p(st["soh"]), _p(st["replaceable"]),
                         _p(st["degrade_perc"]), _p(st["replacements"]), _p(st["skipped"]), days, eol,
                         _p(np.ascontiguousarray(valid, np.int32)), _p(np.ascontiguousarray(cyc)), _p(d), _p(cap),
                         _p(reached))
    return d, cap, reached


def test_state_update_equals_degradation_update(host):
    """30 successive updates: mixed replaceable, row 1 wears out and is replaced (row 2, not replaceable, stays
    worn), one invalid row per update, fractional days."""
    rng = np.random.default_rng(3)
    S, T = 6, 48
    e_rated = np.array([4000.0, 900.0, 900.0, 5200.5, 777.0, 3000.0])
    deg = degradation.Degradation(e_rated, yearly_degrade=[2.0, 1.5, 1.5, 0.0, 3.25, 2.0], state_of_health=[73, 99, 99, 73, 60, 73],
                                  replaceable=[True, True, False, True, False, True], eol_condition=77.5)
    st = dict(e_rated=deg.e_rated.copy(), yearly=deg.yearly.copy(), soh=deg.soh.copy(),
              replaceable=deg.replaceable.astype(np.int32), degrade_perc=np.zeros(S), replacements=np.zeros(S, np.int64),
              skipped=np.zeros(S, np.int64))
    replaced = False
    for k in range(30):
        ene = rng.uniform(0.0, 1.0, (S, T)) * e_rated[:, None]
        ene[1:3] = np.tile([0.0, 900.0], T // 2)       # full cycles: rows 1 and 2 wear fast
        valid = np.ones(S, bool)
        valid[k % S] = False
        days = T / 24.0 + 0.1 * k / 3.0
        cyc = np.where(valid, degradation.cycle_damage(ene, e_rated, UPPER, LIFE), 0.0)
        want_d = deg.update(ene, days, valid=valid, year=2017)
        d, cap, reached = _native_update(host, st, days, deg.eol, valid, cyc)
        assert np.array_equal(d, want_d), k
        assert np.array_equal(st["degrade_perc"], deg.degrade_perc), k
        assert np.array_equal(st["replacements"], deg.replacements) and np.array_equal(st["skipped"], deg.skipped)
        assert np.array_equal(cap, deg.capacity()), k
        replaced |= bool(reached[1])
    assert replaced and deg.replacements[1] >= 1 and deg.replacements[2] == 0
    assert deg.capacity()[2] <= 0.99 * 900.0 and (deg.skipped == 5).all()


def test_state_update_with_the_module_off_is_the_callers_noop():
    """incl_cycle_degrade off: update returns zeros and touches nothing (the entry point writes zeros and the
    unchanged capacity without calling the state update; tests/test_gpu_degradation_resident.py)."""
    deg = degradation.Degradation([1000.0, 2000.0], yearly_degrade=10.0, incl_cycle_degrade=False)
    assert np.array_equal(deg.update(np.tile([0.0, 1000.0], (2, 6)), 12.5), np.zeros(2))
    assert np.array_equal(deg.degrade_perc, np.zeros(2)) and np.array_equal(deg.capacity(), deg.e_rated)


# ---- the same routines and the argument validation, stand-alone under the sanitizers

REFUSED = ["damage_negative_S", "damage_negative_T", "damage_short_stride", "damage_null_ene", "damage_null_rated",
           "damage_null_out", "damage_null_upper", "damage_null_life", "damage_empty_table", "damage_long_table",
           "update_null_batch", "update_null_state", "update_negative_S", "update_negative_T", "update_negative_col",
           "update_negative_first", "update_past_batch", "update_first_overflow", "update_past_columns",
           "update_col_overflow", "update_nan_days", "update_inf_days", "update_nan_eol", "update_long_table",
           "update_null_table", "update_null_x", "update_null_istats", "update_null_capacity", "update_null_skipped"]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("rainflow_asan")
    exe = str(d / "rainflow_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
                        os.path.join(HERE, "native", "rainflow_sanitize.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [(x, e) for _, x, e in rainflow_cases.shapes(UPPER)]
    wx, wE = rainflow_cases.walks()
    rows += list(zip(wx, wE))
    words = [float(len(UPPER)), *UPPER, *LIFE, float(len(rows))]
    for x, e in rows:
        words += [float(len(x)), float(e), *x]
    np.asarray(words, np.float64).tofile(str(d / "in.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, env=env,
                       timeout=120)
    out = np.fromfile(str(d / "out.bin")) if os.path.exists(str(d / "out.bin")) else None
    return p, rows, out


def test_sanitized_run_is_clean(sanitized):
    p, _, _ = sanitized
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    assert p.stdout.rstrip().endswith("done") and "failures=0" in p.stdout


def test_sanitized_run_counts_the_same_damage(sanitized):
    _, rows, out = sanitized
    assert out is not None and len(out) == len(rows)
    for i, (x, e) in enumerate(rows):
        assert out[i] == degradation.cycle_damage(np.asarray(x)[None, :], e, UPPER, LIFE)[0], i


@pytest.mark.parametrize("case", REFUSED)
def test_malformed_call_is_refused_with_a_message(sanitized, case):
    m = re.search(rf"^{case} err=(.*)$", sanitized[0].stdout, re.M)
    assert m and len(m.group(1)) > 8, sanitized[0].stdout[-1500:]
