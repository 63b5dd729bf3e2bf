"""The economic sizing's arithmetic on the CPU: csrc/dvh_value_cut.h (the routines csrc/dvh_value_sizing.hip runs)
compiled by g++ through tests/native/value_cut_host.cpp.  The cuts bit-equal to the numpy restatement
(value_sizing.host_cut, same operations in the same order) and within the forward rounding bound of a long-double
recomputation; the master within HiGHS's feasibility tolerance of scipy's linprog on seeded cut sets; cuts from PDHG
duals (converged and cut short) never above HiGHS's window optimum at other sizes; a stand-alone program drives the
same routines and the entry points' argument validation under AddressSanitizer / UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import value_sizing_cases as C
import value_sizing_ref as R
from dervet_hip import value_sizing as VS
from oracle import pdlp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "der-vet_amd", "csrc")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vc") / "value_cut_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC,
                    os.path.join(HERE, "native", "value_cut_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.vc_window_cuts.restype = None
    lib.vc_window_cuts.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 18
    lib.vc_master.restype = ctypes.c_int
    lib.vc_master.argtypes = [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_double] * 7 + [ctypes.c_void_p]
    return lib


def native_cut(lib, lp, x, y):
    f = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    K = lp["K"]
    ix, dv = np.ascontiguousarray(K.indices, np.int32), f(lp["dv"])
    dt, dj = np.ascontiguousarray(lp["dcm_t"], np.int32), np.ascontiguousarray(lp["dcm_j"], np.int32)
    a = [f(lp[k]) for k in ("c", "l", "u", "q")] + [f(x), f(y)]
    sc = [f([lp[k]]) for k in ("c0", "E", "P", "soc_target", "llsoc", "ulsoc")]
    emax = None if lp["emax"] is None else f(lp["emax"])
    out = np.full(VS.CUT_COLS, -7.0)
    lib.vc_window_cuts(lp["T"], lp["J"], lp["mI"], 1, _p(dt), _p(dj), _p(ix), _p(dv), *[_p(v) for v in a],
                       *[_p(v) for v in sc], _p(emax), _p(out))
    return out


def cut_windows():
    """Seeded windows with a primal / dual pair each: HiGHS's, and random duals (negative >= duals included, which the
    cut clamps)."""
    rng = np.random.default_rng(7)
    out = []
    for T, J, kw in [(2, 0, {}), (2, 1, {}), (25, 1, {}), (25, 4, {}), (48, 1, dict(sdr=0.5)), (192, 4, {}),
                     (300, 0, {}), (300, 1, dict(emax_frac=900.0)), (769, 1, {}), (769, 4, dict(llsoc=0.0, soc_target=1.0, ulsoc=1.0))]:
        s = C.positions([100 + T + J], 1, T, J=J, **kw)[0]
        lp = R.window_lp(s, 0, 2000.0, 300.0)
        h = R.solve_highs(lp)
        assert h["ok"], (T, J, kw)
        out.append((f"T{T}_J{J}_highs", lp, h["x"], h["y"]))
        out.append((f"T{T}_J{J}_random", lp, rng.uniform(0, 300, len(h["x"])), rng.normal(0, 0.2, len(h["y"]))))
    return out


@pytest.mark.parametrize("case", cut_windows(), ids=lambda c: c[0])
def test_cut_equals_the_numpy_restatement_and_the_long_double_sum(host, case):
    _, lp, x, y = case
    got = native_cut(host, lp, x, y)
    want = R.cut_of(lp, x, y)
    assert got[VS.FLAG] == 0.0
    assert np.array_equal(got[:6], want[:6]), (got, want)           # the same operations in the same order: equal
    R.assert_within_rounding(got, lp, x, y)


def test_a_window_that_is_not_the_battery_pattern_is_flagged(host):
    s = C.positions([5], 1, 25, J=1)[0]
    lp = R.window_lp(s, 0, 1000.0, 200.0)
    lp = dict(lp, dcm_t=lp["dcm_t"][::-1].copy())   # descending steps: not the builder's order
    got = native_cut(host, lp, np.zeros(lp["K"].shape[1]), np.zeros(lp["K"].shape[0]))
    assert got[VS.FLAG] == 2.0 and np.isnan(got[:6]).all()


def master_sets():
    """Seeded cut sets: tangents of a convex function (interior optima), planes that push to a box corner or edge,
    duplicates and parallel cuts."""
    rng = np.random.default_rng(99)
    out = []
    for n in (1, 2, 3, 64, 256):
        for kind in ("tangent", "corner", "edge", "duplicates", "parallel"):
            box = (0.0, 5000.0, 0.0, 800.0)
            if kind in ("tangent", "duplicates", "parallel"):
                # tangents of f(E, P) = 1e5 exp(-E / 2000) + 8e4 exp(-P / 300) at seeded points
                pts = np.column_stack([rng.uniform(0, 5000, n), rng.uniform(0, 800, n)])
                f = 1e5 * np.exp(-pts[:, 0] / 2000) + 8e4 * np.exp(-pts[:, 1] / 300)
                gE, gP = -50.0 * np.exp(-pts[:, 0] / 2000), -8e4 / 300 * np.exp(-pts[:, 1] / 300)
                cuts = np.column_stack([f - gE * pts[:, 0] - gP * pts[:, 1], gE, gP])
                if kind == "duplicates" and n > 1:
                    cuts[1::2] = cuts[0:-1:2][:len(cuts[1::2])]
                if kind == "parallel" and n > 1:
                    cuts[1::2, 1:] = cuts[0:-1:2, 1:][:len(cuts[1::2])]
                    cuts[1::2, 0] += rng.uniform(-50, 50, len(cuts[1::2]))
                cost = (4.0, 30.0, 1.0)
            elif kind == "corner":   # steep benefits: E = Emax, P = Pmax
                cuts = np.column_stack([rng.uniform(0, 1e4, n), -rng.uniform(20, 30, n), -rng.uniform(100, 200, n)])
                cost = (4.0, 30.0, 1.0)
            else:                    # no benefit in E, a kink in P
                cuts = np.column_stack([rng.uniform(0, 1e4, n), np.zeros(n), -rng.uniform(0, 60, n)])
                cost = (4.0, 30.0, 1.0)
            out.append((f"{kind}_{n}", cuts, cost, box))
    return out


@pytest.mark.parametrize("case", master_sets(), ids=lambda c: c[0])
def test_master_is_within_the_highs_tolerance_of_linprog(host, case):
    _, cuts, (cE, cP, alpha), (elo, ehi, plo, phi) = case
    cuts = np.ascontiguousarray(cuts)
    out = np.zeros(4)
    rc = host.vc_master(len(cuts), _p(cuts), cE, cP, alpha, elo, ehi, plo, phi, _p(out))
    assert rc == 0
    spec = VS.ValueSizingSpec(ccost_kwh=cE, ccost_kw=cP, alpha=alpha, energy_min=elo, energy_max=ehi, power_min=plo,
                              power_max=phi)
    _, _, _, want = VS.master_host(cuts, spec)
    tol = 1e-9 * (1.0 + abs(want))
    print(f"master {out[3]!r} linprog {want!r}")
    assert abs(out[3] - want) <= tol
    # and the point is feasible and attains its objective
    E, P, th = out[:3]
    assert elo <= E <= ehi and plo <= P <= phi
    assert (cuts[:, 0] + cuts[:, 1] * E + cuts[:, 2] * P - th).max() <= tol
    assert abs((cE * E + cP * P + alpha * th) - out[3]) <= tol


@pytest.mark.parametrize("opts", [dict(eps=1e-7, eps_obj=1e-7), dict(max_iters=64)], ids=["eps1e-7", "iters64"])
def test_cuts_from_pdhg_duals_never_exceed_the_window_optimum(opts):
    """Weak duality: the cut of any y is below V(s') everywhere, up to rinf sum |x_j| over the free columns (the tau
    columns, whose reduced cost a PDHG dual leaves at rinf, not 0) and the rounding bound."""
    pos = C.positions([31, 32], 1, 48)
    rng = np.random.default_rng(5)
    others = np.column_stack([rng.uniform(0, 12000, 6), rng.uniform(0, 2000, 6)])
    for k in range(2):
        for E, P in [(3000.0, 400.0), (0.0, 0.0), (12000.0, 2000.0)]:
            lp = R.window_lp(pos[0], k, E, P)
            r = pdlp_ref.solve(lp, opts)
            cut = R.cut_of(lp, r["x"], r["y"])
            if "max_iters" in opts:
                assert r["status"] == pdlp_ref.ITER_LIMIT
            for E2, P2 in others:
                lp2 = R.window_lp(pos[0], k, E2, P2)
                h = R.solve_highs(lp2)
                assert h["ok"]
                slack = cut[VS.RINF] * np.abs(h["x"][3 * lp["T"]:]).sum() + 1e-9 * (1.0 + abs(h["obj"]))
                below = cut[VS.A] + cut[VS.GE] * E2 + cut[VS.GP] * P2
                assert below <= h["obj"] + slack, (k, E, P, E2, P2, below, h["obj"], slack)


@pytest.fixture(scope="module")
def sanitized_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("asan") / "value_cut_sanitize")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "native", "value_cut_sanitize.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)


def test_sanitized_run_is_clean(sanitized_run):
    p = sanitized_run
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    assert p.stdout.rstrip().endswith("done") and "failures=0" in p.stdout and "FAILED" not in p.stdout


@pytest.mark.parametrize("case,code", [("cuts_null_group", -1), ("cuts_null_out", -1), ("cuts_past_batch", -1),
                                       ("cuts_ice", -3), ("cuts_emin", -3), ("cuts_many_periods", -3),
                                       ("spec_nothing_sized", -1), ("spec_free_energy", -1), ("spec_free_power", -1),
                                       ("spec_zero_energy_cost", -1), ("spec_negative_power_cost", -1),
                                       ("master_null_arrays", -1), ("master_many_candidates", -1),
                                       ("master_cut_capacity", -1), ("master_count", -1)])
def test_malformed_call_is_refused_with_a_message(sanitized_run, case, code):
    m = re.search(rf"^{case} rc=(-?\d+) err=(.*)$", sanitized_run.stdout, re.M)
    assert m and int(m.group(1)) == code and len(m.group(2)) > 8, sanitized_run.stdout[-1500:]
