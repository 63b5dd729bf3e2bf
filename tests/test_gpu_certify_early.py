"""GPU: the early exit for infeasible windows inside the PDHG kernels (``certify=2``; csrc/dvh_kernels.hip pdhg_kernel,
csrc/dvh_band_grid.hip) against HiGHS, the numpy restatement of tests/certify_early_ref.py and the same solves at
``certify=1``.  On the "interconnect" path POI windows reach the band kernel's interconnection form; on "default" the
month-long ones (T = 768) reach the generic kernel, while the ELL tier's small-window kernels take most of those of up
to 512 columns (T <= 25 here, except with two demand periods at T = 25) -- that tier ignores the level, so there
level 2 must be level 1 bit for bit -- and "generic" puts every shape on the generic kernel.  Both kernels test the dual of T(z_k) at every KKT check.

Measured on the MI355X (the population below on the generic kernel and the interconnection form): every HiGHS-infeasible
window certified inside the kernels, the latest at iteration 3,456 (T = 768, J = 1, margin_out with PV: the
restatement's own worst), none later than the restatement's iteration plus one KKT period; every feasible window
bit-identical to level 1."""
import dataclasses

import numpy as np
import pytest

import certify_early_ref as er
import certify_ref as cr
from dervet_hip import BatchSolver, _lib
from dervet_hip.lp import builder, scenarios

pytestmark = pytest.mark.gpu
MAX_ITERS = 100000
PATHS = ("default", "generic", "interconnect")
TS = (2, 3, 5, 25, 768)   # smallest recurrence / the grid form's two-reading threshold / a partial wave / the full block
SHAPES = [(T, J, pv) for T in TS for J in er.JS for pv in (False, True)]


@pytest.fixture(scope="module")
def solver(gpu_solver):  # (gpu_solver: the suite's no-GPU failure message)
    s = BatchSolver(0, max_iters=MAX_ITERS, certify=2)
    yield s
    s.close()


def _solve(s, lps, level, path="default", max_iters=MAX_ITERS):
    """(results, certify_stats without the time, kernel_stats, host_syncs) of one solve; the solver's settings restored."""
    try:
        s.set_kernel_path(path)
        s.set_options(certify=level, max_iters=max_iters)
        res = s.solve(lps)
        st = {k: v for k, v in s.certify_stats().items() if k != "ms"}
        return res, st, s.kernel_stats(), s.host_syncs()
    finally:
        s.set_kernel_path("default")
        s.set_options(certify=2, max_iters=MAX_ITERS)


def _bits(r):
    return (r.status, r.iters, r.x.tobytes(), r.y.tobytes(),
            np.array([r.obj, r.primal_res_rel, r.dual_res_rel, r.gap_rel]).tobytes())


def _check_early(key, r):
    """The bars of an early-certified window: status, the iteration schedule and parity with the restatement, the ray."""
    lp = er.window(key)
    ref = er.restated(key)
    margin, viol = cr.farkas(lp, r.y)
    print(f"{key}: iters {r.iters} (restated {ref['iters']}) margin {margin:.6e} (reported {r.primal_res_rel:.6e}) "
          f"viol {viol:.3e} (reported {r.dual_res_rel:.3e})")
    assert r.status_name == "infeasible" and r.obj == np.inf and r.gap_rel == 0.0
    assert ref["status"] == er.PRIMAL_INFEASIBLE and ref["iters"] <= er.EARLY_CAP
    assert r.iters % er.KKT_PERIOD == 0 and 0 < r.iters <= er.EARLY_CAP
    assert r.iters <= ref["iters"] + er.KKT_PERIOD
    er.farkas_bars(lp, r.y, r.primal_res_rel)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("T,J,pv", SHAPES)
def test_infeasible_windows_stop_at_the_check_that_certifies_them(solver, path, T, J, pv):
    keys = er.keys_of(T, J, pv)
    lps = [er.window(k) for k in keys]
    hs = [er.highs(k) for k in keys]
    bad = [i for i, h in enumerate(hs) if h[0] == 2]
    good = [i for i, h in enumerate(hs) if h[0] == 0]
    assert len(bad) + len(good) == len(keys) and bad and good
    two, st2, ks2, _ = _solve(solver, lps, 2, path)
    print(path, T, J, pv, [(r.status_name, r.iters) for r in two], st2, ks2)
    one, st1, ks1, _ = _solve(solver, lps, 1, path)
    assert st1["early"] == 0 and ks1 == ks2
    if path == "interconnect":  # the interconnection form, or the generic kernel behind it for a window it refuses
        assert ks2["band_windows"] + ks2["generic_windows"] == len(lps) and ks2["ell_windows"] == 0
    elif path == "generic" or T > 25 or ks2["generic_windows"]:  # POI windows end on the generic kernel
        assert ks2["generic_windows"] == len(lps) and ks2["band_windows"] == 0 and ks2["ell_windows"] == 0
    else:  # n <= 512: the ELL tier's small-window kernels own the shapes they fit and ignore the level
        assert ks2["ell_windows"] == len(lps) and ks2["band_windows"] == 0 and ks2["generic_windows"] == 0
        assert [_bits(r) for r in two] == [_bits(r) for r in one] and st2 == st1 and st2["early"] == 0
        return
    # 1. every infeasible window is certified inside the kernel (on the parent: iters = 100,000, early missing)
    for i in bad:
        _check_early(keys[i], two[i])
    assert st2["early"] == len(bad) and st2["examined"] == 0
    assert st2["early_max_iters"] == max(two[i].iters for i in bad)
    # 2. every feasible window is what level 1 returns, bit for bit, and HiGHS's optimum
    for i in good:
        assert two[i].status_name == "optimal" and _bits(two[i]) == _bits(one[i]), keys[i]
        assert abs(two[i].obj - hs[i][1]) <= 1e-5 * abs(hs[i][1]), keys[i]


@pytest.mark.parametrize("path", ("generic", "interconnect"))
def test_a_window_of_a_mixed_batch_gets_its_solo_result(solver, path):
    keys = er.keys_of(25, 1, False) + er.keys_of(5, 2, True)
    lps = [er.window(k) for k in keys]
    mixed, st, _, syncs2 = _solve(solver, lps, 2, path)
    _, _, _, syncs1 = _solve(solver, lps, 1, path)
    assert syncs1 == syncs2
    n_bad = sum(er.highs(k)[0] == 2 for k in keys)
    assert st["early"] == n_bad and 0 < n_bad < len(keys)
    for k, lp, r in zip(keys, lps, mixed):
        solo, st_solo, _, _ = _solve(solver, [lp], 2, path)
        assert _bits(solo[0]) == _bits(r), k
        assert st_solo["early"] == (1 if er.highs(k)[0] == 2 else 0)


def test_a_limit_below_the_certifying_check_leaves_the_window_to_the_after_pass(solver):
    key = next(k for T in (25, 5) for J in er.JS for k in er.keys_of(T, J, False)
               if er.highs(k)[0] == 2 and er.restated(k)["iters"] == 2 * er.KKT_PERIOD)
    lp = er.window(key)
    full, st_full, _, _ = _solve(solver, [lp], 2, "generic")
    assert full[0].iters == 2 * er.KKT_PERIOD and st_full["early"] == 1
    res, st, _, _ = _solve(solver, [lp], 2, "generic", max_iters=er.KKT_PERIOD)
    one, st1, _, _ = _solve(solver, [lp], 1, "generic", max_iters=er.KKT_PERIOD)
    print(key, res[0].status_name, res[0].iters, st)
    assert res[0].status_name == "infeasible" and res[0].iters == er.KKT_PERIOD
    assert st["early"] == 0 and st["examined"] == 1 and st["primal_infeasible"] == 1
    er.farkas_bars(lp, res[0].y, res[0].primal_res_rel)
    assert _bits(res[0]) == _bits(one[0]) and st == st1  # level 1's behaviour


@pytest.mark.parametrize("path", ("generic", "interconnect"))
def test_early_certificates_are_bit_reproducible(solver, path):
    keys = er.keys_of(25, 2, True) + er.keys_of(768, 1, True)
    lps = [er.window(k) for k in keys]
    (a, sa, _, _), (b, sb, _, _) = _solve(solver, lps, 2, path), _solve(solver, lps, 2, path)
    assert sa == sb and sa["early"] == sum(er.highs(k)[0] == 2 for k in keys)
    assert [_bits(r) for r in a] == [_bits(r) for r in b]


def _config4_batch():
    """Four config-4 battery windows, the third with an upper energy bound at step 1 below what one step of discharge
    at the rating leaves (unreachable, not crossed): infeasible, on the battery band / ELL tiers."""
    lps = [lp for g in scenarios.config4([3]) for lp in builder.group_window_lps(g)][:4]
    lp = lps[2]
    T = lp.m_eq - 1
    p = lp.indptr[1]  # row 1: -dt rte ch_0 + dt dis_0 - (1 - dt sdr) ene_0 + ene_1 = 0
    reach = -lp.data[p + 2] * lp.q[0] - lp.data[p + 1] * lp.u[T]  # the lowest ene_1
    lo = lp.l[2 * T + 1]
    assert lo < reach
    u = lp.u.copy()
    u[2 * T + 1] = 0.5 * (lo + reach)
    lps[2] = dataclasses.replace(lp, u=u)
    return lps


@pytest.mark.parametrize("path", ("band1", "band3", "ell"))
def test_the_other_tiers_ignore_the_level(solver, path):
    lps = _config4_batch()
    assert cr.highs_status(lps[2])[0] == 2
    one, st1, ks1, _ = _solve(solver, lps, 1, path, max_iters=4096)
    two, st2, ks2, _ = _solve(solver, lps, 2, path, max_iters=4096)
    print(path, [(r.status_name, r.iters) for r in two], st2, ks2)
    assert ks2 == ks1 and ks2["generic_windows"] == 0
    assert [_bits(r) for r in two] == [_bits(r) for r in one]
    assert st2 == st1 and st2["early"] == 0 and st2["primal_infeasible"] == 1 and two[2].status == _lib.PRIMAL_INFEASIBLE


def test_battery_windows_forced_onto_the_generic_kernel_are_certified_early(solver):
    keys = [k for T in (5, 25, 768) for k in er.keys_no_poi(T, 1, False)]
    lps = [er.window(k) for k in keys]
    res, st, ks, _ = _solve(solver, lps, 2, "generic")
    print([(r.status_name, r.iters) for r in res], st, ks)
    assert ks["generic_windows"] == len(lps)
    bad = [i for i, k in enumerate(keys) if er.highs(k)[0] == 2]
    assert len(bad) == 3 and st["early"] == 3 and st["examined"] == 0
    for i, (k, r) in enumerate(zip(keys, res)):
        if i in bad:
            _check_early(k, r)
        else:
            assert r.status_name == "optimal" and abs(r.obj - er.highs(k)[1]) <= 1e-5 * abs(er.highs(k)[1])
