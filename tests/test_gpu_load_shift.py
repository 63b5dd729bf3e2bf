"""GPU: the band kernel's load-shift form (csrc/dvh_band_shift.hip, BatchSolver.set_kernel_path("load_shift")):
battery windows with a controllable load (dervet MicrogridDER/LoadControllable.py:215-251), built by
builder.battery_group(ctrl_load=...) and solved on cuda:0 against HiGHS on the same LP with tests/test_gpu_interconnect.py's
bars: status optimal, objective within 1e-5 relative, primal residual <= 1e-6.  The windows are tests/ctrl_load_ref.py's
(that file's battery and series, P = 150 kW, 4 h).  The form is opt-in: the default cascade keeps these windows on the
ELL / generic kernels."""
import dataclasses
import functools

import numpy as np
import pytest

import ctrl_load_ref as ref
import result_contract as rc
from dervet_hip.lp import builder, scenarios
from oracle import cases, window_lp
from planted_lp import from_window

pytestmark = pytest.mark.gpu

COUNTS = ("band_windows", "ell_windows", "generic_windows", "large_windows", "chain_windows")


@functools.lru_cache(maxsize=None)
def _case(T, J, ds):
    """(window LPs, their HiGHS objectives), computed once."""
    lps = builder.group_window_lps(ref.group(T, J, list(ds)))
    return lps, tuple(_highs_objs(lps))


def _highs_objs(lps):
    hs = [window_lp.solve_highs(from_window(lp)) for lp in lps]
    assert all(h["status"] == 0 for h in hs)
    return [h["obj"] for h in hs]


def _within_bars(lps, res, objs):
    for k, (lp, r, ho) in enumerate(zip(lps, res, objs)):
        assert r.status == 0, (k, r.status_name)
        assert abs(r.obj - ho) <= 1e-5 * abs(ho), (k, r.obj, ho)
        assert window_lp.primal_residual_rel(from_window(lp), r.x)[0] <= 1e-6, k


def _only_band(ks, count):
    assert ks["band_windows"] == count, ks
    assert ks["ell_windows"] == ks["generic_windows"] == ks["large_windows"] == ks["chain_windows"] == 0, ks


def _solve(gpu_solver, lps, path="load_shift", **kw):
    try:
        gpu_solver.set_kernel_path(path)
        return gpu_solver.solve(lps, **kw), gpu_solver.kernel_stats(), gpu_solver.host_syncs()
    finally:
        gpu_solver.set_kernel_path("default")


@pytest.mark.parametrize("T,J,ds", ref.SHAPES)
def test_load_shift_form_takes_every_shape_and_matches_highs(gpu_solver, T, J, ds):
    lps, objs = _case(T, J, tuple(ds))
    res, ks, _ = _solve(gpu_solver, lps)
    if T >= 5:
        _only_band(ks, len(lps))
        assert 9000300 <= ks["variant"] < 9000400, ks  # dvh_band_shift.hip: 9000000 + 300 + waves per workgroup
    _within_bars(lps, res, objs)


@pytest.mark.parametrize("T,J,ds", [s for s in ref.SHAPES if s[0] in (5, 65, 768)])
def test_default_path_leaves_them_on_ell_or_generic(gpu_solver, T, J, ds):
    lps, objs = _case(T, J, tuple(ds))
    res = gpu_solver.solve(lps)
    ks = gpu_solver.kernel_stats()
    assert ks["band_windows"] == 0 and ks["ell_windows"] + ks["generic_windows"] == len(lps), ks
    _within_bars(lps, res, objs)


def test_mixed_batch_moves_only_the_load_shift_windows(gpu_solver):
    arr, meta = cases.load_market()
    sig = {k.split("__", 1)[1]: v for k, v in arr.items() if k.startswith("es__")}
    head = [lp for g in scenarios.config4(range(2)) for lp in builder.group_window_lps(g)]
    market = builder.group_window_lps(scenarios.market_days(sig, meta["es"]["params"], days=list(range(0, 365, 40))))
    ice = [lp for g in scenarios.config5(range(1), years=1)[:3] for lp in builder.group_window_lps(g)]
    shift, objs = _case(65, 4, (0, 17, 41))
    first = head + market + ice
    stats = {}
    for path in ("default", "load_shift"):
        _, alone, _ = _solve(gpu_solver, first, path)
        res, ks, syncs = _solve(gpu_solver, first + shift, path)
        stats[path] = (alone, ks, syncs, res)
    d_alone, d_all, d_syncs, d_res = stats["default"]
    s_alone, s_all, s_syncs, s_res = stats["load_shift"]
    # the first three groups land where the default cascade puts them ...
    assert {k: s_alone[k] for k in COUNTS} == {k: d_alone[k] for k in COUNTS}, (s_alone, d_alone)
    assert d_alone["band_windows"] == len(head) + len(ice) and d_alone["ell_windows"] == len(market), d_alone
    # ... and of the whole batch only the load-shift windows move, from the ELL / generic kernels to the band count
    assert d_all["band_windows"] == d_alone["band_windows"], d_all
    assert d_all["ell_windows"] + d_all["generic_windows"] == len(market) + len(shift), d_all
    assert s_all["band_windows"] == d_alone["band_windows"] + len(shift), s_all
    assert s_all["ell_windows"] == len(market) and s_all["generic_windows"] == 0, s_all
    assert s_syncs == d_syncs, (s_syncs, d_syncs)
    assert all(r.status == 0 for r in d_res + s_res)
    _within_bars(shift, s_res[len(first):], objs)
    for a, b_ in zip(d_res[:len(first)], s_res[:len(first)]):  # the other windows: the same kernels, the same results
        assert a.obj == b_.obj and a.iters == b_.iters


@pytest.mark.parametrize("T,J,ds", [s for s in ref.SHAPES if (s[0], s[1]) in ((65, 4), (768, 1))])
def test_result_contract_holds(gpu_solver, T, J, ds):
    lps, objs = _case(T, J, tuple(ds))
    res, ks, _ = _solve(gpu_solver, lps)
    _only_band(ks, len(lps))
    for k, (lp, r, opt) in enumerate(zip(lps, res, objs)):
        rc.check_both(from_window(lp), r, opt, f"T{T}J{J} window {k}", form="band_shift")


def test_the_lower_bound_of_pw_is_carried_and_not_mirrored(gpu_solver):
    T, J, ds = 48, 1, (0, 24)
    lps, sym = _case(T, J, ds)
    lo = lps[0].l.copy()
    lo[3 * T + J:4 * T + J] = -0.5 * ref.P
    lp = dataclasses.replace(lps[0], l=lo)
    obj = _highs_objs([lp])[0]
    assert obj > sym[0] * (1 + 1e-4), (obj, sym[0])  # the tighter lower bound binds: the two optima differ
    res, ks, _ = _solve(gpu_solver, [lp])
    _only_band(ks, 1)
    _within_bars([lp], res, [obj])
    assert res[0].x[3 * T + J:4 * T + J].min() >= -0.5 * ref.P


def _permuted(lp, T, seed):
    """The window with its load rows in a random order among themselves, its >= rows likewise, and the entries of
    every row in a random order (the battery's T + 1 rows keep their places: row t + 1 is step t's)."""
    from dervet_hip.solver import WindowLP
    rng = np.random.default_rng(seed)
    order = np.concatenate([np.arange(T + 1), T + 1 + rng.permutation(lp.m_eq - T - 1),
                            lp.m_eq + rng.permutation(lp.m - lp.m_eq)])
    indptr, indices, data = [0], [], []
    for i in order:
        e = np.arange(lp.indptr[i], lp.indptr[i + 1])
        e = e[rng.permutation(len(e))]
        indices.append(lp.indices[e])
        data.append(lp.data[e])
        indptr.append(indptr[-1] + len(e))
    return WindowLP(np.asarray(indptr, np.int32), np.concatenate(indices).astype(np.int32), np.concatenate(data),
                    lp.c, lp.q[order], lp.l, lp.u, lp.m_eq, lp.c0)


def test_row_order_and_entry_order_do_not_matter(gpu_solver):
    T, J, ds = 65, 4, (0, 17, 41)
    lp = _case(T, J, ds)[0][0]
    perm = _permuted(lp, T, 7)
    assert not np.array_equal(perm.indices, lp.indices)
    res, ks, _ = _solve(gpu_solver, [lp, perm])
    _only_band(ks, 2)
    assert res[0].status == 0 and res[1].status == 0
    assert abs(res[1].obj - res[0].obj) <= 1e-9 * abs(res[0].obj), (res[0].obj, res[1].obj)


def test_windows_outside_the_shape_are_handed_on(gpu_solver):
    T, J, ds = 65, 4, (0, 17, 41)
    lps, objs = _case(T, J, ds)
    lo = lps[1].l.copy()
    lo[4 * T + J + 20] = 1.0  # a lower bound of el the kernel does not carry
    plain = builder.group_window_lps(ref.group(T, J, list(ds), rated_power=None))  # the battery form's window
    batch = [dataclasses.replace(lps[1], l=lo)] + plain
    res, ks, _ = _solve(gpu_solver, batch)
    assert ks["band_windows"] == len(plain) and ks["ell_windows"] + ks["generic_windows"] == 1, ks
    _within_bars(batch, res, _highs_objs(batch))


def test_the_battery_and_ice_forms_refuse_these_windows(gpu_solver):
    # (the default path runs both band passes over them: none is counted as a band window)
    lps, _ = _case(129, 1, tuple(ref.every24(129)))
    gpu_solver.solve(lps)
    assert gpu_solver.kernel_stats()["band_windows"] == 0


def test_certify_1_works_through_the_after_pass(gpu_solver):  # (gpu_solver: the suite's no-GPU failure message)
    """An infeasible window that is not crossed bounds: el's upper bound at a day's first step below E_L, which the
    day-start row asks for.  The form runs it to the iteration limit; the certificate pass behind the solve proves it."""
    import certify_ref as cr
    from dervet_hip import BatchSolver
    T, J, ds = 48, 1, (0, 24)
    lps, objs = _case(T, J, ds)
    hi = lps[1].u.copy()
    hi[4 * T + J + 24] = 0.5 * ref.P * ref.DH
    batch = [lps[0], dataclasses.replace(lps[1], u=hi)]
    assert cr.highs_status(batch[1])[0] == 2
    with BatchSolver(0, certify=1) as s:
        s.set_kernel_path("load_shift")
        res = s.solve(batch)
        ks, st = s.kernel_stats(), s.certify_stats()
    _only_band(ks, 2)
    _within_bars(batch[:1], res[:1], objs[:1])
    assert res[1].status_name == "infeasible", (res[1].status_name, res[1].iters)
    margin, viol = cr.farkas(batch[1], res[1].y)
    assert margin > 0.0 and viol <= 1e-8 * margin, (margin, viol)
    assert st["primal_infeasible"] == 1 and st["examined"] == 1, st


def test_warm_start_from_own_solution_takes_fewer_iterations(gpu_solver):
    lps, objs = _case(129, 1, tuple(ref.every24(129)))
    try:
        cold, _, _ = _solve(gpu_solver, lps)
        gpu_solver.set_options(warm_start=1)
        warm, ks, _ = _solve(gpu_solver, lps, start=[(r.x, r.y) for r in cold])
    finally:
        gpu_solver.set_options(warm_start=0)
    _only_band(ks, len(lps))
    for c, w in zip(cold, warm):
        assert c.status == 0 and w.status == 0
        assert w.iters < c.iters, (w.iters, c.iters)
    _within_bars(lps, warm, objs)
