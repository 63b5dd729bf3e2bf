"""GPU: battery windows with one electric vehicle (builder.battery_group(ev=...), dervet MicrogridDER/ElectricVehicles.py
ElectricVehicle1) on the band kernel's load-shift form (csrc/dvh_band_shift.hip, set_kernel_path("load_shift")) and on
the default cascade, against HiGHS on the same LP with tests/test_gpu_load_shift.py's bars: status optimal, objective
within 1e-5 relative, primal residual <= 1e-6.  The windows are tests/ev_ref.py's.  The kernel is the controllable
load's, unchanged: the builder lays the EV's rows out in its shape, so no window may be handed on."""
import dataclasses
import functools

import numpy as np
import pytest

import ev_ref as ref
import result_contract as rc
from dervet_hip.lp import builder, scenarios
from oracle import cases, window_lp
from planted_lp import from_window

pytestmark = pytest.mark.gpu

COUNTS = ("band_windows", "ell_windows", "generic_windows", "large_windows", "chain_windows")
BY_ID = dict(zip(ref.IDS, ref.SHAPES))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(window LPs, their HiGHS objectives) of a shared shape, computed once."""
    lps = builder.group_window_lps(ref.group(*BY_ID[name]))
    assert all(ref.shift_form_accepts(lp) for lp in lps)
    hs = [window_lp.solve_highs(from_window(lp)) for lp in lps]
    assert all(h["status"] == 0 for h in hs)
    return lps, tuple(h["obj"] for h in hs)


def _within_bars(lps, res, objs):
    for k, (lp, r, ho) in enumerate(zip(lps, res, objs)):
        pres = window_lp.primal_residual_rel(from_window(lp), r.x)[0] if r.status == 0 else float("nan")
        print(f"EV window {k}: status {r.status_name} obj {r.obj:.9g} HiGHS {ho:.9g} rel {abs(r.obj - ho) / abs(ho):.2e} "
              f"primal residual {pres:.2e} iters {r.iters}")
        assert r.status == 0, (k, r.status_name)
        assert abs(r.obj - ho) <= 1e-5 * abs(ho), (k, r.obj, ho)
        assert pres <= 1e-6, k


def _only_band(ks, count):
    assert ks["band_windows"] == count, ks
    assert ks["ell_windows"] == ks["generic_windows"] == ks["large_windows"] == ks["chain_windows"] == 0, ks


def _solve(gpu_solver, lps, path="load_shift", **kw):
    try:
        gpu_solver.set_kernel_path(path)
        return gpu_solver.solve(lps, **kw), gpu_solver.kernel_stats(), gpu_solver.host_syncs()
    finally:
        gpu_solver.set_kernel_path("default")


@pytest.mark.parametrize("name", ref.IDS)
def test_load_shift_form_takes_every_shape_and_matches_highs(gpu_solver, name):
    lps, objs = _case(name)
    res, ks, _ = _solve(gpu_solver, lps)
    _only_band(ks, len(lps))
    assert 9000300 <= ks["variant"] < 9000400, ks  # dvh_band_shift.hip: 9000000 + 300 + waves per workgroup
    _within_bars(lps, res, objs)


@pytest.mark.parametrize("name", ref.IDS)
def test_default_path_solves_them_on_ell_or_generic(gpu_solver, name):
    lps, objs = _case(name)
    res = gpu_solver.solve(lps)
    ks = gpu_solver.kernel_stats()
    assert ks["band_windows"] == 0 and ks["ell_windows"] + ks["generic_windows"] == len(lps), ks
    _within_bars(lps, res, objs)


@pytest.mark.parametrize("name", ["T65J4", "T768J1"])
def test_result_contract_holds(gpu_solver, name):
    lps, objs = _case(name)
    res, ks, _ = _solve(gpu_solver, lps)
    _only_band(ks, len(lps))
    for k, (lp, r, opt) in enumerate(zip(lps, res, objs)):
        rc.check_both(from_window(lp), r, opt, f"{name} window {k}", form="band_shift")


def test_mixed_batch_moves_only_the_ev_windows(gpu_solver):
    """The config 4 head, market days, ICE windows (tests/test_gpu_load_shift.py's mixed batch) and the EV windows.  The
    market days keep the cascade's ELL pass in the batch on both paths, so equal host syncs say that the load-shift launch
    adds no host wait.  (Measured on the MI355X with the head and the EV windows alone: 3 syncs on the load-shift path, 5
    on the default path -- there the EV windows are the only ones that go down the cascade.)"""
    arr, meta = cases.load_market()
    sig = {k.split("__", 1)[1]: v for k, v in arr.items() if k.startswith("es__")}
    head = [lp for g in scenarios.config4(range(2)) for lp in builder.group_window_lps(g)]
    market = builder.group_window_lps(scenarios.market_days(sig, meta["es"]["params"], days=list(range(0, 365, 40))))
    ice = [lp for g in scenarios.config5(range(1), years=1)[:3] for lp in builder.group_window_lps(g)]
    ev, objs = _case("T129J1")
    first = head + market + ice
    stats = {}
    for path in ("default", "load_shift"):
        _, alone, _ = _solve(gpu_solver, first, path)
        res, ks, syncs = _solve(gpu_solver, first + ev, path)
        stats[path] = (alone, ks, syncs, res)
    d_alone, d_all, d_syncs, d_res = stats["default"]
    s_alone, s_all, s_syncs, s_res = stats["load_shift"]
    print(f"EV mixed batch: host syncs default {d_syncs} load_shift {s_syncs}; default {d_all}; load_shift {s_all}")
    assert {k: s_alone[k] for k in COUNTS} == {k: d_alone[k] for k in COUNTS}, (s_alone, d_alone)
    assert d_alone["band_windows"] == len(head) + len(ice) and d_alone["ell_windows"] == len(market), d_alone
    # of the whole batch only the EV windows move, from the ELL / generic kernels to the band count
    assert d_all["band_windows"] == d_alone["band_windows"], d_all
    assert d_all["ell_windows"] + d_all["generic_windows"] == len(market) + len(ev), d_all
    assert s_all["band_windows"] == d_alone["band_windows"] + len(ev), s_all
    assert s_all["ell_windows"] == len(market) and s_all["generic_windows"] == 0, s_all
    assert s_all["large_windows"] == s_all["chain_windows"] == 0, s_all
    assert s_syncs == d_syncs, (s_syncs, d_syncs)
    assert all(r.status == 0 for r in d_res + s_res)
    _within_bars(ev, s_res[len(first):], objs)
    _within_bars(ev, d_res[len(first):], objs)
    for a, b_ in zip(d_res[:len(first)], s_res[:len(first)]):  # the other windows: the same kernels, the same results
        assert a.obj == b_.obj and a.iters == b_.iters


def test_an_unreachable_target_is_certified_infeasible(gpu_solver):  # (gpu_solver: the suite's no-GPU failure message)
    """13 plugged hours at 50 kW cannot collect 1,000 kWh: the form runs the window to the iteration limit and the
    certificate pass behind the solve proves it infeasible."""
    import certify_ref as cr
    from dervet_hip import BatchSolver
    T, J, pl, _ = BY_ID["T72J1"]
    good, objs = _case("T72J1")
    bad = builder.group_window_lps(ref.group(T, J, pl, 1000.0))[1]
    assert ref.shift_form_accepts(bad) and cr.highs_status(bad)[0] == 2
    batch = [good[0], bad]
    with BatchSolver(0, certify=1) as s:
        s.set_kernel_path("load_shift")
        res = s.solve(batch)
        ks, st = s.kernel_stats(), s.certify_stats()
    _only_band(ks, 2)
    _within_bars(batch[:1], res[:1], objs[:1])
    assert res[1].status_name == "infeasible", (res[1].status_name, res[1].iters)
    margin, viol = cr.farkas(bad, res[1].y)
    assert margin > 0.0 and viol <= 1e-8 * margin, (margin, viol)
    assert st["primal_infeasible"] == 1 and st["examined"] == 1, st


def test_the_solved_state_is_the_references(gpu_solver):
    """ev_energy of the GPU's solution: zero at every plug-in, the target at every plug-out, within the residual bar."""
    name = "T72J1"
    T, J, pl, tg = BY_ID[name]
    lps, _ = _case(name)
    res, _, _ = _solve(gpu_solver, lps)
    g = ref.group(T, J, pl, tg)
    e = builder.ev_energy(g, np.array([r.x for r in res]))
    plug_in, plug_out = ref.plug_steps(pl)
    scale = 1e-6 * max(1.0, float(np.abs(lps[0].q).max()))
    assert np.all(np.abs(e[:, plug_in]) <= scale) and np.all(np.abs(e[:, plug_out] - tg) <= scale)
