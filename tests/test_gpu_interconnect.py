"""GPU: the band kernel's interconnection form (csrc/dvh_band_grid.hip, BatchSolver.set_kernel_path("interconnect")):
battery windows with POI import / export limit rows (MicrogridPOI.py:215-258), a curtailable-PV column block
(IntermittentResourceSizing.py:79-91) and / or charge-from-PV rows (PV grid_charge = 0), built by
builder.battery_group and solved on cuda:0 against HiGHS on the same LP with tests/test_gpu_poi.py's bars: status
optimal, objective within 1e-5 relative, primal residual <= 1e-6.  The form is opt-in: the default cascade keeps
handing these windows down to the generic CSR kernel.  (The battery's fixed O&M, a constant of the objective, keeps
every window's optimum away from 0 -- a short window whose PV covers its load costs nothing else -- so that the relative
objective bar is defined for each.)"""
import dataclasses
import functools

import numpy as np
import pytest

from dervet_hip.lp import builder, scenarios
from dervet_hip.solver import WindowLP
from oracle import cases, window_lp
from planted_lp import from_window

pytestmark = pytest.mark.gpu

VARIANTS = ("poi", "poi_pv", "gc_pv", "poi_gc_pv")
SIZES = (2, 3, 5, 64, 65, 129, 744, 768)  # smallest recurrence, wave boundaries, idle lanes past T, the full block
SHAPES = [(T, J) for T in SIZES for J in (0, 1, 4) if J <= T]
BAT = dict(E=2000.0, Pch=500.0, Pdis=500.0, rte=0.9, sdr=0.0, soc_target=0.5, ulsoc=1.0, llsoc=0.1, fixedOM=1.0,
           OMexpenses=0.0, hp=0.0)
POI = dict(max_import=-650.0, max_export=0.0)
ICE = dict(rated_power=300.0, n=1.0, min_power=100.0, efficiency=0.0866, fuel_cost=3.5, variable_om_cost=0.0)


def _group(T, J, variant, G=2, ice=None):
    rng = np.random.default_rng(1000 * T + 10 * J + VARIANTS.index(variant))
    t = np.arange(T)
    kw = {}
    if "poi" in variant:
        kw["poi"] = POI
    if "pv" in variant:
        kw["pv_curtail_max"] = np.repeat((50.0 + 900.0 * np.sin(np.pi * (t + 0.5) / T))[None], G, 0)
    if "gc" in variant:
        kw["grid_charge"] = False
    # disjoint demand periods; the steps with t % (J + 1) == J have no DCM row
    masks = np.array([t % (J + 1) == j for j in range(J)], bool).reshape(J, T)
    return builder.battery_group(T, 1.0, rng.uniform(400.0, 700.0, (G, T)), BAT,
                                 retail_price=rng.uniform(0.05, 0.15, (G, T)), demand_masks=masks if J else None,
                                 demand_prices=rng.uniform(8.0, 20.0, (G, J)) if J else None, ice=ice, **kw)


def _lps(T, J, variant, **kw):
    return builder.group_window_lps(_group(T, J, variant, **kw))


@functools.lru_cache(maxsize=None)
def _highs(T, J, variant):
    """HiGHS objectives of the (T, J, variant) windows, computed once."""
    out = []
    for lp in _lps(T, J, variant):
        h = window_lp.solve_highs(from_window(lp))
        assert h["status"] == 0, (T, J, variant)
        out.append(h["obj"])
    return tuple(out)


def _within_bars(lps, res, objs):
    for k, (lp, r, ho) in enumerate(zip(lps, res, objs)):
        assert r.status == 0, (k, r.status_name)
        assert abs(r.obj - ho) <= 1e-5 * abs(ho), (k, r.obj, ho)
        assert window_lp.primal_residual_rel(from_window(lp), r.x)[0] <= 1e-6, k


def _highs_objs(lps):
    hs = [window_lp.solve_highs(from_window(lp)) for lp in lps]
    assert all(h["status"] == 0 for h in hs)
    return [h["obj"] for h in hs]


def _only_band(ks, count):
    assert ks["band_windows"] == count, ks
    assert ks["ell_windows"] == ks["generic_windows"] == ks["large_windows"] == ks["chain_windows"] == 0, ks


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T,J", SHAPES)
def test_interconnection_form_takes_every_shape_and_matches_highs(gpu_solver, T, J, variant):
    lps = _lps(T, J, variant)
    try:
        gpu_solver.set_kernel_path("interconnect")
        res = gpu_solver.solve(lps)
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_kernel_path("default")
    if T >= 5:  # (T <= 4: the two readings of n overlap, such a window may be handed on)
        _only_band(ks, len(lps))
    _within_bars(lps, res, _highs(T, J, variant))


def test_default_path_does_not_run_the_form(gpu_solver):
    lps = _lps(65, 1, "poi_gc_pv")
    res = gpu_solver.solve(lps)
    ks = gpu_solver.kernel_stats()
    assert ks["band_windows"] == 0 and ks["ell_windows"] + ks["generic_windows"] == len(lps), ks
    _within_bars(lps, res, _highs(65, 1, "poi_gc_pv"))


def test_a_batch_the_battery_form_takes_whole_still_waits_twice(gpu_solver):
    lps = [lp for g in scenarios.config4(range(30)) for lp in builder.group_window_lps(g)]
    try:
        gpu_solver.set_kernel_path("interconnect")
        res = gpu_solver.solve(lps)
        ks, syncs = gpu_solver.kernel_stats(), gpu_solver.host_syncs()
    finally:
        gpu_solver.set_kernel_path("default")
    assert all(r.status == 0 for r in res)
    assert ks["band_windows"] == 360 and syncs == 2, (ks, syncs)


def test_mixed_batch_moves_only_the_interconnection_windows(gpu_solver):
    arr, meta = cases.load_market()
    sig = {k.split("__", 1)[1]: v for k, v in arr.items() if k.startswith("es__")}
    head = [lp for g in scenarios.config4(range(2)) for lp in builder.group_window_lps(g)]
    market = builder.group_window_lps(scenarios.market_days(sig, meta["es"]["params"], days=list(range(0, 365, 40))))
    ice = [lp for g in scenarios.config5(range(1), years=1)[:3] for lp in builder.group_window_lps(g)]
    grid = _lps(65, 1, "poi_gc_pv")
    first = head + market + ice
    stats = {}
    try:
        for path in ("default", "interconnect"):
            gpu_solver.set_kernel_path(path)
            gpu_solver.solve(first)
            alone = gpu_solver.kernel_stats()
            res = gpu_solver.solve(first + grid)
            stats[path] = (alone, gpu_solver.kernel_stats(), gpu_solver.host_syncs(), res)
    finally:
        gpu_solver.set_kernel_path("default")
    counts = ("band_windows", "ell_windows", "generic_windows", "large_windows", "chain_windows")
    d_alone, d_all, d_syncs, d_res = stats["default"]
    i_alone, i_all, i_syncs, i_res = stats["interconnect"]
    # the first three groups land where the default cascade puts them ...
    assert {k: i_alone[k] for k in counts} == {k: d_alone[k] for k in counts}, (i_alone, d_alone)
    assert d_alone["band_windows"] == len(head) + len(ice) and d_alone["ell_windows"] == len(market), d_alone
    # ... and of the whole batch only the interconnection windows move, from the ELL / generic kernels to the band count
    assert d_all["band_windows"] == d_alone["band_windows"], d_all
    assert d_all["ell_windows"] + d_all["generic_windows"] == len(market) + len(grid), d_all
    assert i_all["band_windows"] == d_alone["band_windows"] + len(grid), i_all
    assert i_all["ell_windows"] == len(market) and i_all["generic_windows"] == 0, i_all
    assert i_syncs == d_syncs, (i_syncs, d_syncs)
    assert all(r.status == 0 for r in d_res + i_res)
    _within_bars(grid, i_res[len(first):], _highs(65, 1, "poi_gc_pv"))
    for a, b_ in zip(d_res[:len(first)], i_res[:len(first)]):  # the other windows: the same kernels, the same results
        assert a.obj == b_.obj and a.iters == b_.iters


def _permuted(lp, seed):
    """The window with its >= rows in a random order and the entries of every row in a random order."""
    rng = np.random.default_rng(seed)
    order = np.concatenate([np.arange(lp.m_eq), lp.m_eq + rng.permutation(lp.m - lp.m_eq)])
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
    lp = _lps(65, 1, "poi_gc_pv")[0]
    perm = _permuted(lp, 7)
    assert not np.array_equal(perm.indices, lp.indices)
    try:
        gpu_solver.set_kernel_path("interconnect")
        res = gpu_solver.solve([lp, perm])
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_kernel_path("default")
    _only_band(ks, 2)
    assert res[0].status == 0 and res[1].status == 0
    assert abs(res[1].obj - res[0].obj) <= 1e-9 * abs(res[0].obj), (res[0].obj, res[1].obj)


def _with_duplicated_import_row(lp, T, t):
    """The POI import row of step t (the first POI row block follows the DCM rows) appended once more."""
    n_dcm = lp.m - lp.m_eq - 3 * T  # poi_gc_pv: DCM rows, then T import, T export, T charge-from-PV rows
    i = lp.m_eq + n_dcm + t
    e = np.arange(lp.indptr[i], lp.indptr[i + 1])
    return WindowLP(np.append(lp.indptr, lp.indptr[-1] + len(e)).astype(np.int32), np.append(lp.indices, lp.indices[e]),
                    np.append(lp.data, lp.data[e]), lp.c, np.append(lp.q, lp.q[i]), lp.l, lp.u, lp.m_eq, lp.c0)


def test_windows_outside_the_shape_are_handed_on(gpu_solver):
    T = 65
    base = _lps(T, 1, "poi_gc_pv")
    pv0 = 3 * T + 1
    lo = base[1].l.copy()
    lo[pv0 + 20] = 1.0
    lps = [_with_duplicated_import_row(base[0], T, 11), dataclasses.replace(base[1], l=lo)]
    lps += _lps(T, 1, "poi", ice=ICE)
    objs = _highs_objs(lps)
    try:
        gpu_solver.set_kernel_path("interconnect")
        res = gpu_solver.solve(lps)
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_kernel_path("default")
    assert ks["band_windows"] == 0 and ks["ell_windows"] + ks["generic_windows"] == len(lps), ks
    _within_bars(lps, res, objs)


def test_crossed_pv_bounds_are_reported_infeasible(gpu_solver):
    T = 65
    lps = _lps(T, 1, "poi_gc_pv")
    hi = lps[0].u.copy()
    hi[3 * T + 1 + 20] = -1.0
    lps[0] = dataclasses.replace(lps[0], u=hi)
    try:
        gpu_solver.set_kernel_path("interconnect")
        res = gpu_solver.solve(lps)
    finally:
        gpu_solver.set_kernel_path("default")
    assert res[0].status_name == "infeasible" and res[0].iters == 0
    _within_bars(lps[1:], res[1:], _highs(T, 1, "poi_gc_pv")[1:])


def test_warm_start_from_own_solution_takes_fewer_iterations(gpu_solver):
    lps = _lps(129, 1, "poi_gc_pv")
    try:
        gpu_solver.set_kernel_path("interconnect")
        cold = gpu_solver.solve(lps)
        gpu_solver.set_options(warm_start=1)
        warm = gpu_solver.solve(lps, start=[(r.x, r.y) for r in cold])
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_options(warm_start=0)
        gpu_solver.set_kernel_path("default")
    _only_band(ks, len(lps))
    for c, w in zip(cold, warm):
        assert c.status == 0 and w.status == 0
        assert w.iters < c.iters, (w.iters, c.iters)
    _within_bars(lps, warm, _highs(129, 1, "poi_gc_pv"))


def _golden_groups(**kw):
    """tests/test_gpu_poi.py's sets: the es+pv+dg golden case's 12 monthly windows with the rows added."""
    wins, arr, meta, _ = cases.case_windows("es+pv+dg")
    p = meta["params"]
    gen = float(p["PV"]["rated_capacity"]) * np.nan_to_num(arr["pv_profile"])
    return scenarios.windows_by_period(2017, 1.0, arr["site_load"][None], np.zeros_like(gen)[None],
                                       cases.battery_from_params(p), tariff_def=meta["tariff"],
                                       ene_min=arr["agg_emin"][None], ene_max=arr["agg_emax"][None],
                                       pv_curtail_max=(12.0 * gen)[None], **kw)


@pytest.mark.parametrize("name", ["poi_no_export", "grid_charge_curtailable"])
def test_golden_case_windows_land_on_the_form(gpu_solver, name):
    kw = dict(poi=dict(max_import=-12000.0, max_export=0.0)) if name == "poi_no_export" else dict(grid_charge=False)
    lps = [lp for g in _golden_groups(**kw) for lp in builder.group_window_lps(g)]
    assert len(lps) == 12
    try:
        gpu_solver.set_kernel_path("interconnect")
        res = gpu_solver.solve(lps)
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_kernel_path("default")
    _only_band(ks, len(lps))
    _within_bars(lps, res, _highs_objs(lps))
