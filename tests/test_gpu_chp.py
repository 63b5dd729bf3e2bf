"""GPU: the band kernel's heat form (csrc/dvh_band_heat.hip, BatchSolver.set_kernel_path("chp")): battery windows with
one combined-heat-and-power unit and the site's steam / hot-water loads (dervet MicrogridDER/CombinedHeatPower.py,
MicrogridPOI.py:215-258), built by builder.battery_group(chp=...) and solved on cuda:0 against HiGHS on the same LP with
tests/test_gpu_interconnect.py's bars: status optimal, objective within 1e-5 relative, primal residual <= 1e-6.  The
windows are tests/chp_ref.py's.  The form is opt-in: the default cascade keeps these windows on the ELL / generic
kernels -- and, above the on-chip size of those kernels (n or m > 4096: the shapes with T = 744 and 768 here), on the
grid-wide path that takes one window at a time."""
import dataclasses
import functools

import numpy as np
import pytest

import chp_ref as ref
import result_contract as rc
from dervet_hip.lp import builder, scenarios
from oracle import cases, window_lp
from planted_lp import from_window

pytestmark = pytest.mark.gpu

COUNTS = ("band_windows", "ell_windows", "generic_windows", "large_windows", "chain_windows")
SMALL_MAX = 4096  # csrc/dvh_internal.h kSmallMax


@functools.lru_cache(maxsize=None)
def _case(T, J):
    """(window LPs, their HiGHS objectives), computed once."""
    lps = builder.group_window_lps(ref.group(T, J))
    return lps, tuple(_highs_objs(lps))


def _highs_objs(lps):
    hs = [window_lp.solve_highs(from_window(lp)) for lp in lps]
    assert all(h["status"] == 0 for h in hs)
    return [h["obj"] for h in hs]


def _within_bars(lps, res, objs):
    for k, (lp, r, ho) in enumerate(zip(lps, res, objs)):
        pres = window_lp.primal_residual_rel(from_window(lp), r.x)[0] if r.status == 0 else float("nan")
        print(f"CHP window {k}: status {r.status_name} iters {r.iters} obj {r.obj:.9f} highs {ho:.9f} "
              f"rel {abs(r.obj - ho) / abs(ho):.2e} pres {pres:.2e}")
        assert r.status == 0, (k, r.status_name)
        assert abs(r.obj - ho) <= 1e-5 * abs(ho), (k, r.obj, ho)
        assert pres <= 1e-6, k


def _only_band(ks, count):
    assert ks["band_windows"] == count, ks
    assert ks["ell_windows"] == ks["generic_windows"] == ks["large_windows"] == ks["chain_windows"] == 0, ks


def _solve(gpu_solver, lps, path="chp", **kw):
    try:
        gpu_solver.set_kernel_path(path)
        return gpu_solver.solve(lps, **kw), gpu_solver.kernel_stats(), gpu_solver.host_syncs()
    finally:
        gpu_solver.set_kernel_path("default")


@pytest.mark.parametrize("T,J", ref.SHAPES)
def test_heat_form_takes_every_shape_and_matches_highs(gpu_solver, T, J):
    lps, objs = _case(T, J)
    res, ks, _ = _solve(gpu_solver, lps)
    _only_band(ks, len(lps))
    if T >= 5:
        assert ks["variant"] == 9000412, ks  # dvh_band_heat.hip: 9000000 + 400 + waves per workgroup (768 / 64)
    _within_bars(lps, res, objs)


@pytest.mark.parametrize("T,J", ref.SHAPES)
def test_default_path_leaves_them_to_the_other_kernels(gpu_solver, T, J):
    lps, objs = _case(T, J)
    res = gpu_solver.solve(lps)
    ks = gpu_solver.kernel_stats()
    assert ks["band_windows"] == 0, ks
    if max(lps[0].n, lps[0].m) <= SMALL_MAX:
        assert ks["ell_windows"] + ks["generic_windows"] == len(lps), ks
    else:  # above the on-chip size: one window at a time on the grid-wide path
        assert ks["large_windows"] == len(lps), ks
    _within_bars(lps, res, objs)


@pytest.mark.parametrize("path", ["load_shift", "interconnect"])
@pytest.mark.parametrize("T,J", [(2, 0), (3, 1), (5, 1), (65, 4), (768, 1)])
def test_the_other_opt_in_forms_refuse_these_windows(gpu_solver, path, T, J):
    lps, objs = _case(T, J)
    res, ks, _ = _solve(gpu_solver, lps, path)
    assert ks["band_windows"] == 0, ks
    _within_bars(lps, res, objs)


def test_mixed_batch_moves_only_the_chp_windows(gpu_solver):
    arr, meta = cases.load_market()
    sig = {k.split("__", 1)[1]: v for k, v in arr.items() if k.startswith("es__")}
    head = [lp for g in scenarios.config4(range(2)) for lp in builder.group_window_lps(g)]
    market = builder.group_window_lps(scenarios.market_days(sig, meta["es"]["params"], days=list(range(0, 365, 40))))
    ice = [lp for g in scenarios.config5(range(1), years=1)[:3] for lp in builder.group_window_lps(g)]
    heat, objs = _case(65, 4)
    first = head + market + ice
    stats = {}
    for path in ("default", "chp"):
        _, alone, _ = _solve(gpu_solver, first, path)
        res, ks, syncs = _solve(gpu_solver, first + heat, path)
        stats[path] = (alone, ks, syncs, res)
    d_alone, d_all, d_syncs, d_res = stats["default"]
    s_alone, s_all, s_syncs, s_res = stats["chp"]
    # the first three groups land where the default cascade puts them ...
    assert {k: s_alone[k] for k in COUNTS} == {k: d_alone[k] for k in COUNTS}, (s_alone, d_alone)
    assert d_alone["band_windows"] == len(head) + len(ice) and d_alone["ell_windows"] == len(market), d_alone
    # ... and of the whole batch only the CHP windows move, from the ELL / generic kernels to the band count
    assert d_all["band_windows"] == d_alone["band_windows"], d_all
    assert d_all["ell_windows"] + d_all["generic_windows"] == len(market) + len(heat), d_all
    assert s_all["band_windows"] == d_alone["band_windows"] + len(heat), s_all
    assert s_all["ell_windows"] == len(market) and s_all["generic_windows"] == 0, s_all
    assert s_syncs == d_syncs, (s_syncs, d_syncs)
    assert all(r.status == 0 for r in d_res + s_res)
    _within_bars(heat, s_res[len(first):], objs)
    for a, b_ in zip(d_res[:len(first)], s_res[:len(first)]):  # the other windows: the same kernels, the same results
        assert a.obj == b_.obj and a.iters == b_.iters


@pytest.mark.parametrize("T,J", [(65, 4), (768, 1)])
def test_result_contract_holds(gpu_solver, T, J):
    lps, objs = _case(T, J)
    res, ks, _ = _solve(gpu_solver, lps)
    _only_band(ks, len(lps))
    for k, (lp, r, opt) in enumerate(zip(lps, res, objs)):
        rc.check_both(from_window(lp), r, opt, f"T{T}J{J} window {k}", form="band_heat")


def test_the_thermal_lower_bounds_are_carried(gpu_solver):
    T, J = 48, 1
    lps, base = _case(T, J)
    steam = ref.series(T, J)[5].copy()
    steam[:, ::3] += 60.0  # (the must-run stays below the cap: 0.8 (140 + 93.3) = 187 kW)
    lp = builder.group_window_lps(ref.group(T, J, steam_load=steam))[0]
    obj = _highs_objs([lp])[0]
    assert abs(obj - base[0]) > 1e-4 * abs(base[0]), (obj, base[0])  # the higher load binds: the two optima differ
    res, ks, _ = _solve(gpu_solver, [lp])
    _only_band(ks, 1)
    _within_bars([lp], res, [obj])
    CS = 3 * T + J + 2 * T
    assert np.all(res[0].x[CS:CS + T] >= steam[0]) and np.all(res[0].x[CS + T:CS + 2 * T] >= ref.series(T, J)[6][0])


def _permuted(lp, T, seed):
    """The window with its heat rows in a random order among themselves, its >= rows likewise, and the entries of
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
    T, J = 65, 4
    lp = _case(T, J)[0][0]
    perm = _permuted(lp, T, 7)
    assert not np.array_equal(perm.indices, lp.indices)
    res, ks, _ = _solve(gpu_solver, [lp, perm])
    _only_band(ks, 2)
    assert res[0].status == 0 and res[1].status == 0
    assert abs(res[1].obj - res[0].obj) <= 1e-9 * abs(res[0].obj), (res[0].obj, res[1].obj)


def test_windows_outside_the_shape_are_handed_on(gpu_solver):
    T, J = 65, 4
    lps, objs = _case(T, J)
    hi = lps[1].u.copy()
    hi[3 * T + J + 2 * T + 20] = 200.0  # an upper bound of steam the kernel does not carry
    plain = builder.group_window_lps(ref.group(T, J, chp=False))  # the battery form's window
    batch = [dataclasses.replace(lps[1], u=hi)] + plain
    res, ks, _ = _solve(gpu_solver, batch)
    assert ks["band_windows"] == len(plain) and ks["ell_windows"] + ks["generic_windows"] == 1, ks
    _within_bars(batch, res, _highs_objs(batch))


def _slotless_cases(lp, T, J):
    """The window with, one at a time, a datum the kernel keeps no slot for made non-zero (or on's upper bound
    infinite): the device's structure check has to refuse each, or the form would solve another LP."""
    CE, m = 3 * T + J, lp.m
    dear = np.nonzero(lp.c[CE:CE + T] > 0.0)[0]   # steps where generating costs more than it saves: elec at its minimum
    cheap = np.nonzero(lp.c[CE:CE + T] < 0.0)[0]  # ... and where it pays: elec at the cap
    assert len(dear) >= 3 and len(cheap) >= 1

    def changed(field, j, v):
        a = getattr(lp, field).copy()
        a[j] = v
        return dataclasses.replace(lp, **{field: a})

    return {"q of a heat row": changed("q", T + 1 + dear[0], 5.0), "q of a ratio row": changed("q", m - 1, -20.0),
            "q of a generator row": changed("q", m - 3, -10.0), "l of on": changed("l", CE + T + 11, 0.5),
            "c of on": changed("c", CE + T + 12, 3.0), "u of on": changed("u", CE + T + dear[2], np.inf),
            "l of elec": changed("l", CE + dear[1], 250.0), "u of elec": changed("u", CE + cheap[0], 100.0)}


def test_data_without_a_slot_are_refused_on_the_device(gpu_solver):
    T, J = 65, 4
    lps, objs = _case(T, J)
    cases_ = _slotless_cases(lps[0], T, J)
    batch = list(cases_.values())
    want = _highs_objs(batch)
    moved = [abs(o - objs[0]) > 1e-5 * abs(objs[0]) for o in want]
    print("CHP slotless cases whose optimum differs from the window's:", dict(zip(cases_, moved)))
    assert sum(moved) >= 4, moved  # (a form that took these and dropped the datum would miss the bar; the count of
    # band windows below is the direct check for all eight)
    res, ks, _ = _solve(gpu_solver, batch + [lps[1]])
    assert ks["band_windows"] == 1 and ks["ell_windows"] + ks["generic_windows"] == len(batch), ks
    _within_bars(batch, res[:len(batch)], want)


def test_windows_above_the_on_chip_size_mixed_with_small_ones(gpu_solver):
    """Mode 7 also hands the form the heat-sized windows above n, m = 4096 (csrc/dvh_solve.cpp solve_packed), with one
    status read-back per batch: small and large CHP windows, a plain battery window and a large window the form refuses
    (a finite upper bound of steam), which goes on to the grid-wide path, in one batch."""
    small, so = _case(65, 4)
    large, lo_ = _case(768, 1)
    T, J = 768, 1
    hi = large[1].u.copy()
    hi[3 * T + J + 2 * T + 20] = 200.0
    refused = dataclasses.replace(large[1], u=hi)
    plain = builder.group_window_lps(ref.group(65, 4, chp=False))[:1]
    batch = [small[0], large[0], refused, plain[0], small[1], large[1]]
    want = [so[0], lo_[0], _highs_objs([refused])[0], _highs_objs(plain)[0], so[1], lo_[1]]
    res, ks, syncs = _solve(gpu_solver, batch)
    assert ks["band_windows"] == 5 and ks["large_windows"] == 1, ks
    assert ks["ell_windows"] == ks["generic_windows"] == ks["chain_windows"] == 0, ks
    _within_bars(batch, res, want)
    dres, dks, dsyncs = _solve(gpu_solver, batch, "default")
    assert dks["band_windows"] == 1 and dks["large_windows"] == 3 and dks["ell_windows"] + dks["generic_windows"] == 2, dks
    _within_bars(batch, dres, want)
    print(f"CHP mixed batch host syncs: chp {syncs} default {dsyncs}")
    assert res[3].obj == dres[3].obj and res[3].iters == dres[3].iters  # the battery window: the same kernel, the same result


def test_certify_1_works_through_the_after_pass(gpu_solver):  # (gpu_solver: the suite's no-GPU failure message)
    """An infeasible window that is not crossed bounds: a steam load at one step whose heat the unit cannot make,
    ehr (s + h) > cap.  The form runs it to the iteration limit; the certificate pass behind the solve proves it.
    The load is 5,000: the pass finds the ray of so plain a case at its first test, 64 iterations.  A marginal one is
    beyond its iteration cap whatever kernel ran the window before it -- its numpy restatement, certify_ref.certify,
    leaves s = 400 (0.8 x 430 = 344 kW against 300) undecided after all 65,536 iterations and needs 59,520 for
    s = 1,000."""
    import certify_ref as cr
    from dervet_hip import BatchSolver
    T, J = 48, 1
    lps, objs = _case(T, J)
    steam = ref.series(T, J)[5].copy()
    steam[1, 24] = 5000.0  # 0.8 (5000 + h) > 300
    bad = builder.group_window_lps(ref.group(T, J, steam_load=steam))[1]
    assert np.all(bad.l <= bad.u)
    batch = [lps[0], bad]
    assert cr.highs_status(batch[1])[0] == 2
    with BatchSolver(0, certify=1) as s:
        s.set_kernel_path("chp")
        res = s.solve(batch)
        ks, st = s.kernel_stats(), s.certify_stats()
    _only_band(ks, 2)
    _within_bars(batch[:1], res[:1], objs[:1])
    assert res[1].status_name == "infeasible", (res[1].status_name, res[1].iters)
    margin, viol = cr.farkas(batch[1], res[1].y)
    assert margin > 0.0 and viol <= 1e-8 * margin, (margin, viol)
    assert st["primal_infeasible"] == 1 and st["examined"] == 1, st


def test_warm_start_from_own_solution_takes_fewer_iterations(gpu_solver):
    lps, objs = _case(129, 1)
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
