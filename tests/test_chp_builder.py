"""CPU: builder.battery_group(chp=...) -- one combined-heat-and-power unit with the site's steam and hot-water loads,
dervet MicrogridDER/CombinedHeatPower.py and MicrogridPOI.py:215-258 -- against the independent dense restatement of
tests/chp_ref.py and HiGHS, and the properties of the shared windows that chp_ref's docstring states."""
import numpy as np
import pytest

import chp_ref as ref
from dervet_hip.lp import builder, scenarios
from oracle import window_lp
from planted_lp import from_window


def _dense_of(T, J, k, G=2, seed=None, loads=True):
    load, retail, masks, dprice, fuel, steam, hot = ref.series(T, J, G, seed)
    return ref.dense(T, 1.0, load[k], ref.BAT, retail[k], masks, None if dprice is None else dprice[k], ref.CHP, fuel[k],
                     steam[k] if loads else None, hot[k] if loads else None)


def _solve(lp):
    h = window_lp.solve_highs(lp)
    assert h["status"] == 0, h["message"]
    return h


def _by_rows(lp):
    """The LP's rows as a sorted list of (equality?, right-hand side, ((column, value), ...)): the comparison up to the
    row order inside the equality block and inside the >= block."""
    K = lp["K"].tocsr()
    K.sort_indices()
    return sorted((i < lp["m_eq"], float(lp["q"][i]),
                   tuple(zip(K.indices[K.indptr[i]:K.indptr[i + 1]].tolist(), K.data[K.indptr[i]:K.indptr[i + 1]].tolist())))
                  for i in range(K.shape[0]))


@pytest.mark.parametrize("T,J", ref.SHAPES)
def test_builder_lp_equals_the_restatement(T, J):
    g = ref.group(T, J)
    mI = int(sum((np.arange(T) % (J + 1) == j).sum() for j in range(J)))  # DCM rows: ctrl_load_ref.series' masks
    assert (g.n, g.m_eq, g.m, g.inputs) == (7 * T + J, 2 * T + 1, 2 * T + 1 + mI + 3 * T, None)
    assert set(g.chp) >= {"cap", "pmin", "fuel_price", "steam_load", "hotwater_load"}
    # the documented row order: battery, heat rows, DCM rows, then per step cap / min / ratio
    lens = np.diff(g.indptr)
    assert np.all(lens[T + 1:2 * T + 1] == 3) and np.all(lens[2 * T + 1:2 * T + 1 + mI] == 4) and np.all(lens[2 * T + 1 + mI:] == 2)
    CE = 3 * T + J
    first = g.indices[g.indptr[2 * T + 1 + mI:-1]].reshape(T, 3)
    assert np.array_equal(first, np.stack([CE + np.arange(T), CE + np.arange(T), CE + 2 * T + np.arange(T)], axis=1))
    for k, w in enumerate(builder.group_window_lps(g)):
        for i in range(w.m):  # the builder writes every row with sorted columns
            assert np.all(np.diff(w.indices[w.indptr[i]:w.indptr[i + 1]]) > 0), i
        assert ref.heat_form_accepts(w)
        got, want = from_window(w), _dense_of(T, J, k)
        assert got["m_eq"] == want["m_eq"] and got["K"].shape == want["K"].shape
        assert _by_rows(got) == _by_rows(want)
        assert (got["K"] != want["K"]).nnz == 0  # (the restatement writes its rows in the builder's documented order)
        for key in ("q", "l", "u"):
            assert np.array_equal(got[key], want[key]), key
        # (elec's cost is a sum of three terms of up to 0.15 that cancel, added in another order: a few ulps of 0.15)
        assert np.allclose(got["c"], want["c"], rtol=1e-15, atol=1e-15)
        assert abs(got["c0"] - want["c0"]) <= 1e-12 * abs(want["c0"])


@pytest.mark.parametrize("T,J", ref.SHAPES)
def test_highs_objectives_agree_and_terms_sum_to_the_objective(T, J):
    g = ref.group(T, J)
    xs = []
    for k, w in enumerate(builder.group_window_lps(g)):
        a, b = _solve(from_window(w)), _solve(_dense_of(T, J, k))
        print(f"CHP T{T}J{J} window {k}: builder {a['obj']:.9f} restatement {b['obj']:.9f}")
        assert abs(a["obj"] - b["obj"]) <= 1e-9 * abs(b["obj"]), (k, a["obj"], b["obj"])
        xs.append(a["x"])
    x = np.array(xs)
    terms = builder.evaluate_terms(g, x)
    total = sum(terms.values())
    want = (g.c * x).sum(axis=1) + g.c0
    assert np.all(np.abs(total - want) <= 1e-9 * np.abs(want)), (total, want)
    assert {"chp naturalgas_fuel_cost", "chp variable_om", "chp fixed_om"} <= set(terms)
    load, retail, masks, dprice, fuel, steam, hot = ref.series(T, J)
    el = x[:, 3 * T + J:4 * T + J]
    assert np.allclose(terms["chp naturalgas_fuel_cost"], (fuel * el).sum(axis=1), rtol=1e-12)
    assert np.allclose(terms["chp variable_om"], ref.CHP["variable_om_cost"] * el.sum(axis=1), rtol=1e-12)
    assert np.all(terms["chp fixed_om"] == 0.0)


@pytest.mark.parametrize("T,J", [s for s in ref.SHAPES if s[0] >= 48])
def test_the_shared_windows_have_the_properties_chp_ref_states(T, J):
    load, retail, masks, dprice, fuel, steam, hot = ref.series(T, J)
    ratio, ehr, cap = ref.CHP["max_steam_ratio"], ref.CHP["electric_heat_ratio"], ref.CHP["rated_power"]
    must = ehr * (steam[0] + np.maximum(hot[0], steam[0] / ratio))
    assert must.max() < 136.0 < cap
    with_loads = _solve(_dense_of(T, J, 0))
    without = _solve(_dense_of(T, J, 0, loads=False))
    el = with_loads["x"][3 * T + J:4 * T + J]
    counts = (int((steam[0] / ratio > hot[0]).sum()), int((np.abs(el - must) < 1e-6).sum()), int((el > cap - 1e-6).sum()))
    share = (with_loads["obj"] - without["obj"]) / with_loads["obj"]
    print(f"CHP T{T}J{J}: ratio lifts {counts[0]} at must-run {counts[1]} at cap {counts[2]} loads cost {share:.3e}")
    assert counts == (ref.RATIO_LIFTS[T, J], ref.AT_MUST_RUN[T, J], ref.AT_CAP[T, J])
    assert ref.LOADS_COST[0] <= share <= ref.LOADS_COST[1]


def test_missing_loads_become_zeros_and_fixed_om_is_a_constant():
    T, J = 48, 1
    load, retail, masks, dprice, fuel, steam, hot = ref.series(T, J)
    g = builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice,
                              chp=dict(ref.CHP, fuel_price=fuel[0], fixed_om=[3.0, 4.0], steam_load=steam))
    CE = 3 * T + J
    assert np.array_equal(g.l[:, CE + 2 * T:CE + 3 * T], steam) and np.all(g.l[:, CE + 3 * T:] == 0.0)
    assert np.all(g.chp["hotwater_load"] == 0.0) and np.array_equal(g.chp["fuel_price"], np.stack([fuel[0], fuel[0]]))
    assert np.array_equal(g.terms["chp fixed_om"][1], [3.0, 4.0])
    plain = ref.group(T, J, loads=False)
    assert np.all(plain.l[:, CE + 2 * T:] == 0.0)
    k = 0
    a = _solve(from_window(builder.group_window_lps(plain)[k]))
    b = _solve(_dense_of(T, J, k, loads=False))
    assert abs(a["obj"] - b["obj"]) <= 1e-9 * abs(b["obj"])


def test_the_heat_form_check_refuses_what_the_kernel_keeps_no_slot_for():
    import dataclasses
    T, J = 5, 1
    w = builder.group_window_lps(ref.group(T, J))[0]
    CE = 3 * T + J

    def changed(field, j, v):
        a = getattr(w, field).copy()
        a[j] = v
        return dataclasses.replace(w, **{field: a})

    assert ref.heat_form_accepts(w)
    for field, j, v in (("u", CE + 1, 500.0), ("u", CE + 2 * T, 100.0), ("u", CE + 3 * T + 4, 100.0),  # elec / steam / hot
                        ("l", CE + 2, 1.0), ("l", CE + T + 2, 0.5), ("u", CE + T, np.inf), ("u", CE + T, 0.0),
                        ("c", CE + T + 3, 1.0), ("q", T + 1 + 2, 1.0), ("q", w.m - 1, -1.0), ("q", w.m - 3, 1.0)):
        assert not ref.heat_form_accepts(changed(field, j, v)), (field, j, v)
    assert ref.heat_form_accepts(changed("l", CE + 2 * T + 1, 75.0))  # a thermal load is any lower bound
    plain = builder.group_window_lps(ref.group(T, J, chp=False))[0]
    assert not ref.heat_form_accepts(plain)


def test_refused_combinations_raise():
    T = 24
    load, retail, masks, dprice, fuel, steam, hot = ref.series(T, 1)
    unit = dict(ref.CHP, fuel_price=fuel, steam_load=steam, hotwater_load=hot)
    ice = dict(rated_power=300.0, n=1.0, min_power=100.0, efficiency=0.0866, fuel_cost=3.5, variable_om_cost=0.0)
    pl = np.zeros(T, bool)
    pl[2:9] = True
    for kw in (dict(ice=ice), dict(poi=dict(max_import=-650.0, max_export=0.0)), dict(pv_curtail_max=np.ones((2, T))),
               dict(grid_charge=False, pv_gen=np.ones((2, T))),
               dict(ctrl_load=dict(rated_power=150.0, duration=4.0, day_starts=[0])),
               dict(ev=dict(ch_max=50.0, ene_target=100.0, plugged=pl))):
        with pytest.raises(NotImplementedError):
            builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice,
                                  chp=unit, **kw)


def test_valuation_device_builder_and_sizing_refuse_these_windows():
    from dervet_hip import valuation
    from dervet_hip.lp import gpu_builder
    T = 24
    load, retail, masks, dprice, fuel, steam, hot = ref.series(T, 1)
    unit = dict(ref.CHP, fuel_price=fuel, steam_load=steam, hotwater_load=hot)
    with pytest.raises(NotImplementedError):
        valuation.bill_inputs(ref.group(T, 1))
    with pytest.raises(NotImplementedError):
        gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks,
                                       demand_prices=dprice, chp=unit)
    with pytest.raises(NotImplementedError):
        scenarios.config4(range(1), spec=True, chp=dict(ref.CHP, fuel_price=0.08))


def test_config4_chp_groups_are_solved_by_highs():
    groups = scenarios.config4_chp(range(2), only=[1, 6])
    plain = scenarios.config4(range(2), only=[1, 6])
    assert len(groups) == 2
    for g, p in zip(groups, plain):
        T = g.T
        assert (g.T, g.J, g.G) == (p.T, p.J, 2) and (g.n, g.m_eq, g.m) == (p.n + 4 * T, 2 * T + 1, p.m + 4 * T)
        CE = 3 * T + g.J
        hour = np.arange(T) % 24  # (both windows start at midnight)
        assert np.array_equal(g.l[0, CE + 2 * T:CE + 3 * T], np.where((hour >= 8) & (hour < 18), 80.0, 32.0))
        assert set(np.unique(g.l[:, CE + 3 * T:])) == {45.0, 90.0}
        for w in builder.group_window_lps(g):
            assert ref.heat_form_accepts(w)
            _solve(from_window(w))
    feb, jul = groups
    assert np.all(feb.chp["fuel_price"] == 0.08 * 1.25) and np.all(jul.chp["fuel_price"] == 0.08)
    both = scenarios.config4_chp(range(2), rated_power=[200.0, 400.0], only=[0])[0]
    ion = 3 * both.T + both.J + both.T
    r_cap = both.indptr[both.m - 3 * both.T]  # the first step's cap row: (elec_0, on_0)
    assert np.array_equal(both.data[:, r_cap + 1], [200.0, 400.0]) and both.indices[r_cap + 1] == ion
