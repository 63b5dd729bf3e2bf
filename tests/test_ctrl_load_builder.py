"""CPU: builder.battery_group(ctrl_load=...) -- the controllable (load-shifting) load of dervet
MicrogridDER/LoadControllable.py -- against the independent dense restatement of tests/ctrl_load_ref.py and HiGHS."""
import numpy as np
import pytest

import ctrl_load_ref as ref
from dervet_hip.lp import builder, scenarios
from oracle import window_lp
from planted_lp import from_window

SMALL = [s for s in ref.SHAPES if s[0] <= 129]


def _dense_of(T, J, ds, k, G=2, seed=None):
    load, retail, masks, dprice = ref.series(T, J, G, seed)
    return ref.dense(T, 1.0, load[k], ref.BAT, retail[k], masks, None if dprice is None else dprice[k], ref.P, ref.DH, ds)


def _solve(lp):
    h = window_lp.solve_highs(lp)
    assert h["status"] == 0, h["message"]
    return h


@pytest.mark.parametrize("T,J,ds", ref.SHAPES)
def test_builder_lp_equals_the_restatement(T, J, ds):
    g = ref.group(T, J, ds)
    assert (g.n, g.m_eq, g.inputs) == (5 * T + J, 2 * T + 1 + len(ds), None)
    for k, w in enumerate(builder.group_window_lps(g)):
        for i in range(w.m):  # the builder writes every row with sorted columns
            assert np.all(np.diff(w.indices[w.indptr[i]:w.indptr[i + 1]]) > 0), i
        got, want = from_window(w), _dense_of(T, J, ds, k)
        assert got["m_eq"] == want["m_eq"]
        assert np.array_equal(got["K"].toarray(), want["K"].toarray())
        for key in ("q", "l", "u"):
            assert np.array_equal(got[key], want[key]), key
        assert np.allclose(got["c"], want["c"], rtol=1e-15, atol=0.0)
        assert abs(got["c0"] - want["c0"]) <= 1e-12 * abs(want["c0"])


@pytest.mark.parametrize("T,J,ds", SMALL)
def test_highs_objectives_agree_and_terms_sum_to_the_objective(T, J, ds):
    g = ref.group(T, J, ds)
    xs = []
    for k, w in enumerate(builder.group_window_lps(g)):
        a, b = _solve(from_window(w)), _solve(_dense_of(T, J, ds, k))
        assert abs(a["obj"] - b["obj"]) <= 1e-9 * abs(b["obj"]), (k, a["obj"], b["obj"])
        xs.append(a["x"])
    x = np.array(xs)
    total = sum(builder.evaluate_terms(g, x).values())
    want = (g.c * x).sum(axis=1) + g.c0
    assert np.all(np.abs(total - want) <= 1e-9 * np.abs(want)), (total, want)
    assert {"ctrl_load retailETS"} <= set(g.terms)


@pytest.mark.parametrize("T,J,ds", SMALL)
def test_the_load_never_raises_the_optimum(T, J, ds):
    with_load = builder.group_window_lps(ref.group(T, J, ds))
    without = builder.group_window_lps(ref.group(T, J, ds, rated_power=None))
    for a, b in zip(with_load, without):
        oa, ob = _solve(from_window(a))["obj"], _solve(from_window(b))["obj"]
        assert oa <= ob + 1e-9 * abs(ob), (oa, ob)


def test_the_load_strictly_lowers_the_5_1_window():
    """One window of seed 0: HiGHS gives 5236.49 without the load and 3448.94 with it."""
    a = _solve(from_window(builder.group_window_lps(ref.group(5, 1, [0, 2], G=1, seed=0))[0]))["obj"]
    b = _solve(from_window(builder.group_window_lps(ref.group(5, 1, [0, 2], G=1, seed=0, rated_power=None))[0]))["obj"]
    print(f"CTRL_LOAD (5, 1, [0, 2]) seed 0: without {b:.2f} with {a:.2f}")
    assert a < b - 1e-6 * abs(b), (a, b)
    assert abs(b - 5236.49) <= 0.01 and abs(a - 3448.94) <= 0.01, (a, b)


def test_pw_is_zero_on_one_step_days():
    for T, J, ds, one in ((3, 1, [0, 1], [0]), (64, 1, [0, 63], [63]), (6, 1, [0, 1, 2, 5], [0, 1, 5])):
        g = ref.group(T, J, ds)
        for w in builder.group_window_lps(g):
            x = _solve(from_window(w))["x"]
            assert np.all(np.abs(x[3 * T + J + np.array(one)]) <= 1e-9), (T, ds)


def test_duration_zero_returns_the_legacy_group_bit_for_bit():
    legacy = ref.group(48, 1, [0, 24], rated_power=None)
    for dur in (0.0, np.zeros(2)):
        g = ref.group(48, 1, [0, 24], duration=dur)
        for f in ("indptr", "indices", "data", "c", "c0", "q", "l", "u"):
            a, b = getattr(g, f), getattr(legacy, f)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
        assert (g.m_eq, list(g.terms), g.ctrl_load) == (legacy.m_eq, list(legacy.terms), None)
        assert g.inputs is not None


def test_refused_combinations_raise():
    T = 24
    load, retail, masks, dprice = ref.series(T, 1)
    cl = dict(rated_power=ref.P, duration=ref.DH, day_starts=[0])
    ice = dict(rated_power=300.0, n=1.0, min_power=100.0, efficiency=0.0866, fuel_cost=3.5, variable_om_cost=0.0)
    for kw in (dict(ice=ice), dict(poi=dict(max_import=-650.0, max_export=0.0)), dict(pv_curtail_max=np.ones((2, T))),
               dict(grid_charge=False, pv_gen=np.ones((2, T)))):
        with pytest.raises(NotImplementedError):
            builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice,
                                  ctrl_load=cl, **kw)
    for ds in ([1], [0, 5, 5], [0, T], []):
        with pytest.raises(ValueError):
            builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, ctrl_load=dict(cl, day_starts=ds))


def test_valuation_device_builder_and_sizing_refuse_these_windows():
    from dervet_hip import valuation
    from dervet_hip.lp import gpu_builder
    T = 24
    load, retail, masks, dprice = ref.series(T, 1)
    cl = dict(rated_power=ref.P, duration=ref.DH, day_starts=[0])
    with pytest.raises(NotImplementedError):
        valuation.bill_inputs(ref.group(T, 1, [0]))
    with pytest.raises(NotImplementedError):
        gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks,
                                       demand_prices=dprice, ctrl_load=cl)
    with pytest.raises(NotImplementedError):
        scenarios.config4(range(1), spec=True, ctrl_load=dict(rated_power=ref.P, duration=ref.DH))


def test_config4_load_shift_days_follow_the_calendar():
    groups = scenarios.config4_load_shift(range(2), rated_power=ref.P, duration=ref.DH, only=[1])
    plain = scenarios.config4(range(2), only=[1])
    assert len(groups) == 1
    g, p = groups[0], plain[0]
    assert (g.T, g.J, g.G) == (28 * 24, p.J, 2)
    assert np.array_equal(g.ctrl_load["day_starts"], np.arange(0, 28 * 24, 24))
    assert (g.n, g.m_eq, g.m) == (p.n + 2 * g.T, 2 * g.T + 1 + 28, p.m + g.T + 28)
    both = scenarios.config4_load_shift(range(2), rated_power=[100.0, 200.0], duration=[2.0, 0.0], only=[0])[0]
    el = 4 * both.T + both.J
    assert np.array_equal(both.u[:, el], [200.0, 0.0]) and np.array_equal(both.l[:, el - 1], [-100.0, -200.0])
