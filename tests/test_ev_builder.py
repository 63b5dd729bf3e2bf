"""CPU: builder.battery_group(ev=...) -- one electric vehicle, dervet MicrogridDER/ElectricVehicles.py ElectricVehicle1
-- against the dense restatement of the reference's own rows in tests/ev_ref.py and HiGHS.  The builder lays the rows
out in the load-shift kernel's shape (cycles, bounded ev_ene, a free start on the trailing session), the restatement
keeps the reference's (free ev_ene, rows as written there): the two LPs differ row for row and must agree on the
optimum and on feasibility."""
import numpy as np
import pytest

import ev_ref as ref
from dervet_hip.lp import builder, gpu_builder, scenarios
from oracle import window_lp
from planted_lp import from_window

SMALL = [s for s in ref.SHAPES if s[0] <= 129]
SMALL_IDS = [i for s, i in zip(ref.SHAPES, ref.IDS) if s[0] <= 129]
FIELDS = ("indptr", "indices", "data", "c", "c0", "q", "l", "u")


def _both(T, J, pl, tg, k):
    w = builder.group_window_lps(ref.group(T, J, pl, tg))[k]
    return window_lp.solve_highs(from_window(w)), window_lp.solve_highs(ref.dense_of(T, J, pl, tg, k))


@pytest.mark.parametrize("T,J,pl,tg", ref.SHAPES, ids=ref.IDS)
def test_layout_and_the_load_shift_form_accepts_it(T, J, pl, tg):
    g = ref.group(T, J, pl, tg)
    D = int(np.count_nonzero(g.ev["code"] & builder.EV_START))
    assert (g.n, g.m_eq, g.m) == (5 * T + J, 2 * T + 1 + D, 2 * T + 1 + D + len(g.inputs["dcm_t"]))
    assert g.inputs["has_ev"] and np.array_equal(g.inputs["ev_code"], g.ev["code"])
    for w in builder.group_window_lps(g):
        for i in range(w.m):  # the builder writes every row with sorted columns
            assert np.all(np.diff(w.indices[w.indptr[i]:w.indptr[i + 1]]) > 0), i
        assert np.all(np.diff(w.indptr[w.m_eq:]) == 4)
        assert ref.shift_form_accepts(w)


@pytest.mark.parametrize("T,J,pl,tg", ref.SHAPES, ids=ref.IDS)
def test_highs_objectives_agree_with_the_reference_rows(T, J, pl, tg):
    for k in range(2 if T <= 129 else 1):
        a, b = _both(T, J, pl, tg, k)
        assert a["status"] == 0 and b["status"] == 0, (a["message"], b["message"])  # the shape is feasible
        print(f"EV T{T}J{J} window {k}: builder {a['obj']:.9f} reference rows {b['obj']:.9f}")
        assert abs(a["obj"] - b["obj"]) <= 1e-9 * abs(b["obj"]), (k, a["obj"], b["obj"])


@pytest.mark.parametrize("T,J,pl,tg", SMALL, ids=SMALL_IDS)
def test_an_unreachable_target_is_infeasible_in_both(T, J, pl, tg):
    a, b = _both(T, J, pl, 1000.0, 0)
    assert a["status"] == 2 and b["status"] == 2, (a["status"], b["status"])


@pytest.mark.parametrize("T,J,pl,tg", SMALL, ids=SMALL_IDS)
def test_terms_sum_to_the_objective_and_ev_energy_is_the_reference_state(T, J, pl, tg):
    g = ref.group(T, J, pl, tg)
    xs = []
    for w in builder.group_window_lps(g):
        h = window_lp.solve_highs(from_window(w))
        assert h["status"] == 0
        xs.append(h["x"])
    x = np.array(xs)
    terms = builder.evaluate_terms(g, x)
    total, want = sum(terms.values()), (g.c * x).sum(axis=1) + g.c0
    assert np.all(np.abs(total - want) <= 1e-9 * np.abs(want)), (total, want)
    assert list(g.terms)[-2:] == ["ev retailETS", "ev fixed_om"] and np.array_equal(terms["ev fixed_om"], [3.0, 3.0])
    e = builder.ev_energy(g, x)
    _, plug_out = ref.plug_steps(pl)
    for k in range(g.G):
        ev_ch = x[k, 3 * T + J:4 * T + J]
        assert np.all(ev_ch[~pl] <= 1e-9)
        state = ref.state_of(pl, 1.0, ev_ch)
        assert np.allclose(e[k, pl], state[pl], rtol=0.0, atol=1e-6 * tg), k
        assert np.allclose(e[k, plug_out], tg, rtol=0.0, atol=1e-6 * tg)  # the reference's ev_ene_p = ene_target
        others = ~pl
        others[plug_out] = False
        assert not e[k, others].any()
        for p in plug_out:  # every session that ends inside the window collects the target
            assert abs(state[p - 1] + ev_ch[p - 1] - tg) <= 1e-6 * tg, (k, p)


def test_the_trailing_session_charges_at_negative_prices():
    T, J, pl, tg = ref.SHAPES[4]
    assert T == 72 and pl[66:].all() and not pl[65]
    a, _ = _both(T, J, pl, tg, 0)
    assert a["x"][3 * T + J + 66:4 * T + J].sum() > 1.0


def test_ev_none_returns_the_plain_group_bit_for_bit():
    T, J, pl, tg = ref.SHAPES[5]
    load, retail, masks, dprice = ref.series(T, J)
    kw = dict(retail_price=retail, demand_masks=masks, demand_prices=dprice)
    plain, g = builder.battery_group(T, 1.0, load, ref.BAT, **kw), builder.battery_group(T, 1.0, load, ref.BAT, ev=None, **kw)
    for f in FIELDS:
        a, b = getattr(g, f), getattr(plain, f)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert (g.m_eq, list(g.terms), g.ev) == (plain.m_eq, list(plain.terms), None)
    assert "has_ev" not in g.inputs


def test_scalar_and_per_window_ratings():
    T, J, pl, tg = ref.SHAPES[1]
    g = ref.group(T, J, pl, np.array([120.0, 90.0]), ch_max=np.array([50.0, 40.0]))
    ee = 4 * T + J
    assert np.array_equal(g.u[:, ee], [120.0, 90.0]) and np.array_equal(g.u[:, ee + T - 1], [150.0, 120.0])  # R = 3 dt ch_max
    assert np.array_equal(g.u[:, ee - T:ee], np.where(pl, np.array([[50.0], [40.0]]), 0.0))
    assert not g.l[:, ee - T:].any()


def test_refused_combinations_and_masks_raise():
    T = 24
    load, retail, masks, dprice = ref.series(T, 1)
    ev = dict(ch_max=50.0, ene_target=100.0, plugged=ref.hours(T, 18, 7))
    ice = dict(rated_power=300.0, n=1.0, min_power=100.0, efficiency=0.0866, fuel_cost=3.5, variable_om_cost=0.0)
    cl = dict(rated_power=150.0, duration=4.0, day_starts=[0])
    for kw in (dict(ice=ice), dict(poi=dict(max_import=-650.0, max_export=0.0)), dict(pv_curtail_max=np.ones((2, T))),
               dict(grid_charge=False, pv_gen=np.ones((2, T))), dict(ctrl_load=cl)):
        with pytest.raises(NotImplementedError):
            builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice,
                                  ev=ev, **kw)
    with pytest.raises(NotImplementedError):
        gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, retail_price=retail, ev=ev, ice=ice)
    one = lambda on: np.isin(np.arange(T), on)  # noqa: E731
    bad = [np.ones(T, bool),                    # never unplugged: no session ends inside the window
           np.zeros(T, bool),                   # never plugged
           one([20, 21, 22, 23]),               # only a session cut by the window's end
           one([3, 4, 6, 7]),                   # a one-step unplugged gap between two sessions
           np.ones(T + 1, bool), one([3])[:T - 1]]  # not of length T
    for pl in bad:
        with pytest.raises(ValueError):
            builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, ev=dict(ev, plugged=pl))
    builder.battery_group(T, 1.0, load, ref.BAT, retail_price=retail, ev=dict(ev, plugged=one([3, 4, 22])))  # a gap at T - 1 is none


def test_the_spec_has_the_groups_shape():
    for T, J, pl, tg in ref.SHAPES[:6]:
        load, retail, masks, dprice = ref.series(T, J)
        ev = dict(ch_max=ref.CH_MAX, ene_target=tg, fixed_om=3.0, plugged=pl)
        s = gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks,
                                           demand_prices=dprice, ev=ev)
        g = ref.group(T, J, pl, tg)
        assert (s.n, s.m, s.m_eq, s.nnz) == (g.n, g.m, g.m_eq, len(g.indices))
        assert s.c0.tobytes() == g.c0.tobytes()
        assert np.array_equal(gpu_builder.desc_of([s])[0], builder.pack_groups([g]).desc)


def test_sizing_refuses_these_windows():
    from dervet_hip import value_sizing
    T, J, pl, tg = ref.SHAPES[0]
    load, retail, masks, dprice = ref.series(T, J)
    s = gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, retail_price=retail, demand_masks=masks, demand_prices=dprice,
                                       ev=dict(ch_max=ref.CH_MAX, ene_target=tg, plugged=pl))
    with pytest.raises(NotImplementedError, match="EV"):
        value_sizing._Resident([s], None, "cpu")


def test_config4_ev_masks_follow_the_calendar():
    groups = scenarios.config4_ev(range(2), only=[1])
    plain = scenarios.config4(range(2), only=[1])
    assert len(groups) == 1
    g, p = groups[0], plain[0]
    T = 28 * 24
    hour = np.arange(T) % 24  # February 2017 starts at hour 0 of a day
    assert (g.T, g.J, g.G) == (T, p.J, 2)
    assert np.array_equal(g.ev["plugged"], (hour >= 18) | (hour < 7))
    D = int(np.count_nonzero(g.ev["code"] & builder.EV_START))
    # 28 sessions end inside the window (the first one cut by its start), each with its plug-out step and the rest
    # of that day as cycles of their own; the session cut by the window's end has no start row
    assert D == 3 * 28 and np.count_nonzero(g.ev["code"] & builder.EV_TRAIL) == 6
    assert (g.n, g.m_eq, g.m) == (p.n + 2 * T, 2 * T + 1 + D, p.m + T + D)
    day = scenarios.config4_ev(range(1), ch_max=[30.0], ene_target=[90.0], plugin_hour=9, plugout_hour=17, only=[0])[0]
    hour = np.arange(day.T) % 24
    assert np.array_equal(day.ev["plugged"], (hour >= 9) & (hour < 17))
    assert np.array_equal(day.ev["ch_max"], [30.0]) and np.array_equal(day.ev["ene_target"], [90.0])
    assert ref.shift_form_accepts(builder.group_window_lps(day)[0])
    spec = scenarios.config4_ev(range(2), only=[1], spec=True)[0]
    assert np.array_equal(spec.ev["code"], g.ev["code"]) and (spec.n, spec.m, spec.nnz) == (g.n, g.m, len(g.indices))
