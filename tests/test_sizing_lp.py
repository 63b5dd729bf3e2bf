"""Reliability sizing on the CPU: the sizing LP of dervet_hip.lp.sizing (shapes, row and column order, windows past
the series end, refused inputs) and the loop restated in tests/sizing_ref.py (HiGHS + the oracle's outage
simulation) against the reference's golden sizes of its load-shedding sizing runs
(test/test_load_shedding/results/Sizing/{w_ls1,wo_ls1}/size_2mw_5hr.csv)."""
from dataclasses import replace

import numpy as np
import pytest
import scipy.sparse as sp

import sizing_ref
from dervet_hip import reliability
from dervet_hip.lp import sizing


def _small(N=40, **kw):
    rng = np.random.default_rng(3)
    case = reliability.OutageCase(critical_load=rng.uniform(200.0, 900.0, N).round(5), dt=1.0, max_outage_duration=24,
                                  ess=dict(rte=0.9, llsoc=0.1, ulsoc=0.95), soc_init=0.8,
                                  pv_max=[rng.uniform(0.0, 300.0, N)], pv_nu=[0.5], pv_gamma=[0.4], dg_power=[50.0],
                                  load_shed_pct=np.array([100.0, 80.0, 50.0] * 8))
    spec = reliability.SizingSpec(target_hours=3, ccost=7.0, ccost_kw=100.0, ccost_kwh=800.0, **kw)
    return case, spec


@pytest.mark.parametrize("K,L", [(1, 1), (2, 3), (13, 6)])
def test_shapes_follow_the_formulas(K, L):
    case, spec = _small()
    lp = sizing.sizing_lp(case, replace(spec, target_hours=L), list(range(K)))
    assert (lp.n, lp.m_eq, lp.m - lp.m_eq, len(lp.indices)) == (2 + 3 * K * L, K * L, 5 * K * L, 14 * K * L)
    assert lp.indptr[0] == 0 and lp.indptr[-1] == 14 * K * L and len(lp.indptr) == 6 * K * L + 1
    assert lp.c0 == 7.0 and lp.c[0] == 800.0 and lp.c[1] == 100.0 and not lp.c[2:].any()
    K_ = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))
    assert K_.has_sorted_indices or (np.diff(lp.indptr) <= 4).all()
    for r in range(lp.m):  # columns strictly increasing within every row (the solver rejects duplicates)
        cols = lp.indices[lp.indptr[r]:lp.indptr[r + 1]]
        assert (np.diff(cols) > 0).all()


def test_row_and_column_order_k2_l3():
    case, spec = _small()
    S = [5, 11]
    lp = sizing.sizing_lp(case, spec, S)
    A = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n)).toarray()
    L, dt, rte = 3, 1.0, 0.9
    ch = lambda w, k: 2 + 9 * w + k          # noqa: E731
    dis = lambda w, k: 2 + 9 * w + 3 + k     # noqa: E731
    s = lambda w, k: 2 + 9 * w + 6 + k       # noqa: E731
    # equality (w, k) = row 3 w + k;  k = 0 starts from min(soc_init, ulsoc) E
    row = np.zeros(lp.n)
    row[[0, ch(0, 0), dis(0, 0), s(0, 0)]] = [-0.8, -rte * dt, dt, 1.0]
    np.testing.assert_array_equal(A[0], row)
    row = np.zeros(lp.n)
    row[[ch(1, 2), dis(1, 2), s(1, 1), s(1, 2)]] = [-rte * dt, dt, -1.0, 1.0]
    np.testing.assert_array_equal(A[5], row)
    assert not lp.q[:6].any()
    # >= rows of (w, k) = (1, 1): rows 6 + 5 (3 + 1) ..
    r0 = 6 + 5 * 4
    want = [({0: 0.95, s(1, 1): -1.0}, 0.0), ({0: -0.1, s(1, 1): 1.0}, 0.0), ({1: 1.0, ch(1, 1): -1.0}, 0.0),
            ({1: 1.0, dis(1, 1): -1.0}, 0.0)]
    i = S[1] + 1
    _, _, _, pv_vari, _ = reliability.der_mix_properties(case)
    d = case.critical_load[i] * (80.0 / 100.0) - 50.0 - pv_vari[i]
    want.append(({ch(1, 1): -1.0, dis(1, 1): 1.0}, d))
    for j, (ent, q) in enumerate(want):
        row = np.zeros(lp.n)
        for col, v in ent.items():
            row[col] = v
        np.testing.assert_array_equal(A[r0 + j], row, err_msg=f"row {j}")
        assert lp.q[r0 + j] == q
    # bounds: sized E and P in [0, inf), dispatch in [0, inf)
    assert not lp.l.any() and np.isinf(lp.u).all()
    # soc_init above ulsoc: the window starts from ulsoc E
    lp2 = sizing.sizing_lp(replace(case, soc_init=1.0), spec, S)
    assert lp2.data[0] == -0.95


def test_window_past_the_series_end_has_no_demand_there():
    case, spec = _small()
    N = len(case.critical_load)
    lp = sizing.sizing_lp(case, spec, [N - 1, 3])
    d = lp.q[lp.m_eq + 4::5]
    assert d[0] != 0.0 and d[1] == 0.0 and d[2] == 0.0 and d[3:].all()
    x, st = sizing_ref.solve_highs(lp)
    assert st == 0 and x[0] > 0 and x[1] > 0
    with pytest.raises(ValueError, match="starts"):
        sizing.sizing_lp(case, spec, [N])
    with pytest.raises(ValueError, match="starts"):
        sizing.sizing_lp(case, spec, [])


def test_fixed_ratings_and_user_limits_are_bounds():
    case, spec = _small()
    c2 = replace(case, ess=dict(case.ess, E=5000.0, P_ch=700.0, P_dis=700.0))
    lp = sizing.sizing_lp(c2, replace(spec, size_power=False), [0])
    assert (lp.l[0], lp.u[0], lp.l[1], lp.u[1]) == (0.0, np.inf, 700.0, 700.0)
    lp = sizing.sizing_lp(c2, replace(spec, size_energy=False, user_power_min=10.0, user_power_max=9000.0), [0])
    assert (lp.l[0], lp.u[0], lp.l[1], lp.u[1]) == (5000.0, 5000.0, 10.0, 9000.0)


def test_refused_inputs():
    case, spec = _small()
    with pytest.raises(ValueError, match="nothing to size"):
        sizing.sizing_lp(case, replace(spec, size_energy=False, size_power=False), [0])
    with pytest.raises(ValueError, match="ccost_kwh"):
        sizing.sizing_lp(case, replace(spec, ccost_kwh=0.0), [0])
    with pytest.raises(ValueError, match="ccost_kw "):
        sizing.sizing_lp(case, replace(spec, ccost_kw=0.0), [0])
    sizing.sizing_lp(case, replace(spec, ccost_kw=0.0, size_power=False), [0])  # an unsized quantity needs no cost
    with pytest.raises(ValueError, match="P_ch == P_dis"):
        sizing.sizing_lp(replace(case, ess=dict(case.ess, P_ch=100.0, P_dis=200.0)), replace(spec, size_power=False), [0])
    with pytest.raises(ValueError, match="at least one step"):
        sizing.sizing_lp(case, replace(spec, target_hours=0.2), [0])
    with pytest.raises(ValueError, match="max_outage_duration"):
        sizing.sizing_lp(case, replace(spec, target_hours=30), [0])


def test_seed_is_a_stable_descending_sort_of_the_rolling_requirement():
    case, spec = _small()
    cl = np.asarray(case.critical_load)
    req = np.array([cl[t:t + 3].sum() for t in range(len(cl))])
    got = sizing.seed_starts(case, replace(spec, n_seed=5))
    assert set(got) == set(np.argsort(-req, kind="stable")[:5]) and len(got) == 5
    flat = replace(case, critical_load=np.full(12, 100.0))  # ties keep the series order; the tail sums fewer steps
    np.testing.assert_array_equal(sizing.seed_starts(flat, replace(spec, n_seed=12)), np.arange(12))


def test_candidate_rounding():
    assert sizing.candidate(10743.2275, 0.0) == 10744.0
    assert sizing.candidate(2737.0000001, 0.0) == 2737.0 and sizing.candidate(2737.0000001, 0.0, up=True) == 2738.0
    assert sizing.candidate(2736.99999, 0.0) == 2737.0
    assert sizing.candidate(12.3, 50.5) == 50.5 and sizing.candidate(-1e-9, 0.0) == 0.0


GOLDEN_ADDED = {"wo_ls1": [4282, 4807, 4951], "w_ls1": [4284, 4809, 4953]}


@pytest.mark.parametrize("name", sorted(GOLDEN_ADDED))
def test_cpu_loop_reproduces_the_golden_sizes(name):
    case, spec, gold = sizing_ref.golden_cases()[name]
    r = sizing_ref.golden_reference(name)
    assert (r.energy, r.power) == (gold["Energy Rating (kWh)"], gold["Discharge Rating (kW)"])
    assert gold["Charge Rating (kW)"] == gold["Discharge Rating (kW)"]
    assert r.status == "SIZED" and r.rounds == 4
    assert r.starts[:10] == [int(v) for v in sizing.seed_starts(case, spec)] and r.starts[10:] == GOLDEN_ADDED[name]
    assert not sizing_ref.near_integer(r, spec)


def test_golden_values():
    g = {n: m for n, (_, _, m) in sizing_ref.golden_cases().items()}
    assert (g["w_ls1"]["Discharge Rating (kW)"], g["w_ls1"]["Energy Rating (kWh)"]) == (2737.0, 8046.0)
    assert (g["wo_ls1"]["Discharge Rating (kW)"], g["wo_ls1"]["Energy Rating (kWh)"]) == (2737.0, 10744.0)
    assert all(m["target_hours"] == 4 and m["ccost_kw"] == 100 and m["ccost_kwh"] == 800 for m in g.values())


def test_round_limit_on_the_cpu():
    r = sizing_ref.golden_reference("wo_ls1", 1)
    assert (r.energy, r.power, r.status, r.rounds, len(r.starts)) == (10744.0, 2711.0, "ROUND_LIMIT", 1, 10)


def test_energy_only_with_the_golden_power_gives_the_golden_energy():
    case, spec, gold = sizing_ref.golden_cases()["wo_ls1"]
    c = replace(case, ess=dict(case.ess, P_ch=2737.0, P_dis=2737.0))
    r = sizing_ref.size_for_reliability(c, replace(spec, size_power=False))
    assert (r.energy, r.power, r.status) == (gold["Energy Rating (kWh)"], 2737.0, "SIZED")


def test_user_energy_min_above_the_need_is_the_size():
    case, spec, _ = sizing_ref.golden_cases()["wo_ls1"]
    r = sizing_ref.size_for_reliability(case, replace(spec, user_energy_min=20000.0))
    assert (r.energy, r.status) == (20000.0, "SIZED") and 0 < r.power <= 2737.0


@pytest.mark.parametrize("seed", sizing_ref.FAMILY_SEEDS)
def test_committed_family_seeds_qualify(seed):
    """The GPU comparison (tests/test_gpu_sizing.py) may leave out a case whose HiGHS optimum lies within 1e-3
    above an integer; for the committed seeds the CPU loop leaves out none, never stalls, and the family covers
    every option."""
    fam = sizing_ref.random_family(seed)
    refs = sizing_ref.family_reference(seed)
    for (c, s), r in zip(fam, refs):
        assert r.status == "SIZED" and 1 <= r.rounds <= 8
        assert not sizing_ref.near_integer(r, s)
    assert {(s.size_energy, s.size_power) for _, s in fam} == {(True, True), (True, False), (False, True)}
    assert {c.dt for c, _ in fam} == {1.0, 0.5} and any(c.pv_max for c, _ in fam) and any(c.dg_power for c, _ in fam)
    assert any(c.load_shed_pct is not None for c, _ in fam) and max(r.rounds for r in refs) > 1
