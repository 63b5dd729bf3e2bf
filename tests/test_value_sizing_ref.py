"""Economic sizing on the CPU against the reference's Usecase 1 goldens (tests/golden/uc1_sizing.*, from
Results/Usecase1/<case>/{sizeuc3, objective_valuesuc3}.csv): the annuity scalar, the restated year window at the golden
size, the monolithic relaxed sizing LP (tests/value_sizing_ref.py) and the cutting-plane loop restated with HiGHS duals
(dervet_hip.value_sizing.loop_host).  Sizes are judged by the reference's own 3 % bar (MAX_PERCENT_ERROR,
test_beta_release_validation_report.py:41): the objective is flat near the optimum, so a loop that stops at a relative
gap of 1e-6 may sit tens of kWh from the LP's vertex; objectives are judged tightly."""
import numpy as np
import pytest

import value_sizing_cases as C
import value_sizing_ref as R
from dervet_hip import annuity_scalar
from dervet_hip import value_sizing as VS


@pytest.fixture(scope="module")
def es():
    positions, specs, meta = C.uc1("es")
    return dict(positions=positions, spec=specs[0], meta=meta)


@pytest.fixture(scope="module")
def es_mono(es):
    return R.monolithic(es["positions"], 0, es["spec"])


def test_annuity_scalar_is_the_golden_one(es):
    alpha = annuity_scalar(2017, 2037, [2017], 0.022, 0.06)
    assert abs(alpha - 14.454006150790663) <= 1e-12 * alpha
    assert alpha == es["spec"].alpha
    g, size = es["meta"]["golden_objective"], es["meta"]["golden_size"]
    assert abs(alpha - g["es fixed_om"] / (10.0 * size["Discharge Rating (kW)"])) <= 1e-12 * alpha
    assert g["escapex"] == 800.0 * size["Discharge Rating (kW)"] + 250.0 * size["Energy Rating (kWh)"]
    # an opt year inside the horizon: inflated after it, deflated before it, discounted from k = 0
    want = sum((1.022 ** (k - 2)) / 1.06 ** k for k in range(5))
    assert abs(annuity_scalar(2017, 2022, [2019], 0.022, 0.06) - want) <= 1e-14 * want


@pytest.mark.parametrize("name", ["es", "es+pv"])
def test_golden_size_reproduces_the_golden_objective_terms(name):
    positions, specs, meta = C.uc1(name)
    size, g = meta["golden_size"], meta["golden_objective"]
    lp = R.window_lp(positions[0], 0, size["Energy Rating (kWh)"], size["Discharge Rating (kW)"])
    h = R.solve_highs(lp)
    assert h["ok"]
    T = lp["T"]
    dcm = float(lp["c"][3 * T:] @ h["x"][3 * T:])
    a = specs[0].alpha
    print(f"{name}: alpha DCM {a * dcm!r} (golden {g['DCM']!r}) alpha retailETS {a * (h['obj'] - dcm)!r} (golden {g['retailETS']!r})")
    # the two terms trade against each other along the optimal face: their sum is what the optimum pins
    assert abs(a * h["obj"] - (g["DCM"] + g["retailETS"])) <= 1e-9 * (g["DCM"] + g["retailETS"])
    assert abs(a * dcm - g["DCM"]) <= 1e-9 * g["DCM"]
    assert abs(a * (h["obj"] - dcm) - g["retailETS"]) <= 1e-9 * g["retailETS"]


@pytest.mark.slow
def test_monolithic_optimum_rounds_up_to_the_golden_size(es, es_mono):
    m, size, g = es_mono, es["meta"]["golden_size"], es["meta"]["golden_objective"]
    print(f"monolithic E {m['E']!r} P {m['P']!r} objective {m['obj']!r}; golden total {sum(g.values())!r}")
    assert m["ok"]
    assert np.ceil(m["E"] - 1e-7 * m["E"]) == size["Energy Rating (kWh)"] == 11958.0
    assert np.ceil(m["P"] - 1e-7 * m["P"]) == size["Discharge Rating (kW)"] == 1993.0
    # the golden total is the integer optimum: above the relaxed one, by less than one unit of each size costs
    total = sum(g.values())
    assert m["obj"] <= total <= m["obj"] + es["spec"].c_energy + es["spec"].c_power


@pytest.mark.slow
def test_restated_loop_reaches_the_monolithic_optimum_of_usecase1(es, es_mono):
    s, size = es["spec"], es["meta"]["golden_size"]
    r = VS.loop_host(R.evaluate_highs(es["positions"], 0), s)
    opt = es_mono["obj"]
    print(f"loop: {r.status_name} rounds {r.rounds} cuts {r.n_cuts} E {r.energy_lp!r} -> {r.energy} P {r.power_lp!r} -> {r.power} "
          f"lower - opt {r.lower - opt:.3e} upper - opt {r.upper - opt:.3e}")
    assert r.status == VS.SIZED
    tol = s.gap_tol * (1.0 + abs(opt))
    assert r.lower <= opt + 1e-9 * abs(opt) and r.upper >= opt - 1e-9 * abs(opt)   # exact duals: true bounds
    assert r.upper - opt <= tol
    assert abs(r.energy - size["Energy Rating (kWh)"]) <= 0.03 * size["Energy Rating (kWh)"]
    assert abs(r.power - size["Discharge Rating (kW)"]) <= 0.03 * size["Discharge Rating (kW)"]


@pytest.mark.parametrize("cand", [1, 4], ids=["C1", "C4"])
def test_restated_loop_reaches_the_monolithic_optimum_of_the_seeded_cases(cand):
    """Interior optima, a box edge and the corner E = P = 0 (the cases the GPU tests size)."""
    positions, specs = C.small_cases(cand)
    for k, s in enumerate(specs):
        m = R.monolithic(positions, k, s)
        r = VS.loop_host(R.evaluate_highs(positions, k), s)
        tol = s.gap_tol * (1.0 + abs(m["obj"]))
        print(f"case {k}: rounds {r.rounds} cuts {r.n_cuts} E {r.energy_lp:.3f} (HiGHS {m['E']:.3f}) P {r.power_lp:.3f} "
              f"(HiGHS {m['P']:.3f}) lower - opt {r.lower - m['obj']:.3e} upper - opt {r.upper - m['obj']:.3e}")
        assert r.status == VS.SIZED
        assert r.lower <= m["obj"] + 1e-9 * abs(m["obj"]) and 0.0 <= r.upper - m["obj"] + 1e-9 * abs(m["obj"]) <= tol + 1e-9 * abs(m["obj"])
        assert abs(r.energy - m["E"]) <= 0.03 * m["E"] + 1.0 and abs(r.power - m["P"]) <= 0.03 * m["P"] + 1.0


def test_an_infeasible_size_ends_the_case():
    """sdr > 0 with P_max = 0 and E_min > 0: no window is feasible at any candidate."""
    from dataclasses import replace
    positions = C.positions([3], 1, 48, sdr=1.0)
    s = replace(C.spec(0.1, 1), power_max=0.0, energy_min=500.0)
    r = VS.loop_host(R.evaluate_highs(positions, 0), s)
    assert r.status == VS.LP_FAILED and np.isnan(r.energy)
