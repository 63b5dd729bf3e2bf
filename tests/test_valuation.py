"""Scenario valuation, host form (dervet_hip/valuation.py bill_windows_host, value_scenarios_host: the numpy statement
of the kernels' operations) pinned to the reference's golden bills, pro forma, npv, payback and cost-benefit files of
Usecase 2 es and es + PV + DG (tests/golden/uc2_bills.json, uc2_payback.json).  The device form is checked against this
one in tests/test_gpu_valuation.py, the C++ form (csrc/dvh_cba.h) in tests/test_valuation_native.py.

Bars: the bill of the golden dispatch against the golden bill columns 1e-12 relative (tests/test_benefit.py's bar for
the original charges; the dispatch columns are stored at full precision).  The valuation is fed the golden pro forma's
own 2017 values, which are rounded to five decimals of ~1e5 $: columns, yearly net, npv row and the two present values
1e-9 relative, payback and discounted payback 1e-8, IRR 1e-9 absolute (the rounding alone leaves ~1.3e-10, 4e-12 and
1.4e-10 respectively).
"""
import json
import os

import numpy as np
import pytest

from dervet_hip import valuation as V
from dervet_hip.lp import scenarios
from oracle import cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXTRA = ("Tax Credit", "Other Incentives", "User Constraints Value")
NAMES = ["es", "es+pv+dg"]


def golden(name):
    with open(os.path.join(GOLDEN, "uc2_bills.json")) as f:
        b = json.load(f)[name]
    with open(os.path.join(GOLDEN, "uc2_payback.json")) as f:
        p = json.load(f)[name]
    return b, p


def golden_groups(name):
    """The case's 12 monthly window groups (product builder), its oracle windows and series."""
    wins, arr, meta, _ = cases.case_windows(name)
    bat = cases.battery_from_params(meta["params"])
    p = meta["params"]
    gen = None
    if "PV" in p and p["PV"].get("curtail", "0") in ("0", "0.0"):
        gen = float(p["PV"]["rated_capacity"]) * np.nan_to_num(arr["pv_profile"])
    groups = scenarios.windows_by_period(2017, 1.0, arr["site_load"][None], None if gen is None else gen[None], bat,
                                         tariff_def=meta["tariff"], ene_min=arr["agg_emin"][None],
                                         ene_max=arr["agg_emax"][None])
    return groups, wins, arr


def golden_financials(b):
    """Financials of a golden case from its pro forma: capital cost (every "Capital Cost" column), fixed O&M, the
    three extra columns, the value streams' growth rates and the discount rate."""
    pf = b["proforma"]
    capex = -sum(pf[k][0] for k in pf if k.endswith("Capital Cost"))
    fixed = -[pf[k][1] for k in pf if k.endswith("Fixed O&M Cost")][0]
    return V.Financials(years=len(b["proforma_index"]) - 1, opt_years=(0,), rate=b["npv_discount_rate"] / 100.0,
                        growth=[b["growth"]["retailTimeShift"], b["growth"]["DCM"], 0.0, 0.0, 0.0], capex=capex,
                        fixed_om=fixed, extra=np.array([pf[k] for k in EXTRA]))


def one_window_bills(avoided_energy, avoided_demand):
    """A bill table of one row whose avoided charges are the given ones."""
    r = np.zeros((1, V.BILL_ROWS))
    r[0, V.ORIG_RETAIL], r[0, V.ORIG_DEMAND] = avoided_energy, avoided_demand
    return r


def np_irr(values):
    """numpy.irr (numpy < 1.20) restated: the real root of the NPV polynomial with rate > -1 nearest to rate 0."""
    res = np.roots(np.asarray(values, np.float64)[::-1])
    res = res[(res.imag == 0) & (res.real > 0)].real
    if len(res) == 0:
        return np.nan
    rate = 1.0 / res - 1.0
    return float(rate[np.argmin(np.abs(rate))])


def check_against_golden(val, b, p):
    """The bars of this module's docstring on a Valuation (numpy) of one scenario fed the golden 2017 values."""
    pf, gp = val.proforma[0], b["proforma"]
    cols = {"Avoided Energy Charge": pf[:, 1], "Avoided Demand Charge": pf[:, 2], "Fixed O&M": pf[:, 6],
            "Capital Cost": pf[:, 0]}
    want = {"Avoided Energy Charge": np.array(gp["Avoided Energy Charge"]),
            "Avoided Demand Charge": np.array(gp["Avoided Demand Charge"]),
            "Fixed O&M": np.array([gp[k] for k in gp if k.endswith("Fixed O&M Cost")][0]),
            "Capital Cost": np.sum([gp[k] for k in gp if k.endswith("Capital Cost")], axis=0)}
    for j, k in enumerate(EXTRA):
        cols[k], want[k] = pf[:, V.FIXED_COLS + j], np.array(gp[k])
    for k in cols:
        np.testing.assert_allclose(cols[k], want[k], rtol=1e-9, atol=0.0, err_msg=k)
    assert not pf[:, 3:6].any()  # DA value, variable O&M, fuel: zero in the goldens
    for k in gp:  # every golden column that is not restated is zero
        if k not in want and not k.endswith(("Capital Cost", "Fixed O&M Cost")) and k != "Yearly Net Value":
            assert not np.any(gp[k]), k
    net = pf.sum(axis=1)
    np.testing.assert_allclose(net, gp["Yearly Net Value"], rtol=1e-9)
    rate = b["npv_discount_rate"] / 100.0
    disc = (1.0 + rate) ** np.arange(len(net))
    gn = b["npv"]
    assert val.npv[0] == pytest.approx(gn["Lifetime Present Value"], rel=1e-9)
    assert np.sum(pf[:, 1] / disc) == pytest.approx(gn["Avoided Energy Charge"], rel=1e-9)
    assert np.sum(pf[:, 2] / disc) == pytest.approx(gn["Avoided Demand Charge"], rel=1e-9)
    assert np.sum(pf[:, 6] / disc) == pytest.approx([gn[k] for k in gn if k.endswith("Fixed O&M Cost")][0], rel=1e-9)
    for j, k in enumerate(EXTRA):
        assert np.sum(pf[:, V.FIXED_COLS + j] / disc) == pytest.approx(gn[k], rel=1e-9)
    pay = p["payback"]
    assert val.payback[0] == pytest.approx(pay["Payback Period"], rel=1e-8)
    if pay["Discounted Payback Period"] is None:
        assert np.isnan(val.discounted_payback[0])
    else:
        assert val.discounted_payback[0] == pytest.approx(pay["Discounted Payback Period"], rel=1e-8)
    assert val.irr[0] == pytest.approx(pay["Internal Rate of Return"], abs=1e-9)
    assert val.irr[0] == pytest.approx(np_irr(gp["Yearly Net Value"]), abs=1e-9)
    assert val.irr[0] == pytest.approx(np_irr(net), abs=1e-9)
    life = p["cost_benefit"]["Lifetime Present Value"]
    assert val.pv_cost[0] == pytest.approx(life["cost"], rel=1e-9)
    assert val.pv_benefit[0] == pytest.approx(life["benefit"], rel=1e-9)
    # benefit / cost (CBA.py:510-523); the payback file's column is the inverse, from an older reference version
    assert val.bc_ratio[0] == pytest.approx(life["benefit"] / life["cost"], rel=1e-9)
    assert 1.0 / val.bc_ratio[0] == pytest.approx(pay["Cost-Benefit Ratio"], rel=1e-9)
    assert val.npv[0] == pytest.approx(pay["Lifetime Net Present Value"], rel=1e-9)
    assert val.valid[0] == 1


def golden_dispatch_bills(name):
    """bill_windows_host over the 12 windows with the golden dispatch written into x: [12, BILL_ROWS]."""
    groups, wins, arr = golden_groups(name)
    rows = []
    for g, w in zip(groups, wins):
        sel, T = w["index"], g.T
        x = np.zeros((1, g.n))
        x[0, :T], x[0, T:2 * T], x[0, 2 * T:3 * T] = arr["golden_ch"][sel], arr["golden_dis"][sel], arr["golden_ene"][sel]
        x[0, 3 * T:] = -1e9  # tau: the bill must take the dispatch's own peaks
        bills, peaks, bad = V.bill_windows_host(V.bill_inputs(g, orig=w["load"][None]), x)
        assert not bad.any() and peaks.shape == (1, g.J)
        rows.append(bills[0])
    return np.array(rows)


@pytest.mark.parametrize("name", NAMES)
def test_host_bill_of_the_golden_dispatch_reproduces_the_golden_bills(name):
    b, _ = golden(name)
    rows = golden_dispatch_bills(name)
    for key, col in (("original_energy_charge", V.ORIG_RETAIL), ("original_demand_charge", V.ORIG_DEMAND),
                     ("energy_charge", V.RETAIL), ("demand_charge", V.DEMAND)):
        np.testing.assert_allclose(rows[:, col], b[key], rtol=1e-12, err_msg=key)
    assert not rows[:, [V.DA, V.ORIG_DA, V.FUEL]].any()
    # the year's avoided charges are the golden pro forma's 2017 row
    ae, ad = (rows[:, V.ORIG_RETAIL] - rows[:, V.RETAIL]).sum(), (rows[:, V.ORIG_DEMAND] - rows[:, V.DEMAND]).sum()
    assert ae == pytest.approx(b["proforma"]["Avoided Energy Charge"][1], rel=1e-9)
    assert ad == pytest.approx(b["proforma"]["Avoided Demand Charge"][1], rel=1e-9)


@pytest.mark.parametrize("name", NAMES)
def test_host_valuation_of_the_golden_values_reproduces_proforma_npv_payback_irr(name):
    b, p = golden(name)
    bills = one_window_bills(b["proforma"]["Avoided Energy Charge"][1], b["proforma"]["Avoided Demand Charge"][1])
    val = V.value_scenarios_host(bills, None, [0, 1], [0], [0], golden_financials(b))
    check_against_golden(val, b, p)


@pytest.mark.parametrize("name", NAMES)
def test_host_valuation_from_the_twelve_golden_bills(name):
    """The same from the 12 monthly bills of the golden dispatch (summed in CSR order)."""
    b, p = golden(name)
    rows = golden_dispatch_bills(name)
    val = V.value_scenarios_host(rows, np.zeros(12, np.int32), [0, 12], np.arange(12), np.zeros(12, int),
                                 golden_financials(b))
    check_against_golden(val, b, p)


def _value(fin, ae=1000.0, ad=500.0, years=(0,)):
    bills = np.concatenate([one_window_bills(ae, ad) for _ in years])
    return V.value_scenarios_host(bills, None, [0, len(years)], np.arange(len(years)), list(years), fin)


def test_one_year():
    v = _value(V.Financials(years=1, rate=0.05, capex=1000.0))
    assert v.proforma.shape == (1, 2, 7)
    assert v.npv[0] == pytest.approx(-1000.0 + 1500.0 / 1.05, rel=1e-14)
    assert v.payback[0] == pytest.approx(1000.0 / 1500.0, rel=1e-15)
    assert v.irr[0] == pytest.approx(0.5, abs=1e-12)


def test_all_positive_flows_have_no_irr():
    v = _value(V.Financials(years=10, rate=0.05, capex=-10.0))
    assert np.isnan(v.irr[0]) and v.npv[0] > 0 and v.pv_cost[0] == 0.0
    assert np.isnan(v.bc_ratio[0])


def test_first_year_that_earns_nothing_never_pays_back():
    for fixed in (1500.0, 2000.0):   # net_1 = 0, net_1 < 0
        v = _value(V.Financials(years=5, rate=0.05, capex=100.0, fixed_om=fixed))
        assert np.isnan(v.payback[0]) and np.isnan(v.discounted_payback[0])
        assert np.isfinite(v.npv[0])


def test_zero_capex_has_no_ratio():
    v = _value(V.Financials(years=5, rate=0.05, capex=0.0))
    assert np.isnan(v.bc_ratio[0]) and v.pv_cost[0] == 0.0 and v.payback[0] == 0.0
    assert v.discounted_payback[0] == 0.0 and np.isnan(v.irr[0])


def test_zero_rate_discounted_payback_is_the_payback():
    v = _value(V.Financials(years=5, rate=0.0, capex=3000.0))
    assert v.discounted_payback[0] == v.payback[0] == 2.0


def test_two_opt_years_with_a_gap_and_a_year_before_the_first():
    g = 1.0 + 2.5 / 100.0
    fin = V.Financials(years=6, opt_years=(1, 3), rate=0.07, growth=[2.5, 0.0, 0, 0, 0], capex=5000.0)
    bills = np.concatenate([one_window_bills(1000.0, 10.0), one_window_bills(50.0, 5.0), one_window_bills(2000.0, 20.0)])
    v = V.value_scenarios_host(bills, None, [0, 3], [0, 1, 2], [1, 1, 3], fin)
    assert v.valid[0] == 1
    np.testing.assert_allclose(v.proforma[0, 1:, 1], [1050.0 / g, 1050.0, 1050.0 * g, 2000.0, 2000.0 * g, 2000.0 * g * g],
                               rtol=1e-15)
    np.testing.assert_array_equal(v.proforma[0, 1:, 2], [15.0, 15.0, 15.0, 20.0, 20.0, 20.0])
    assert v.proforma[0, 0, 1] == 0.0 and v.proforma[0, 0, 0] == -5000.0


def test_validity_flag():
    fin = V.Financials(years=4, opt_years=(0, 2), rate=0.05, capex=100.0)
    bills = np.concatenate([one_window_bills(10.0, 1.0)] * 3)
    ok = V.value_scenarios_host(bills, np.zeros(3, np.int32), [0, 2, 3], [0, 1, 2], [0, 2, 0], fin)
    assert list(ok.valid) == [1, 0]                       # scenario 1 has no window of opt year 2
    flagged = V.value_scenarios_host(bills, np.array([0, 1, 0], np.int32), [0, 2], [0, 1], [0, 2], fin)
    assert list(flagged.valid) == [0]
    stray = V.value_scenarios_host(bills, None, [0, 3], [0, 1, 2], [0, 2, 1], fin)     # year 1 is not an opt year
    assert list(stray.valid) == [0]
    outside = V.value_scenarios_host(bills, None, [0, 3], [0, 1, 7], [0, 2, 2], fin)   # no bill row 7
    assert list(outside.valid) == [0] and np.isfinite(outside.npv[0])


def test_bad_window_bills_nan_and_keeps_its_original_rows():
    rng = np.random.default_rng(1)
    T, G = 30, 3
    inp = V.BillInputs(T=T, J=1, dt=1.0, dcm_t=np.arange(T, dtype=np.int32), dcm_j=np.zeros(T, np.int32),
                       base=rng.uniform(50, 90, (G, T)), retail=rng.uniform(0.1, 0.2, (G, T)),
                       demand=np.full((G, 1), 9.0), om=np.full(G, 2.0))
    x = rng.uniform(0, 5, (G, 3 * T + 1))
    full, _, bad0 = V.bill_windows_host(inp, x)
    bills, peaks, bad = V.bill_windows_host(inp, [x[0], x[1], x[2][:3 * T]], status=[0, 3, 0])
    assert list(bad0) == [0, 0, 0] and list(bad) == [0, 1, 1]
    assert np.array_equal(bills[0], full[0]) and np.isnan(bills[1:, :5]).all() and np.isnan(peaks[1:]).all()
    assert np.array_equal(bills[:, 5:], full[:, 5:])
    assert full[0, V.ORIG_RETAIL] == pytest.approx(np.sum(inp.retail[0] * inp.base[0]), rel=1e-14)
    assert full[0, V.ORIG_DEMAND] == 9.0 * inp.base[0].max()
