"""GPU: scenario valuation on the device (dvh_bill_windows, dvh_value_scenarios; dervet_hip/valuation.py) against the
numpy host form, against the reference's goldens, end to end on the solved golden windows, and over a seeded sweep.

Bars.  Kernel against host form on identical inputs: peaks and flags bit-equal, dollar rows within 1e-12 relative (a
tree sum over <= 1e5 same-sign FP64 terms is good to about log2(T) 2^-53, so 1e-12 leaves three orders of margin; the
two forms add in the same order and are in fact equal), IRR within 1e-10 absolute, NaN pattern exact.  Golden arithmetic
on the device: the CPU bars of tests/test_valuation.py.  End to end: 1e-4 against the goldens, the existing measured bar
of tests/test_gpu_benefit.py for the same solve.
"""
import functools

import numpy as np
import pytest

import test_valuation as TV
import valuation_cases as VC
from dervet_hip import valuation as V
from dervet_hip.lp import builder, scenarios
from dervet_hip.packed import PackedBatch
from dervet_hip.sweep import SeededSweep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def hand_batch(xs, status, lead=2):
    """A packed batch of `lead` dummy windows followed by one window per vector of xs, of which only what the bill
    reads is meaningful: descriptors, x, istats.  Returns (batch, first)."""
    import torch
    ns = [5] * lead + [len(x) for x in xs]
    W = len(ns)
    off = np.concatenate([[0], np.cumsum(ns)])
    desc = np.zeros((W, 8), np.int64)
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3] = ns, 1, 1, 1
    desc[:, 4], desc[:, 5], desc[:, 6], desc[:, 7] = 2 * np.arange(W), np.arange(W), off[:-1], np.arange(W)
    z = np.zeros
    pb = PackedBatch(desc=desc, indptr=z(2 * W, np.int32), indices=z(W, np.int32), data=z(W), c=z(int(off[-1])), c0=z(W),
                     q=z(W), l=z(int(off[-1])), u=z(int(off[-1]))).to_torch(DEV).alloc_outputs()
    pb.x.copy_(torch.as_tensor(np.concatenate([np.full(5, 1e300)] * lead + [np.asarray(x, np.float64) for x in xs])))
    pb.istats[:, 0] = torch.as_tensor(np.concatenate([np.zeros(lead, np.int32), np.asarray(status, np.int32)])).to(DEV)
    return pb, lead


def device_bills(solver, pb, first, inp):
    import torch
    b = V.bill_windows(solver, pb, [inp], first=first, peaks=True)
    torch.cuda.synchronize()
    return b.bills.cpu().numpy(), b.peaks[0].cpu().numpy(), b.bad.cpu().numpy()


@pytest.mark.parametrize("case", VC.bill_cases(), ids=lambda c: c["id"])
def test_bill_kernel_equals_the_host_form_on_identical_x(gpu_solver, case):
    """first > 0; one window not OPTIMAL; with G >= 3 one window whose descriptor reaches past x; two runs."""
    inp, x, status = case["inp"], case["x"], case["status"]
    pb, first = hand_batch(list(x), status)
    xs = list(x)
    if inp.G >= 3:
        pb.desc[first + 2, 6] = pb.x.numel() - 1          # window 2 now ends outside x: never read
        xs[2] = None
    want_b, want_p, want_f = V.bill_windows_host(inp, xs, status)
    got_b, got_p, got_f = device_bills(gpu_solver, pb, first, inp)
    assert np.array_equal(got_f, want_f)
    assert np.array_equal(got_p, want_p, equal_nan=True)                      # peaks: bit-equal
    assert np.array_equal(np.isnan(got_b), np.isnan(want_b))
    np.testing.assert_allclose(got_b, want_b, rtol=1e-12, atol=0.0)
    if inp.G >= 3:
        assert want_f[1] == want_f[2] == 1 and np.isnan(got_b[1:3, :5]).all() and np.isfinite(got_b[1:3, 5:]).all()
        assert np.isfinite(got_b[0]).all()
    again = device_bills(gpu_solver, pb, first, inp)
    for a, b in zip((got_b, got_p, got_f), again):
        assert np.array_equal(a, b, equal_nan=True)                            # run to run: the same bits


def test_bill_kernel_flags_a_demand_charge_row_that_names_no_step(gpu_solver):
    inp, x = VC.bill_group(65, 3, 3)
    inp.dcm_t = inp.dcm_t.copy()
    inp.dcm_t[4], inp.dcm_j[-1] = 65, 3
    pb, first = hand_batch(list(x), [0, 0, 0])
    want = V.bill_windows_host(inp, x)
    got = device_bills(gpu_solver, pb, first, inp)
    assert list(want[2]) == [2, 2, 2]
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def device_value(solver, case, proforma=True):
    import torch
    val = V.value_scenarios(solver, torch.as_tensor(case["bills"]).to(DEV), torch.as_tensor(case["bad"]).to(DEV),
                            case["ptr"], case["idx"], case["year"], case["fin"], proforma=proforma)
    assert val.values.is_cuda and val.valid.is_cuda
    torch.cuda.synchronize()
    return val.numpy()


@pytest.mark.parametrize("case", VC.value_cases(), ids=lambda c: c["id"])
def test_valuation_kernel_equals_the_host_form(gpu_solver, case):
    want = V.value_scenarios_host(case["bills"], case["bad"], case["ptr"], case["idx"], case["year"], case["fin"])
    VC.assert_case_is_what_it_says(want)
    got = device_value(gpu_solver, case)
    VC.assert_valuations_agree(got, want)
    again = device_value(gpu_solver, case)
    assert np.array_equal(got.values, again.values, equal_nan=True) and np.array_equal(got.valid, again.valid)


def test_valuation_kernel_shuffled_packing_order_gives_the_same_bits(gpu_solver):
    a = device_value(gpu_solver, VC.value_case(65, 21, n_opt=2, seed=5))
    b = device_value(gpu_solver, VC.value_case(65, 21, n_opt=2, seed=5, shuffle=True))
    assert np.array_equal(a.values, b.values, equal_nan=True) and np.array_equal(a.valid, b.valid)
    assert np.array_equal(a.proforma, b.proforma, equal_nan=True)
    assert a.valid[2] == 1 and a.valid[3] == 0 and a.valid.sum() == 64


def test_valuation_kernel_marks_a_scenario_whose_opt_year_has_no_window(gpu_solver):
    case = VC.value_case(65, 64, n_opt=3, per=1, seed=2)
    got = device_value(gpu_solver, case, proforma=False)
    assert got.valid[2] == 0 and got.valid[3] == 0 and got.valid.sum() == 63 and got.proforma is None
    assert np.isfinite(got.npv[2]) and np.isnan(got.npv[3])


@pytest.mark.parametrize("name", TV.NAMES)
def test_golden_arithmetic_on_the_device(gpu_solver, name):
    import torch
    b, p = TV.golden(name)
    bills = TV.one_window_bills(b["proforma"]["Avoided Energy Charge"][1], b["proforma"]["Avoided Demand Charge"][1])
    val = V.value_scenarios(gpu_solver, torch.as_tensor(bills).to(DEV), None, [0, 1], [0], [0],
                            TV.golden_financials(b), proforma=True)
    torch.cuda.synchronize()
    TV.check_against_golden(val.numpy(), b, p)


@pytest.mark.parametrize("name", TV.NAMES)
def test_end_to_end_on_the_solved_golden_windows(gpu_solver, name):
    """Solve the 12 golden windows on the GPU, bill and value them there."""
    import torch
    b, p = TV.golden(name)
    groups, wins, _ = TV.golden_groups(name)
    pb = builder.pack_groups(groups).to_torch(DEV).alloc_outputs()
    gpu_solver.solve_packed(pb)
    orig = [w["load"][None] for w in wins]
    dev = V.bill_windows(gpu_solver, pb, groups, orig=orig, peaks=True)
    fin = TV.golden_financials(b)
    val = V.value_scenarios(gpu_solver, dev.bills, dev.bad, [0, 12], np.arange(12), np.zeros(12, int), fin, proforma=True)
    torch.cuda.synchronize()
    assert not dev.bad.cpu().numpy().any() and (pb.istats[:, 0] == 0).all()
    rows, v = dev.bills.cpu().numpy(), val.numpy()
    # the device bill is the host form of the same x, bit for bit
    for k, (g, w) in enumerate(zip(groups, wins)):
        hb, hp, _ = V.bill_windows_host(V.bill_inputs(g, orig=w["load"][None]), pb.window(k)["x"][None])
        assert np.array_equal(rows[k], hb[0]) and np.array_equal(dev.peaks[k].cpu().numpy(), hp)
    ben = (rows[:, V.ORIG_RETAIL] - rows[:, V.RETAIL]) + (rows[:, V.ORIG_DEMAND] - rows[:, V.DEMAND])
    gold = (np.array(b["original_energy_charge"]) - b["energy_charge"]) + \
        (np.array(b["original_demand_charge"]) - b["demand_charge"])
    rel = np.abs(ben - gold) / np.abs(gold)
    print(f"{name}: max per-window benefit rel err {rel.max():.2e}, lifetime PV {v.npv[0]:.2f} vs golden "
          f"{b['npv']['Lifetime Present Value']:.2f}")
    assert rel.max() <= 1e-4, rel
    assert v.proforma[0, 1, 1] + v.proforma[0, 1, 2] == pytest.approx(
        b["proforma"]["Avoided Energy Charge"][1] + b["proforma"]["Avoided Demand Charge"][1], rel=1e-4)
    assert v.npv[0] == pytest.approx(b["npv"]["Lifetime Present Value"], rel=1e-4)
    assert v.valid[0] == 1
    # everything else: the host form fed the device bill
    VC.assert_valuations_agree(v, V.value_scenarios_host(rows, dev.bad.cpu().numpy(), [0, 12], np.arange(12),
                                                         np.zeros(12, int), fin))


def test_value_sweep_of_a_seeded_sweep_built_on_the_device(gpu_solver):
    import torch
    ids = np.arange(16)
    P = scenarios.sweep_parameters(ids)
    sw = SeededSweep(functools.partial(scenarios.config4, spec=True), ids, P["E"], stride=8,
                     features=scenarios.sweep_features(P))
    dev = sw.to_device(gpu_solver, DEV)
    sw.solve(gpu_solver, dev)
    fin = V.Financials(years=20, opt_years=(0,), rate=0.06, growth=[2.2, 2.2, 0.0, 0.0, 0.0],
                       capex=400.0 * P["E"], fixed_om=5.0 * P["E"] / 4.0, extra=np.full((1, 21), 100.0))
    val = V.value_sweep(sw, gpu_solver, dev, fin, proforma=True)
    torch.cuda.synchronize()
    assert val.values.is_cuda and list(val.scenarios) == list(ids)
    # the bill read the series the builder uploaded: the same tensors, nothing uploaded twice
    assert len(val.bills.series) == len(sw.specs) == len(dev.series)
    for used, built in zip(val.bills.series, dev.series):
        for name in ("base", "retail", "demand", "dcm_t", "dcm_j", "om"):
            assert used[name] is built[name] and used[name].data_ptr() == built[name].data_ptr(), name
    # the host form from dev.x copied back
    x, ist = dev.x.cpu().numpy(), dev.istats.cpu().numpy()
    assert (ist[:, 0] == 0).all()
    rows, k = [], 0
    for s in sw.specs:
        off = int(dev.desc[k, 6])
        hb, _, hbad = V.bill_windows_host(s, x[off:off + s.G * s.n].reshape(s.G, s.n), ist[k:k + s.G, 0])
        assert not hbad.any()
        rows.append(hb)
        k += s.G
    rows = np.concatenate(rows)
    assert np.array_equal(val.bills.bills.cpu().numpy(), rows)
    scen, ptr, idx, year = V.sweep_map(sw.tags, fin)
    assert sorted(idx.tolist()) == list(range(dev.count)) and (np.diff(ptr) == 12).all() and not year.any()
    assert [sw.tags[i] for i in idx[:12]] == [(0, w) for w in range(12)]
    want = V.value_scenarios_host(rows, np.zeros(len(rows), np.int32), ptr, idx, year, fin)
    got = val.numpy()
    VC.assert_valuations_agree(got, want)
    assert got.valid.all() and np.isfinite(got.npv).all()
    ms = V.last_ms(gpu_solver)
    assert ms["bill_ms"] > 0.0 and ms["valuation_ms"] > 0.0
