"""GPU: bills and valuation of EV windows (dvh_bill_windows with has_ev; dervet_hip/valuation.py): the device bill of a
solved, device-built batch is bit-identical to the host form, peaks included, and value_sweep values a config4_ev sweep
as the numpy valuation does."""
import functools

import numpy as np
import pytest

import ev_ref as ref
import valuation_cases as VC
from dervet_hip import valuation as V
from dervet_hip.lp import builder, gpu_builder, scenarios
from dervet_hip.sweep import SeededSweep

pytestmark = pytest.mark.gpu

BY_ID = dict(zip(ref.IDS, ref.SHAPES))


def _solved(gpu_solver, names, G=3):
    hosts, specs = [], []
    for name in names:
        T, J, pl, tg = BY_ID[name]
        load, retail, masks, dprice = ref.series(T, J, G)
        kw = dict(retail_price=retail, demand_masks=masks, demand_prices=dprice,
                  ev=dict(ch_max=ref.CH_MAX, ene_target=tg, fixed_om=3.0, plugged=pl))
        hosts.append(builder.battery_group(T, 1.0, load, ref.BAT, **kw))
        specs.append(gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, **kw))
    dev = gpu_builder.pack_specs_device(specs, gpu_solver)
    try:
        gpu_solver.set_kernel_path("load_shift")
        gpu_solver.solve_packed(dev)
    finally:
        gpu_solver.set_kernel_path("default")
    return hosts, specs, dev


def test_device_bill_is_bit_identical_to_the_host_form(gpu_solver):
    import torch
    hosts, specs, dev = _solved(gpu_solver, ["T5J1", "T65J4", "T129J1", "T744J4"])
    torch.cuda.synchronize()
    ist = dev.istats.cpu().numpy()
    assert (ist[:, 0] == 0).all(), ist[:, 0]
    x = dev.x.cpu().numpy()
    for groups in (specs, hosts):  # the series the builder uploaded, and a host group's uploaded by the bill
        b = V.bill_windows(gpu_solver, dev, groups, peaks=True)
        torch.cuda.synchronize()
        bills, bad = b.bills.cpu().numpy(), b.bad.cpu().numpy()
        k = 0
        for gi, g in enumerate(groups):
            off = int(dev.desc[k, 6])
            xs = x[off:off + g.G * g.n].reshape(g.G, g.n)
            hb, hp, hbad = V.bill_windows_host(g, xs, ist[k:k + g.G, 0])
            assert not hbad.any() and not bad[k:k + g.G].any()
            assert bills[k:k + g.G].tobytes() == hb.tobytes(), (gi, bills[k:k + g.G], hb)
            assert b.peaks[gi].cpu().numpy().tobytes() == hp.tobytes(), gi
            # the EV's charging is in the bill: the retail row is not the battery-only one
            plain = V.bill_windows_host(V.BillInputs(**{**V.bill_inputs(g).__dict__, "has_ev": False}), xs)[0]
            assert np.all(hb[:, V.RETAIL] > plain[:, V.RETAIL])
            k += g.G


def test_a_window_without_the_ev_block_is_a_bad_window(gpu_solver):
    """has_ev on a plain battery batch: n < 5T + J, so the dispatch rows are NaN and the window is flagged, not read."""
    import torch
    g = scenarios.config4(range(2), only=[1])[0]
    dev = builder.pack_groups([g]).to_torch("cuda:0").alloc_outputs()
    gpu_solver.solve_packed(dev)
    inp = V.BillInputs(**{**V.bill_inputs(g).__dict__, "has_ev": True})
    b = V.bill_windows(gpu_solver, dev, [inp])
    torch.cuda.synchronize()
    assert b.bad.cpu().tolist() == [V.BAD_WINDOW] * 2 and torch.isnan(b.bills[:, :V.ORIG_RETAIL]).all()


def test_value_sweep_of_a_config4_ev_sweep(gpu_solver):
    import torch
    ids = np.arange(2)
    P = scenarios.sweep_parameters(ids)
    sw = SeededSweep(functools.partial(scenarios.config4_ev, spec=True), ids, P["E"], stride=8,
                     features=scenarios.sweep_features(P))
    dev = sw.to_device(gpu_solver, "cuda:0")
    try:
        gpu_solver.set_kernel_path("load_shift")
        sw.solve(gpu_solver, dev)
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_kernel_path("default")
    fin = V.Financials(years=20, opt_years=(0,), rate=0.06, growth=[2.2, 2.2, 0.0, 0.0, 0.0],
                       capex=400.0 * P["E"], fixed_om=5.0 * P["E"] / 4.0)
    val = V.value_sweep(sw, gpu_solver, dev, fin, proforma=True)
    torch.cuda.synchronize()
    assert dev.count == 24 and all(s.ev is not None for s in sw.specs)
    assert ks["ell_windows"] == ks["generic_windows"] == 0, ks
    x, ist = dev.x.cpu().numpy(), dev.istats.cpu().numpy()
    assert (ist[:, 0] == 0).all(), ist[:, 0]
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
    want = V.value_scenarios_host(rows, np.zeros(len(rows), np.int32), ptr, idx, year, fin)
    got = val.numpy()
    VC.assert_valuations_agree(got, want)  # (rtol 1e-12)
    assert got.valid.all() and np.isfinite(got.npv).all()
