"""Seeded cases of the economic-sizing tests (tests/test_value_sizing_*.py, tests/test_gpu_value_*.py): sites with a
daily load shape, a time-of-use energy price and one demand charge per window, as device-builder specs with one row
per case and one spec per window position.  Plain module, fixed seeds."""
import json
import os

import numpy as np

from dervet_hip import ValueSizingSpec, annuity_scalar
from dervet_hip.lp import gpu_builder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

DT = 1.0
ALPHA = annuity_scalar(2017, 2037, [2017], 0.022, 0.06)   # the Usecase 1 horizon: 14.454006150790663
CCOST_KWH, CCOST_KW, FIXED_OM = 250.0, 800.0, 10.0        # the Usecase 1 battery's costs


def battery(N, llsoc=0.1, ulsoc=0.95, soc_target=0.5, sdr=0.0, rte=0.91):
    # (the ratings are the loop's; fixedOM enters through the spec's unit cost, so the windows carry none)
    return dict(E=np.ones(N), Pch=np.ones(N), Pdis=np.ones(N), rte=rte, sdr=sdr, soc_target=soc_target, ulsoc=ulsoc,
                llsoc=llsoc, OMexpenses=0.0, fixedOM=0.0)


def positions(seeds, W, T, J=1, emax_frac=None, **bat):
    """W window positions of T steps for len(seeds) cases: [BatteryGroupSpec] with G = len(seeds)."""
    N, J = len(seeds), min(J, T)   # (a period needs a step)
    rngs = [np.random.default_rng(int(s)) for s in seeds]
    out = []
    for w in range(W):
        h = (w * T + np.arange(T)) % 24
        load = np.stack([(600.0 + 100.0 * k) + 400.0 * np.sin(2 * np.pi * (h - 15) / 24.0) + 60.0 * r.standard_normal(T)
                         for k, r in enumerate(rngs)])
        price = np.stack([0.05 + 0.10 * ((h >= 16) & (h < 21)) + 0.01 * r.random(T) for r in rngs])
        # J > 1: period 0 covers every step, period j the steps t = j mod J (so a step meets two demand-charge rows)
        masks = None if J == 0 else np.stack([(np.arange(T) % J == j) | (j == 0) for j in range(J)])
        demand = None if J == 0 else np.stack([12.0 + 6.0 * r.random(J) for r in rngs])
        emax = None
        if emax_frac is not None:   # an aggregate SOE ceiling that bites on the afternoon steps
            emax = np.where((h >= 12) & (h < 18), emax_frac, np.inf)[None, :].repeat(N, 0)
        out.append(gpu_builder.battery_group_spec(T, DT, load, battery(N, **bat), retail_price=price,
                                                  demand_masks=masks, demand_prices=demand, ene_max=emax))
    return out


def spec(scale, candidates, energy_max=12000.0, power_max=2000.0, gap_tol=1e-6, **kw):
    """The Usecase 1 battery's costs times ``scale`` (0.1 and 0.03: interior optima on these windows, or the edge
    E = energy_max when the box is tight; 1: the corner E = P = 0)."""
    return ValueSizingSpec(ccost=0.0, ccost_kw=CCOST_KW * scale, ccost_kwh=CCOST_KWH * scale, fixed_om=FIXED_OM * scale,
                           alpha=ALPHA, energy_max=energy_max, power_max=power_max, gap_tol=gap_tol,
                           candidates=candidates, max_rounds=60, **kw)


SEEDS = [11, 12, 13, 14]
SCALES = [0.1, 0.03, 1.0, 0.1]


def small_cases(candidates):
    """4 seeded cases x 3 windows of 48 steps (llsoc 0.1, ulsoc 0.95, soc_target 0.5) and their specs."""
    specs = [spec(s, candidates) for s in SCALES]
    specs[3] = spec(SCALES[3], candidates, energy_max=4000.0)   # (a box edge: E = energy_max, P interior)
    return positions(SEEDS, 3, 48), specs


def long_case(candidates):
    """One case of a single 800-step window (the chain tier; z in the cut pass's workspace)."""
    return positions([21], 1, 800), [spec(0.1, candidates)]


def uc1(name="es", candidates=4, monthly=False, scales=None):
    """The reference's Usecase 1 sizing case (tests/golden/uc1_sizing.*: ene / ch / dis ratings 0, n = year) as
    (positions, specs, meta): one year window as the reference demands, or the twelve months (monthly); the tariff's
    energy price and one demand-charge column per (billing period, month); es+pv: the fixed 1000 kW PV's generation
    taken off the load.  scales: seeded load scales, one case each (default: the golden load alone).  The box is the
    series' own 'Energy Max' ceiling of 32,000 kWh and a power no window could use (the largest load)."""
    from oracle import tariff as OT
    with open(os.path.join(GOLDEN, "uc1_sizing.json")) as f:
        meta = json.load(f)[name]
    arr = np.load(os.path.join(GOLDEN, "uc1_sizing.npz"))
    p = meta["params"]
    load = arr[f"{name}__site_load"]
    if "PV" in p:
        load = load - float(p["PV"]["rated_capacity"]) * np.nan_to_num(arr[f"{name}__pv_profile"])
    T_all, dt = len(load), float(p["Scenario"]["dt"])
    month, he, wd = OT.step_calendar(int(p["Scenario"]["opt_years"]), T_all, dt)
    price = OT.energy_price(meta["tariff"], month, he, wd)
    dem = OT.demand_periods(meta["tariff"], month, he, wd)
    b, fin, sc = p["Battery"], p["Finance"], p["Scenario"]
    scales = np.ones(1) if scales is None else np.asarray(scales, np.float64)
    N = len(scales)
    bat = dict(E=np.ones(N), Pch=np.ones(N), Pdis=np.ones(N), rte=float(b["rte"]) / 100, sdr=float(b["sdr"]),
               soc_target=float(b["soc_target"]) / 100, ulsoc=float(b["ulsoc"]) / 100, llsoc=float(b["llsoc"]) / 100,
               OMexpenses=float(b["OMexpenses"]), fixedOM=0.0)
    positions = []
    for sel in ([np.nonzero(month == mo)[0] for mo in range(1, 13)] if monthly else [np.arange(T_all)]):
        masks, prices = [], []
        for _, d, mask in dem:
            for mo in np.unique(month[sel]):
                mm = mask[sel] & (month[sel] == mo)
                if mm.any():
                    masks.append(mm)
                    prices.append(d)
        positions.append(gpu_builder.battery_group_spec(
            len(sel), dt, scales[:, None] * load[sel][None, :], bat, retail_price=np.tile(price[sel], (N, 1)),
            demand_masks=np.array(masks), demand_prices=np.tile(np.array(prices), (N, 1))))
    alpha = annuity_scalar(int(sc["start_year"]), int(sc["end_year"]), [int(sc["opt_years"])],
                           float(fin["inflation_rate"]) / 100, float(fin["npv_discount_rate"]) / 100)
    specs = [ValueSizingSpec(ccost=float(b["ccost"]), ccost_kw=float(b["ccost_kw"]), ccost_kwh=float(b["ccost_kwh"]),
                             fixed_om=float(b["fixedOM"]), alpha=alpha, energy_max=32000.0, power_max=float(np.ceil(load.max() * s)),
                             candidates=candidates, max_rounds=60) for s in scales]
    return positions, specs, meta
