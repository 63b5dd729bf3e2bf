"""Post-facto reliability sweep on the GPU: the load coverage probability curve of DER-VET's Reliability value
stream (dervet/MicrogridValueStreams/Reliability.py:876-967 ``load_coverage_probability``), one outage simulated
from every start step of every case in one kernel launch (``dvh_outage_coverage``, csrc/dvh_outage.hip).

``der_mix_properties`` restates ``Reliability.get_der_mix_properties`` (:276-332) for plain DER descriptions
(storagevet's DER objects are not available here), and ``load_coverage_probability`` returns the reference's
DataFrame (index 'Outage Length (hrs)', column 'Load Coverage Probability (%)').  SOE at each outage start
follows the reference's choice (:896-905): the 'Aggregated State of Energy (kWh)' results column, the
'Aggregate Energy Min (kWh)' column for User-constraint-only runs, or soc_init x energy rating
(``init_soe=None``).  Bit-exact with the numpy reference (tests/test_gpu_outage.py); no CPU fallback.

``size_for_reliability`` is the sizing step of the same value stream (``Reliability.sizing_module`` :153-219): the
cutting-plane loop that sizes the ESS for an outage target, for a batch of cases in one library call
(``dvh_size_reliability``; the sizing LP of lp/sizing.py built on the device, the scan of every start as one launch of
the outage kernel).  ``first_uncovered`` and ``sizing_windows`` expose its two halves.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _lib


@dataclass
class OutageCase:
    critical_load: np.ndarray                 # [N] kW
    dt: float = 1.0                           # hours per step
    max_outage_duration: int = 24             # hours
    ess: dict = field(default_factory=dict)   # E (kWh), P_ch, P_dis (kW), rte (fraction), llsoc, ulsoc (fractions)
    init_soe: np.ndarray = None               # [N] energy at each outage start; None: soc_init x E
    soc_init: float = 1.0                     # post_facto_initial_soc (fraction)
    pv_max: list = field(default_factory=list)   # [N] arrays, one per PV (maximum generation)
    pv_nu: list = field(default_factory=list)    # nu (fraction) per PV
    pv_gamma: list = field(default_factory=list)  # gamma (fraction) per PV
    dg_power: list = field(default_factory=list)  # max power out (kW) per generator
    n_2: bool = False                         # N-2: drop the largest generator (dg_rating)
    dg_rating: float = 0.0
    load_shed_pct: np.ndarray = None          # [max_outage_duration] % of critical load kept per outage hour


@dataclass
class SizingSpec:
    """What ``size_for_reliability`` sizes for one OutageCase (Reliability.sizing_module's inputs).  The case's
    ``ess`` dict supplies rte, llsoc, ulsoc and the rating that is not sized; 0 = no user limit."""
    target_hours: float                       # Reliability 'target': outage length to ride through
    size_energy: bool = True
    size_power: bool = True
    ccost: float = 0.0                        # $ (constant)
    ccost_kw: float = 0.0                     # $/kW, > 0 when power is sized
    ccost_kwh: float = 0.0                    # $/kWh, > 0 when energy is sized
    user_energy_min: float = 0.0
    user_energy_max: float = 0.0
    user_power_min: float = 0.0
    user_power_max: float = 0.0
    n_seed: int = 10                          # outage starts of the first round (top_n_outages)
    max_rounds: int = 256


def der_mix_properties(case):
    """(dg_gen, pv_max, props, pv_vari, largest_gamma) as Reliability.get_der_mix_properties (:276-332)."""
    N = len(case.critical_load)
    pv_max = np.zeros(N)
    pv_vari = np.zeros(N)
    gamma = 0.0
    for g, nu, ga in zip(case.pv_max, case.pv_nu, case.pv_gamma):
        g = np.asarray(g, np.float64)
        pv_max += g
        pv_vari += g * nu
        gamma = max(gamma, ga)
    dg = float(sum(case.dg_power))
    if case.n_2:
        dg -= case.dg_rating
    e = case.ess
    props = {"charge max": float(e.get("P_ch", 0.0)), "discharge max": float(e.get("P_dis", 0.0)),
             "operation SOE min": e.get("llsoc", 0.0) * float(e.get("E", 0.0)),
             "operation SOE max": e.get("ulsoc", 1.0) * float(e.get("E", 0.0)),
             "rte": float(e.get("rte", 1.0)), "energy rating": float(e.get("E", 0.0)),
             "pv present": bool(case.pv_max)}
    return dg, pv_max, props, pv_vari, gamma


def _cases_struct(cases):
    arr = (_lib.OutageCase * len(cases))()
    keep, sizes = [], []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float64)
        keep.append(a)
        return a.ctypes.data_as(_lib.c_double_p)

    for k, c in enumerate(cases):
        dg, pv_max, props, pv_vari, gamma = der_mix_properties(c)
        N = len(c.critical_load)
        o = arr[k]
        o.n_steps, o.max_outage, o.dt = N, int(c.max_outage_duration), float(c.dt)
        o.critical_load = ptr(c.critical_load)
        o.pv_max = ptr(pv_max) if c.pv_max else None
        o.pv_vari = ptr(pv_vari) if c.pv_max else None
        o.init_soe = ptr(c.init_soe)
        o.load_shed_pct = ptr(c.load_shed_pct)
        o.soe0 = c.soc_init * props["energy rating"]
        o.dg_gen, o.gamma = dg, gamma
        o.soe_min, o.soe_max = props["operation SOE min"], props["operation SOE max"]
        o.charge_max, o.discharge_max, o.rte = props["charge max"], props["discharge max"], props["rte"]
        sizes.append((N, int(c.max_outage_duration / c.dt)))
    return arr, keep, sizes


def outage_coverage(cases, solver):
    """Covered length per start (list of int32 arrays) and the LCP curve per case (list of float arrays)."""
    lib = solver._lib
    arr, keep, sizes = _cases_struct(cases)
    lengths = np.zeros(sum(n for n, _ in sizes), np.int32)
    lcp = np.zeros(sum(L for _, L in sizes), np.float64)
    solver._check(lib.dvh_outage_coverage(solver._h, arr, len(cases), lengths.ctypes.data_as(_lib.c_int32_p),
                                          lcp.ctypes.data_as(_lib.c_double_p)), "dvh_outage_coverage")
    out_l, out_c, a, b = [], [], 0, 0
    for N, L in sizes:
        out_l.append(lengths[a:a + N])
        out_c.append(lcp[b:b + L])
        a += N
        b += L
    return out_l, out_c


def min_soe(cases, target_hours, solver):
    """Reliability.min_soe_iterative (:685-756) per case: [N] minimum SOE (kWh) the ESS must hold at each step
    to ride through a target_hours outage from soc_init x energy rating (the 'Reliability Min State of Energy
    (kWh)' requirement applied to every window as an ene lower bound, :334-354)."""
    lib = solver._lib
    arr, keep, sizes = _cases_struct(cases)
    tgt = np.ascontiguousarray(np.broadcast_to(np.asarray(target_hours, np.int32), (len(cases),)))
    out = np.zeros(sum(n for n, _ in sizes), np.float64)
    solver._check(lib.dvh_outage_min_soe(solver._h, arr, len(cases), tgt.ctypes.data_as(_lib.c_int32_p),
                                         out.ctypes.data_as(_lib.c_double_p)), "dvh_outage_min_soe")
    res, a = [], 0
    for N, _ in sizes:
        res.append(out[a:a + N])
        a += N
    return res


def first_uncovered(cases, target_hours, solver):
    """The sizing loop's scan (Reliability.find_first_uncovered, :391-445) for every case at once: an outage of
    round(target_hours / dt) steps simulated from every start from soc_init x energy rating (``init_soe`` ignored);
    a start is uncovered when fewer steps are covered than the target and than the series has left.  Returns
    (first, n_uncovered): int32 arrays, first = the smallest uncovered start or -1.  Bit-exact with the oracle."""
    lib = solver._lib
    arr, keep, _ = _cases_struct(cases)
    hours = np.broadcast_to(np.asarray(target_hours, np.float64), (len(cases),))
    steps = np.array([int(round(h / c.dt)) for h, c in zip(hours, cases)], np.int32)
    first = np.zeros(len(cases), np.int32)
    count = np.zeros(len(cases), np.int32)
    solver._check(lib.dvh_outage_first_uncovered(solver._h, arr, len(cases), steps.ctypes.data_as(_lib.c_int32_p),
                                                 first.ctypes.data_as(_lib.c_int32_p),
                                                 count.ctypes.data_as(_lib.c_int32_p)), "dvh_outage_first_uncovered")
    return first, count


def _spec_struct(cases, specs):
    """dvh_sizing_spec per case (validated by lp.sizing.terms: ValueError)."""
    from .lp import sizing
    if len(cases) != len(specs):
        raise ValueError("one SizingSpec per OutageCase")
    arr = (_lib.SizingSpec * len(cases))()
    for k, (c, sp) in enumerate(zip(cases, specs)):
        t = sizing.terms(c, sp)
        o = arr[k]
        o.target_hours = float(sp.target_hours)
        o.size_energy, o.size_power = int(bool(sp.size_energy)), int(bool(sp.size_power))
        o.ccost, o.ccost_kw, o.ccost_kwh = float(sp.ccost), float(sp.ccost_kw), float(sp.ccost_kwh)
        o.energy_min, o.energy_max, o.power_min, o.power_max = t["lE"], t["uE"], t["lP"], t["uP"]
        o.energy, o.power = t["lE"], t["lP"]  # (the fixed rating when the quantity is not sized)
        o.llsoc, o.ulsoc, o.soc_init = t["llsoc"], t["ulsoc"], t["soc_init"]
        o.n_seed, o.max_rounds = int(sp.n_seed), int(sp.max_rounds)
    return arr


def sizing_windows(cases, specs, starts, solver):
    """The sizing LP of every case over the given outage starts (``starts[k]``: steps of case k's series), built on
    the device from the resident series and solved as one batch with the solver's options (dvh_sizing_windows).
    Returns a WindowResult per case; bit-identical to ``solver.solve([lp.sizing.sizing_lp(c, s, st) ...])``."""
    from .lp import sizing
    from .solver import WindowResult
    lib = solver._lib
    arr, keep, _ = _cases_struct(cases)
    sarr = _spec_struct(cases, specs)
    if len(starts) != len(cases):
        raise ValueError("one list of starts per case")
    ns = np.array([len(s) for s in starts], np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32).ravel() for s in starts]), np.int32)
    res = (_lib.Result * len(cases))()
    outs = []
    for k, (c, sp) in enumerate(zip(cases, specs)):
        KL = int(ns[k]) * sizing.outage_steps(c, sp)
        x, y = np.zeros(2 + 3 * KL), np.zeros(6 * KL)
        outs.append((x, y))
        res[k].x = x.ctypes.data_as(_lib.c_double_p)
        res[k].y = y.ctypes.data_as(_lib.c_double_p)
    solver._check(lib.dvh_sizing_windows(solver._h, arr, sarr, len(cases), flat.ctypes.data_as(_lib.c_int32_p),
                                         ns.ctypes.data_as(_lib.c_int32_p), res), "dvh_sizing_windows")
    return [WindowResult(outs[k][0], outs[k][1], res[k].obj, res[k].status, res[k].iters, res[k].primal_res_rel,
                         res[k].dual_res_rel, res[k].gap_rel) for k in range(len(cases))]


@dataclass
class SizingResult:
    energy: float                             # kWh
    power: float                              # kW (charge = discharge rating)
    status: str                               # SIZED, ROUND_LIMIT (the last candidate), STALLED, LP_FAILED
    rounds: int                               # LPs solved
    capex: float                              # ccost + ccost_kw power + ccost_kwh energy
    starts: np.ndarray                        # outage starts of the last LP
    lp_status: int                            # dvh_result.status of the last LP (LP_FAILED: why)
    lp_iters: int                             # PDHG iterations summed over the rounds
    min_soe: np.ndarray = None                # with_min_soe: the sized case's 'Reliability Min State of Energy (kWh)'


def sized_case(case, result):
    """``case`` with the ratings of ``result`` (charge = discharge rating), starting every outage from soc_init."""
    import dataclasses
    ess = dict(case.ess, E=result.energy, P_ch=result.power, P_dis=result.power)
    return dataclasses.replace(case, ess=ess, init_soe=None)


def size_for_reliability(cases, specs, solver, with_min_soe=False):
    """Reliability.sizing_module (:153-219) for every case at once: the integer ESS energy and / or power rating that
    rides through a ``target_hours`` outage from every start of the series, found by the reference's cutting-plane
    loop in one library call (dvh_size_reliability) with the series resident on the GPU.  Returns a SizingResult per
    case; with_min_soe adds the sized case's minimum-SOE series (one ``min_soe`` call, as the reference at :209-214;
    needs whole target hours)."""
    lib = solver._lib
    arr, keep, _ = _cases_struct(cases)
    sarr = _spec_struct(cases, specs)
    res = (_lib.SizingResult * len(cases))()
    bufs = []
    for k, sp in enumerate(specs):
        b = np.zeros(int(sp.n_seed) + int(sp.max_rounds), np.int32)
        bufs.append(b)
        res[k].starts = b.ctypes.data_as(_lib.c_int32_p)
    solver._check(lib.dvh_size_reliability(solver._h, arr, sarr, len(cases), res), "dvh_size_reliability")
    out = [SizingResult(res[k].energy, res[k].power, _lib.SIZING_STATUS_NAMES[res[k].status], res[k].rounds,
                        res[k].capex, bufs[k][:res[k].n_starts].copy(), res[k].lp_status, res[k].lp_iters)
           for k in range(len(cases))]
    if with_min_soe:
        idx = [k for k, r in enumerate(out) if r.energy > 0]
        hours = [specs[k].target_hours for k in idx]
        if any(h != int(h) for h in hours):
            raise ValueError("with_min_soe needs whole target hours (Reliability.outage_duration is an int)")
        if idx:
            ms = min_soe([sized_case(cases[k], out[k]) for k in idx], [int(h) for h in hours], solver)
            for k, v in zip(idx, ms):
                out[k].min_soe = v
    return out


def last_sizing_ms(solver):
    """HIP-event time of the last size_for_reliability call: total, LP builds + solves, scans (ms), and rounds summed
    over the cases."""
    ms = ctypes.c_double()
    o3 = (ctypes.c_double * 3)()
    solver._check(solver._lib.dvh_last_sizing_ms(solver._h, ctypes.byref(ms), o3), "dvh_last_sizing_ms")
    return {"total_ms": ms.value, "lp_ms": o3[0], "scan_ms": o3[1], "rounds": int(o3[2])}


def load_coverage_probability(cases, solver):
    """The reference's DataFrames (Reliability.py:959-967), one per case."""
    import pandas as pd
    _, curves = outage_coverage(cases, solver)
    out = []
    for c, v in zip(cases, curves):
        length = np.arange(c.dt, c.max_outage_duration + c.dt, c.dt)[:len(v)]
        df = pd.DataFrame({"Outage Length (hrs)": length, "Load Coverage Probability (%)": v})
        out.append(df.set_index("Outage Length (hrs)"))
    return out


def last_kernel_ms(solver):
    ms = ctypes.c_double()
    solver._check(solver._lib.dvh_last_outage_ms(solver._h, ctypes.byref(ms)), "dvh_last_outage_ms")
    return ms.value
