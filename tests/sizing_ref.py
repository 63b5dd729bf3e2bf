"""TEST INFRASTRUCTURE: DER-VET's reliability sizing loop (Reliability.sizing_module,
dervet/MicrogridValueStreams/Reliability.py:153-219) restated on the CPU -- scipy's HiGHS on
dervet_hip.lp.sizing.sizing_lp, the library's rounding and stall rule, oracle.outage.simulate_outage for the scan.
The GPU loop (dervet_hip.reliability.size_for_reliability) must agree with it integer for integer."""
import json
import os
from dataclasses import dataclass, field, replace
from functools import lru_cache

import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

import outage_cases
from dervet_hip import reliability
from dervet_hip.lp import sizing
from oracle import outage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reliability_sizing.json")


def solve_highs(lp):
    """HiGHS optimum of a WindowLP: (x, status) with status 0 = optimal."""
    K = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))
    me = lp.m_eq
    bounds = [(lo, None if np.isinf(hi) else hi) for lo, hi in zip(lp.l, lp.u)]
    r = linprog(lp.c, A_ub=-K[me:], b_ub=-lp.q[me:], A_eq=K[:me], b_eq=lp.q[:me], bounds=bounds, method="highs")
    return r.x, r.status


def scan(case, E, P, L, stop_at_first=False):
    """scan_case of the case sized (E, P)."""
    return scan_case(replace(case, ess=dict(case.ess, E=E, P_ch=P, P_dis=P)), L, stop_at_first)


def scan_case(case, L, stop_at_first=False):
    """(first uncovered start or -1, number of uncovered starts) of the case's ESS: an outage of L steps simulated
    from every start from soc_init x E; a start is uncovered when covered < L and covered < N - t
    (Reliability.py:431-435)."""
    dg, pmax, props, pvar, gamma = reliability.der_mix_properties(case)
    cl = np.asarray(case.critical_load, np.float64)
    N = len(cl)
    gen = np.repeat(dg, N)
    soe0 = case.soc_init * props["energy rating"]
    first, count = -1, 0
    for t in range(N):
        k, _ = outage.simulate_outage(t, cl, gen, pmax, pvar, gamma, props, soe0, L, int(case.max_outage_duration),
                                      case.dt, case.load_shed_pct)
        if k < L and k < N - t:
            count += 1
            if first < 0:
                first = t
                if stop_at_first:
                    break
    return first, count


@dataclass
class RefSizing:
    energy: float
    power: float
    status: str
    rounds: int
    starts: list
    lp_x: list = field(default_factory=list)  # HiGHS's (E, P) of every round


def size_for_reliability(case, spec):
    t = sizing.terms(case, spec)
    L = t["L"]
    S = [int(v) for v in sizing.seed_starts(case, spec)]
    lp_x = []
    E = P = 0.0
    for rnd in range(1, spec.max_rounds + 1):
        x, st = solve_highs(sizing.sizing_lp(case, spec, S))
        if st != 0:
            return RefSizing(E, P, "LP_FAILED", rnd, S, lp_x)
        lp_x.append((float(x[0]), float(x[1])))
        for up in (False, True):
            E = sizing.candidate(x[0], t["lE"], up) if spec.size_energy else t["lE"]
            P = sizing.candidate(x[1], t["lP"], up) if spec.size_power else t["lP"]
            first, _ = scan(case, E, P, L, stop_at_first=True)
            if first < 0:
                return RefSizing(E, P, "SIZED", rnd, S, lp_x)
            if first not in S:
                break
        else:
            return RefSizing(E, P, "STALLED", rnd, S, lp_x)
        if rnd < spec.max_rounds:
            S.append(first)
    return RefSizing(E, P, "ROUND_LIMIT", spec.max_rounds, S, lp_x)


def near_integer(ref, spec, tol=1e-3):
    """A round whose HiGHS optimum of a sized quantity lies within tol above an integer: the GPU loop's LP optimum,
    a few 1e-7 away, could legitimately round to the other side."""
    for xe, xp in ref.lp_x:
        for x, sized in ((xe, spec.size_energy), (xp, spec.size_power)):
            if sized and x - np.floor(x) <= tol:
                return True
    return False


def golden_cases():
    """{name: (OutageCase, SizingSpec, golden dict)} of the reference's load-shedding sizing runs."""
    with open(GOLDEN) as f:
        g = json.load(f)
    series = outage_cases.load()
    out = {}
    for name, m in g["cases"].items():
        c = series[m["series"]]
        case = reliability.OutageCase(critical_load=c["critical_load"], dt=c["dt"],
                                      max_outage_duration=c["max_outage_duration"],
                                      ess=dict(rte=m["rte"], llsoc=m["llsoc"], ulsoc=m["ulsoc"]),
                                      soc_init=c["soc_init"],
                                      load_shed_pct=c["load_shed_pct"])
        spec = reliability.SizingSpec(target_hours=m["target_hours"], ccost=m["ccost"], ccost_kw=m["ccost_kw"],
                                      ccost_kwh=m["ccost_kwh"])
        out[name] = (case, spec, m)
    return out


def random_family(seed, count=8):
    """Mixed cases for the GPU-vs-CPU loop comparison (PV with nu < 1, generator, shedding, llsoc / ulsoc,
    soc_init < 1, dt 0.5; the sized quantities rotate over both / energy only / power only)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        N = int(rng.integers(500, 701))
        dt = (1.0, 1.0, 0.5)[i % 3]
        L = int(rng.integers(3, 7))
        cl = rng.uniform(200.0, 1500.0, N).round(5)
        pv = i % 2 == 1
        pvs = [np.maximum(0.0, rng.normal(300, 300, N))] if pv else []
        nu, gamma = float(rng.uniform(0.2, 1.0)), float(rng.uniform(0.3, 1.0))
        dg = [float(rng.uniform(0, 300))] if i % 4 >= 2 else []
        shed = rng.choice([100.0, 80.0, 50.0], size=24) if i % 3 == 2 else None
        ess = dict(rte=float(rng.uniform(0.8, 0.95)), llsoc=float(rng.uniform(0, 0.2)),
                   ulsoc=float(rng.uniform(0.85, 1.0)))
        mode = (i + i // 3) % 3  # 0 both, 1 energy only, 2 power only
        if mode == 1:
            ess["P_ch"] = ess["P_dis"] = 2000.0
        if mode == 2:
            ess["E"] = 30000.0
        case = reliability.OutageCase(critical_load=cl, dt=dt, max_outage_duration=24, ess=ess,
                                      soc_init=float(rng.uniform(0.6, 1.0)), pv_max=pvs, pv_nu=[nu] if pv else [],
                                      pv_gamma=[gamma] if pv else [], dg_power=dg, load_shed_pct=shed)
        spec = reliability.SizingSpec(target_hours=L * dt, size_energy=mode != 2, size_power=mode != 1,
                                      ccost_kw=100.0, ccost_kwh=800.0)
        out.append((case, spec))
    return out


FAMILY_SEEDS = (11, 12)  # the committed seeds of random_family (tests/test_sizing_lp.py checks that they qualify)


@lru_cache(maxsize=None)
def golden_reference(name, max_rounds=256):
    """The CPU loop's result on a golden case (computed once per session)."""
    case, spec, _ = golden_cases()[name]
    return size_for_reliability(case, replace(spec, max_rounds=max_rounds))


@lru_cache(maxsize=None)
def family_reference(seed):
    """The CPU loop's results on random_family(seed) (computed once per session)."""
    return tuple(size_for_reliability(c, s) for c, s in random_family(seed))
