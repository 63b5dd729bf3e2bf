"""Reliability sizing LP: the program DER-VET's ``Reliability.size_for_outages`` solves
(dervet/MicrogridValueStreams/Reliability.py:221-274) for one ESS over a set of outage starts, in the canonical
form ``BatchSolver`` takes:  min c'x + c0,  K_E x = q_E,  K_I x >= q_I,  l <= x <= u.

For starts S = [t_0 .. t_{K-1}] and L = round(target_hours / dt) steps per outage:

  columns   x = [E, P], then per window w (in S order) ch[0..L-1], dis[0..L-1], s[0..L-1]  (s_k: energy after step k);
            n = 2 + 3 K L
  equality  (w, k), window-major:  s_k - s_{k-1} - rte dt ch_k + dt dis_k = 0,  s_{-1} = min(soc_init, ulsoc) E
  >= rows   per (w, k), in this order:  ulsoc E - s_k >= 0,  s_k - llsoc E >= 0,  P - ch_k >= 0,  P - dis_k >= 0,
            dis_k - ch_k >= d,   d = shed_k cl[i] - dg_gen - pv_vari[i],  i = t_w + k  (0 past the series end)
  objective ccost_kwh E + ccost_kw P + ccost   (every other cost is 0: get_capex, Reliability.py:235)

nnz = 14 K L, m = 6 K L.  Two deviations from the reference: its integer size variables (ESSSizing.py:83,98) are
relaxed and the optimum rounded up by the caller (``candidate``), and every window starts from
min(soc_init, ulsoc) E, the energy the post-facto simulation starts from (the reference's LP uses the ESS's
soc_target; both are 100 % in its golden cases), so that an LP-feasible size is a simulation-covered one.

csrc/dvh_sizing.hip expands the same values on the device (same formulas, same operation order; bit-identical,
tests/test_gpu_sizing.py).
"""
import math

import numpy as np

from ..solver import WindowLP


def outage_steps(case, spec):
    """L = round(target_hours / dt), the reference's coverage_dt (Reliability.py:120)."""
    return int(round(spec.target_hours / case.dt))


def terms(case, spec):
    """The scalars and series the LP is made of, validated (ValueError).  Shared by the host builder, the C-ABI
    structs (reliability._spec_struct) and the CPU restatement of the loop (tests/sizing_ref.py)."""
    from ..reliability import der_mix_properties
    e = case.ess
    L = outage_steps(case, spec)
    N = len(case.critical_load)
    if L < 1:
        raise ValueError("target_hours must cover at least one step")
    if L > int(case.max_outage_duration):
        raise ValueError("target outage steps exceed max_outage_duration (the simulation's data window)")
    if not (spec.size_energy or spec.size_power):
        raise ValueError("nothing to size: size_energy or size_power must be set")
    if spec.size_energy and not spec.ccost_kwh > 0:
        raise ValueError("sizing energy needs ccost_kwh > 0")
    if spec.size_power and not spec.ccost_kw > 0:
        raise ValueError("sizing power needs ccost_kw > 0")
    if not spec.size_power and float(e.get("P_ch", 0.0)) != float(e.get("P_dis", 0.0)):
        raise ValueError("a fixed power rating needs P_ch == P_dis (one power column)")
    if spec.n_seed < 1 or spec.max_rounds < 1:
        raise ValueError("n_seed and max_rounds must be >= 1")
    if case.load_shed_pct is not None and len(case.load_shed_pct) < L:
        raise ValueError("load_shed_pct shorter than the target outage")
    dg, _, _, pv_vari, _ = der_mix_properties(case)
    rte, llsoc, ulsoc = float(e.get("rte", 1.0)), float(e.get("llsoc", 0.0)), float(e.get("ulsoc", 1.0))
    inf = math.inf
    if spec.size_energy:
        lE, uE = float(spec.user_energy_min or 0.0), float(spec.user_energy_max or inf)
    else:
        lE = uE = float(e.get("E", 0.0))
    if spec.size_power:
        lP, uP = float(spec.user_power_min or 0.0), float(spec.user_power_max or inf)
    else:
        lP = uP = float(e.get("P_dis", 0.0))
    return dict(L=L, N=N, dt=float(case.dt), rte=rte, llsoc=llsoc, ulsoc=ulsoc, a0=min(float(case.soc_init), ulsoc),
                soc_init=float(case.soc_init), lE=lE, uE=uE, lP=lP, uP=uP, dg=float(dg),
                cl=np.ascontiguousarray(case.critical_load, np.float64),
                pv_vari=np.ascontiguousarray(pv_vari, np.float64) if case.pv_max else None,
                shed=None if case.load_shed_pct is None else np.ascontiguousarray(case.load_shed_pct, np.float64))


def seed_starts(case, spec):
    """The first n_seed indices of a stable descending sort of requirement_t = dt * sum_{j<L} cl[t + j] (summed in
    step order, truncated at the series end; Reliability.py:120-122,170-174).  Not shed-scaled."""
    L = outage_steps(case, spec)
    cl = np.ascontiguousarray(case.critical_load, np.float64)
    N = len(cl)
    req = np.zeros(N)
    for j in range(L):
        req[:N - j] = req[:N - j] + cl[j:]
    req = req * float(case.dt)
    return np.argsort(-req, kind="stable")[:spec.n_seed].astype(np.int32)


def candidate(x, lo, up=False):
    """The integer size tried for the LP optimum x: ceil(x - delta) (up: ceil(x + delta)), delta = 1e-7 max(1, |x|),
    floored at the quantity's lower bound."""
    d = 1e-7 * max(1.0, abs(x))
    return max(float(math.ceil(x + d if up else x - d)), float(lo))


def sizing_lp(case, spec, starts):
    """The sizing LP of ``case`` over the outage ``starts`` as a WindowLP."""
    t = terms(case, spec)
    L, N, dt = t["L"], t["N"], t["dt"]
    starts = np.asarray(starts, np.int64).ravel()
    K = len(starts)
    if K < 1 or (starts < 0).any() or (starts >= N).any():
        raise ValueError("starts must be a non-empty list of steps of the series")
    KL = K * L
    n, m_eq, m = 2 + 3 * KL, KL, 6 * KL
    w, k = np.divmod(np.arange(KL), L)
    base = 2 + 3 * w * L
    ch, dis, s = base + k, base + L + k, base + 2 * L + k
    indptr = np.concatenate([4 * np.arange(KL + 1), 4 * KL + 2 * np.arange(1, 5 * KL + 1)]).astype(np.int32)
    indices = np.zeros(14 * KL, np.int32)
    data = np.zeros(14 * KL)
    q = np.zeros(m)
    # equality rows: [E | ch_k, dis_k, s_k] for k = 0, [ch_k, dis_k, s_{k-1}, s_k] after
    first = k == 0
    e = 4 * np.arange(KL)
    indices[e] = np.where(first, 0, ch)
    indices[e + 1] = np.where(first, ch, dis)
    indices[e + 2] = np.where(first, dis, s - 1)
    indices[e + 3] = s
    data[e] = np.where(first, -t["a0"], -t["rte"] * dt)
    data[e + 1] = np.where(first, -t["rte"] * dt, dt)
    data[e + 2] = np.where(first, dt, -1.0)
    data[e + 3] = 1.0
    # >= rows, five per (w, k)
    g = 4 * KL + 10 * np.arange(KL)
    for i, (c0_, v0, c1_, v1) in enumerate(((0, t["ulsoc"], s, -1.0), (0, -t["llsoc"], s, 1.0), (1, 1.0, ch, -1.0),
                                            (1, 1.0, dis, -1.0), (ch, -1.0, dis, 1.0))):
        indices[g + 2 * i] = c0_
        data[g + 2 * i] = v0
        indices[g + 2 * i + 1] = c1_
        data[g + 2 * i + 1] = v1
    i = starts[w] + k
    inside = i < N
    ii = np.minimum(i, N - 1)
    cl = t["cl"][ii]
    if t["shed"] is not None:
        cl = cl * (t["shed"][k] / 100.0)
    d = cl - t["dg"]
    d = d - (t["pv_vari"][ii] if t["pv_vari"] is not None else 0.0)
    q[KL + 5 * np.arange(KL) + 4] = np.where(inside, d, 0.0)
    c = np.zeros(n)
    c[0], c[1] = float(spec.ccost_kwh), float(spec.ccost_kw)
    l = np.zeros(n)
    u = np.full(n, np.inf)
    l[0], u[0], l[1], u[1] = t["lE"], t["uE"], t["lP"], t["uP"]
    return WindowLP(indptr, indices, data, c, q, l, u, m_eq, float(spec.ccost),
                    meta={"kind": "reliability_sizing", "K": K, "L": L, "starts": starts.copy()})
