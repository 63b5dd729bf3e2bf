"""Economic sizing: the ESS energy and power rating that minimise lifetime cost (ESSSizing.py:82-110,
ContinuousSizing.sizing_objective, MicrogridScenario.py:208-217, 293-295, CBA.py:190-213 of the reference; the method
and its deviations: DESIGN.md section 4b, include/dervet_hip.h "Economic sizing").

    F(E, P) = ccost_kwh E + (ccost_kw + alpha fixed_om) P + ccost + alpha sum_w V_w(E, P)

with V_w the optimum of the case's battery window at window position w.  ``size_for_value`` runs Kelley's cutting
planes with the windows solved, cut and the masters solved on the GPU; ``host_cuts`` is the numpy form of the cut
arithmetic (csrc/dvh_value_cut.h, operation for operation), and ``master_host`` / ``loop_host`` restate the master
step, so that a CPU solver's duals can drive the same loop (tests/value_sizing_ref.py).
"""
import ctypes
import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .lp import sizing as _sizing

CUT_COLS = _lib.VALUE_CUT_COLS
A, GE, GP, DOBJ, POBJ, RINF, FLAG, STATUS, ITERS = range(9)
SIZED, ROUND_LIMIT, LP_FAILED, MASTER_FAILED = 0, 1, 2, 3
LANES, WAVE = 256, 64


@dataclass
class ValueSizingSpec:
    """What is sized for one case.  A sized quantity needs a finite box and a positive unit cost; a rating that is not
    sized is ``energy`` / ``power``.  ``fixed_om`` ($/kW-yr) enters the power's unit cost times alpha, so the window
    specs must be built with fixedOM = 0 (their c0 would otherwise hold it at a fixed rating)."""
    size_energy: bool = True
    size_power: bool = True
    ccost: float = 0.0
    ccost_kw: float = 0.0
    ccost_kwh: float = 0.0
    fixed_om: float = 0.0
    alpha: float = 1.0
    energy_min: float = 0.0
    energy_max: float = math.inf
    power_min: float = 0.0
    power_max: float = math.inf
    energy: float = 0.0
    power: float = 0.0
    gap_tol: float = 1e-6
    candidates: int = 4
    max_rounds: int = 40

    @property
    def c_energy(self):
        return float(self.ccost_kwh)

    @property
    def c_power(self):
        return float(self.ccost_kw) + float(self.alpha) * float(self.fixed_om)

    def box(self):
        e = (self.energy_min, self.energy_max) if self.size_energy else (self.energy, self.energy)
        p = (self.power_min, self.power_max) if self.size_power else (self.power, self.power)
        return float(e[0]), float(e[1]), float(p[0]), float(p[1])

    def capex(self, E, P):
        return self.ccost + self.ccost_kw * P + self.ccost_kwh * E

    def as_struct(self):
        s = _lib.ValueSpec()
        s.size_energy, s.size_power = int(bool(self.size_energy)), int(bool(self.size_power))
        s.c_energy, s.c_power, s.c_fixed, s.alpha = self.c_energy, self.c_power, float(self.ccost), float(self.alpha)
        s.energy_min, s.energy_max, s.power_min, s.power_max = self.box()
        s.gap_tol, s.max_rounds = float(self.gap_tol), int(self.max_rounds)
        return s


@dataclass
class ValueSizingResult:
    energy: float = math.nan      # rounded up (lp.sizing.candidate)
    power: float = math.nan
    energy_lp: float = math.nan   # the relaxed optimum: the loop's incumbent
    power_lp: float = math.nan
    lower: float = -math.inf
    upper: float = math.inf
    objective: float = math.nan   # F at the rounded size, from the final solve
    terms: dict = field(default_factory=dict)
    capex: float = math.nan
    rounds: int = 0
    n_cuts: int = 0
    lp_iters: int = 0
    status: int = -1
    lp_status: int = 0
    dispatch: object = None       # per window position: x of the final solve (on request)

    @property
    def status_name(self):
        return _lib.VALUE_STATUS_NAMES.get(self.status, "?")


def annuity_scalar(start_year, end_year, opt_years, inflation, discount):
    """CBA.annuity_scalar (CBA.py:190-213): n = end - start yearly dollars, 1 in the first opt year and inflated /
    deflated from there, discounted from k = 0 (``[0] + ndarray`` there adds elementwise, so np.npv's first term is the
    first year's, undiscounted).  Rates are fractions."""
    n = int(end_year) - int(start_year)
    d = np.ones(n)
    i0 = int(min(opt_years)) - int(start_year)
    i = i0
    while i < n - 1:
        d[i + 1] = d[i] * (1 + inflation)
        i += 1
    i = i0
    while i > 0:
        d[i - 1] = d[i] * (1 / (1 + inflation))
        i -= 1
    return float((d / (1 + discount) ** np.arange(n)).sum())


def round0_points(spec, C):
    """The fixed points of the box a case's first round evaluates, max(C, 2) of them: the two corners, then
    (E_lo + (E_hi - E_lo) / 2^(j - 1), P_lo + (P_hi - P_lo) / 2), j = 2, 3, .."""
    elo, ehi, plo, phi = spec.box()
    pts = [(elo, plo), (ehi, phi)]
    for j in range(2, max(C, 2)):
        pts.append((elo + (ehi - elo) / 2.0 ** (j - 1), plo + (phi - plo) / 2.0))
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# the cut arithmetic on the host (csrc/dvh_value_cut.h in numpy, the same operations in the same order)

def _tree(part):
    """A 256-lane workgroup's sum of its lanes' partials: each wave halves its 64, the waves are added in order."""
    v = np.array(part, np.float64).reshape(LANES // WAVE, WAVE)
    o = WAVE // 2
    while o > 0:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    tot = v[0, 0]
    for w in range(1, LANES // WAVE):
        tot = tot + v[w, 0]
    return tot


def _lane_sum(terms):
    """Lane l's running sum of terms l, l + 256, .. (terms [n] or [n, k]: k terms per step added in column order)."""
    t = np.asarray(terms, np.float64)
    if t.ndim == 1:
        t = t[:, None]
    n, k = t.shape
    rows = -(-n // LANES) if n else 0
    pad = np.zeros((rows * LANES, k))
    pad[:n] = t
    acc = np.zeros(LANES)
    for r in range(rows):
        for c in range(k):
            acc = acc + pad[r * LANES:(r + 1) * LANES, c]
    return acc


def host_cut(T, J, dcm_t, dcm_j, dv, c, l, u, q, x, y, c0, E, P, soc_target, llsoc, ulsoc, emax=None):
    """One window's cut record [CUT_COLS] from its LP vectors (the packed batch's, window-local) and returned x, y."""
    dcm_t, dcm_j = np.asarray(dcm_t, np.int64), np.asarray(dcm_j, np.int64)
    mI = len(dcm_t)
    yy = np.array(y, np.float64)
    yy[T + 1:] = np.where(yy[T + 1:] < 0.0, 0.0, yy[T + 1:])
    z = np.zeros(T)
    tausum = np.zeros(J)
    for j in range(J):
        sel = dcm_j == j
        yi = np.where(sel, yy[T + 1:T + 1 + mI], 0.0)
        z[dcm_t[sel]] = z[dcm_t[sel]] + yy[T + 1:T + 1 + mI][sel]
        tausum[j] = _tree(_lane_sum(yi))
    fin = 1 + 4 * (T - 1)
    t = np.arange(T)
    p = np.where(t == T - 1, fin, 1 + 4 * t)
    yr = yy[1:T + 1]
    kch = dv[p] * yr + (-z)
    kdis = dv[p + 1] * yr + z
    up = np.empty(T)
    up[0] = dv[0] * yy[0]
    up[1:] = dv[1 + 4 * (t[1:] - 1) + 3] * yy[1:T]
    kene = up + dv[p + 2] * yr
    rch, rdis, rene = c[:T] - kch, c[T:2 * T] - kdis, c[2 * T:3 * T] - kene
    rinf = 0.0

    def bound(r, lo, hi):
        nonlocal rinf
        r, lo, hi = np.asarray(r, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        with np.errstate(invalid="ignore"):
            term = np.where(r > 0, np.where(np.isfinite(lo), lo * r, 0.0), np.where(r < 0, np.where(np.isfinite(hi), hi * r, 0.0), 0.0))
        loose = ((r > 0) & ~np.isfinite(lo)) | ((r < 0) & ~np.isfinite(hi))
        if loose.any():
            rinf = max(rinf, float(np.abs(r[loose]).max()))
        return term

    b3 = np.stack([bound(rch, l[:T], u[:T]), bound(rdis, l[T:2 * T], u[T:2 * T]),
                   bound(rene, l[2 * T:3 * T], u[2 * T:3 * T])], axis=1)
    active = np.ones(T, bool) if emax is None else (ulsoc * E <= np.asarray(emax))
    ge = np.stack([np.where(rene > 0, llsoc * rene, 0.0), np.where((rene < 0) & active, ulsoc * rene, 0.0)], axis=1)
    cx3 = np.stack([c[:T] * x[:T], c[T:2 * T] * x[T:2 * T], c[2 * T:3 * T] * x[2 * T:3 * T]], axis=1)
    m = T + 1 + mI
    s_qy = _tree(_lane_sum(q[:m] * yy[:m]))
    s_b = _tree(_lane_sum(b3))
    s_ge = _tree(_lane_sum(ge))
    s_ch = _tree(_lane_sum(np.where(rch < 0, -rch, 0.0)))
    s_dis = _tree(_lane_sum(np.where(rdis < 0, -rdis, 0.0)))
    cx = _tree(_lane_sum(cx3))
    for j in range(J):
        r = c[3 * T + j] - tausum[j]
        s_b = s_b + float(bound([r], [l[3 * T + j]], [u[3 * T + j]])[0])
        cx = cx + c[3 * T + j] * x[3 * T + j]
    dobj = (s_qy + s_b) + c0
    g_e = soc_target * (yy[0] + yy[T]) + s_ge
    g_p = -(s_ch + s_dis)
    out = np.zeros(CUT_COLS)
    out[A], out[GE], out[GP], out[DOBJ], out[POBJ], out[RINF] = (dobj - g_e * E) - g_p * P, g_e, g_p, dobj, cx + c0, rinf
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the master step on the host (value_master_kernel's, with scipy's HiGHS solving the master LP)

def master_host(cuts, spec):
    """(E, P, theta, objective) of the master LP over ``cuts`` [[a, gE, gP], ..] (scipy linprog / HiGHS)."""
    from scipy.optimize import linprog
    cuts = np.asarray(cuts, np.float64).reshape(-1, 3)
    elo, ehi, plo, phi = spec.box()
    # theta >= a + gE E + gP P   <=>   gE E + gP P - theta <= -a
    r = linprog([spec.c_energy, spec.c_power, spec.alpha], A_ub=np.column_stack([cuts[:, 1], cuts[:, 2], -np.ones(len(cuts))]),
                b_ub=-cuts[:, 0], bounds=[(elo, ehi), (plo, phi), (None, None)], method="highs")
    if r.status != 0:
        raise RuntimeError(f"master LP: {r.message}")
    return float(r.x[0]), float(r.x[1]), float(r.x[2]), float(r.fun)


def loop_host(evaluate, spec):
    """The cutting-plane loop of one case with ``evaluate(E, P) -> (sum_w V_w, sum_w a, sum_w gE, sum_w gP, ok)`` (the
    windows solved by any LP solver; ok False: a window was not optimal) and HiGHS on the master.  Returns a
    ValueSizingResult without the final solve (energy / power rounded, objective NaN)."""
    C = int(spec.candidates)
    res = ValueSizingResult()
    cuts, inc = [], None
    pts = round0_points(spec, C)
    while True:
        res.rounds += 1
        for E, P in pts:
            V, a, ge, gp, ok = evaluate(E, P)
            if not ok:
                res.status = LP_FAILED
                return res
            cuts.append((a, ge, gp))
            F = ((spec.c_energy * E + spec.c_power * P) + spec.alpha * V) + spec.ccost
            if not F >= res.upper:
                res.upper, inc = F, (E, P)
        zE, zP, _, obj = master_host(cuts, spec)
        res.lower = max(res.lower, obj + spec.ccost)
        res.n_cuts = len(cuts)
        res.energy_lp, res.power_lp = inc
        if res.upper - res.lower <= spec.gap_tol * (1.0 + abs(res.upper)):
            res.status = SIZED
            break
        if res.rounds >= spec.max_rounds or len(cuts) + C > _lib.VALUE_MAX_CUTS:
            res.status = ROUND_LIMIT
            break
        pts = [(zE, zP)] + [(inc[0] + (j / C) * (zE - inc[0]), inc[1] + (j / C) * (zP - inc[1])) for j in range(1, C)]
    _round_up(res, spec)
    return res


def _round_up(res, spec):
    elo, _, plo, _ = spec.box()
    res.energy = _sizing.candidate(res.energy_lp, elo) if spec.size_energy else res.energy_lp
    res.power = _sizing.candidate(res.power_lp, plo) if spec.size_power else res.power_lp
    res.capex = spec.capex(res.energy, res.power)


# ---------------------------------------------------------------------------------------------------------------------
# the loop on the GPU

class _Resident:
    """The cases' window inputs in HBM, and one round's packed batch built from them for a set of cases at n_cand
    candidate ratings each (window (case k, candidate j) of position p is window first_p + k n_cand + j)."""

    def __init__(self, positions, solver, device):
        import torch
        self.torch, self.solver, self.dev = torch, solver, torch.device(device)
        self.N = positions[0].G
        self.pos = []
        for s in positions:
            if s.G != self.N:
                raise ValueError("every window position needs one row per case")
            if getattr(s, "ctrl_load", None) is not None:
                raise NotImplementedError("economic sizing: windows with a controllable load are not supported")
            if getattr(s, "chp", None) is not None:
                raise NotImplementedError("economic sizing: windows with a CHP are not supported")
            if getattr(s, "ev", None) is not None:
                raise NotImplementedError("economic sizing: windows with an EV are not supported")
            if s.ice is not None or s.emin is not None:
                raise NotImplementedError("economic sizing: ICE and minimum-SOE windows are not supported")
            if s.J > _lib.VALUE_MAX_J:
                raise NotImplementedError(f"economic sizing: at most {_lib.VALUE_MAX_J} demand-charge columns")
            up = lambda a, t=torch.float64: None if a is None else torch.as_tensor(np.array(a)).to(device=self.dev, dtype=t)  # noqa: E731
            d = dict(spec=s, dcm_t=up(s.dcm_t, torch.int32), dcm_j=up(s.dcm_j, torch.int32), c0=up(s.c0))
            for name in ("base", "retail", "da", "demand", "emax"):
                d[name] = up(getattr(s, name))
            for name in ("rte", "sdr", "soc_target", "ulsoc", "llsoc", "om"):
                d[name] = up(s.scal[name])
            self.pos.append(d)

    def build(self, ids, n_cand, E, P):
        """ids: device int64 [count]; E, P: device [count * n_cand].  Returns (packed batch, group structs, firsts)."""
        from .lp import gpu_builder
        from .packed import PackedBatch
        torch = self.torch
        count = len(ids)
        G = count * n_cand
        rows = ids.repeat_interleave(n_cand)
        shapes = [gpu_builder.BatteryGroupSpec(T=d["spec"].T, J=d["spec"].J, dt=d["spec"].dt, dcm_t=d["spec"].dcm_t,
                                               dcm_j=d["spec"].dcm_j, base=np.empty((G, 0)), retail=None, da=None,
                                               demand=None, emin=None, emax=None, scal={}, c0=None) for d in self.pos]
        desc, sz = gpu_builder.desc_of(shapes)
        f64 = dict(dtype=torch.float64, device=self.dev)
        pb = PackedBatch(desc=torch.as_tensor(desc).to(self.dev),
                         indptr=torch.empty(sz["rows"], dtype=torch.int32, device=self.dev),
                         indices=torch.empty(sz["nnz"], dtype=torch.int32, device=self.dev),
                         data=torch.empty(sz["nnz"], **f64), c=torch.empty(sz["n"], **f64),
                         c0=torch.empty(len(desc), **f64), q=torch.empty(sz["m"], **f64),
                         l=torch.empty(sz["n"], **f64), u=torch.empty(sz["n"], **f64)).alloc_outputs()
        p = pb.as_ctypes()
        groups, firsts, keep = [], [], [E, P, rows]
        first = 0
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        for d in self.pos:
            s = d["spec"]
            g = _lib.BatteryGroup()
            g.T, g.J, g.G, g.mI, g.dt = s.T, s.J, G, len(s.dcm_t), s.dt
            g.has_retail, g.has_da = int(s.retail is not None), int(s.da is not None)
            g.has_emin, g.has_emax = 0, int(s.emax is not None)
            g.dcm_t, g.dcm_j = ptr(d["dcm_t"]), ptr(d["dcm_j"])
            for name in ("base", "retail", "da", "demand", "emax", "rte", "sdr", "soc_target", "ulsoc", "llsoc", "om",
                         "c0"):
                t = None if d[name] is None else d[name][rows].contiguous()
                keep.append(t)
                setattr(g, name, ptr(t))
            g.E, g.pch, g.pdis = E.data_ptr(), P.data_ptr(), P.data_ptr()
            groups.append(g)
            firsts.append(first)
            first += G
        torch.cuda.synchronize(self.dev)  # the gathers above ran on torch's stream, the builder runs on the handle's
        for g, f in zip(groups, firsts):
            self.solver._check(self.solver._lib.dvh_build_battery_group(self.solver._h, ctypes.byref(g), ctypes.byref(p), f),
                               "dvh_build_battery_group")
        pb._keep = keep
        return pb, groups, firsts

    def cuts(self, pb, groups, firsts, count, n_cand):
        """window_cuts [W][count][n_cand][CUT_COLS] of a solved batch (asynchronous on the handle's stream)."""
        torch = self.torch
        wc = torch.empty((len(groups), count, n_cand, CUT_COLS), dtype=torch.float64, device=self.dev)
        p = pb.as_ctypes()
        for i, (g, f) in enumerate(zip(groups, firsts)):
            self.solver._check(self.solver._lib.dvh_value_cuts(self.solver._h, ctypes.byref(g), ctypes.byref(p), f,
                                                               wc[i].data_ptr(), None), "dvh_value_cuts")
        return wc


def size_for_value(positions, specs, solver, device="cuda:0", dispatch=False, log=None):
    """Size ``len(specs)`` cases at once.  ``positions``: one ``gpu_builder.BatteryGroupSpec`` per window position
    (one year window, or twelve months, ..), each with one row per case; their E / pch / pdis are ignored (the loop
    supplies them) and their c0 must hold no rating-dependent term (fixedOM = 0).  Every spec needs the same
    ``candidates``.  The sizes, cuts and bounds stay in HBM; per round the host reads back the cases' flag words, and
    finished cases leave the batch.  ``log``: a list that receives one dict per round (cases, host syncs, ..).
    Returns a list of ValueSizingResult."""
    import torch
    N = len(specs)
    if N == 0:
        return []
    C = int(specs[0].candidates)
    if any(int(s.candidates) != C for s in specs):
        raise ValueError("size_for_value: every case needs the same number of candidates per round")
    if not 1 <= C <= _lib.VALUE_MAX_CAND:
        raise ValueError(f"size_for_value: candidates must be 1 .. {_lib.VALUE_MAX_CAND}")
    res_dev = _Resident(positions, solver, device)
    if res_dev.N != N:
        raise ValueError("size_for_value: the window specs need one row per case")
    dev = res_dev.dev
    n0 = max(C, 2)
    cap = min(_lib.VALUE_MAX_CUTS, n0 + C * max(int(s.max_rounds) for s in specs))
    spec_host = (_lib.ValueSpec * N)(*[s.as_struct() for s in specs])
    spec_dev = torch.frombuffer(bytearray(bytes(spec_host)), dtype=torch.uint8).to(dev)
    state = torch.zeros((N, _lib.VALUE_STATE_COLS), dtype=torch.float64, device=dev)
    state[:, 0], state[:, 1] = -math.inf, math.inf
    flags = torch.zeros((N, _lib.VALUE_FLAG_COLS), dtype=torch.int32, device=dev)
    cuts = torch.zeros((N, cap, 3), dtype=torch.float64, device=dev)
    pts = np.array([round0_points(s, C) for s in specs])  # [N, n0, 2]
    E = torch.as_tensor(np.ascontiguousarray(pts[:, :, 0].reshape(-1))).to(dev)
    P = torch.as_tensor(np.ascontiguousarray(pts[:, :, 1].reshape(-1))).to(dev)
    ids = torch.arange(N, device=dev)
    n_cand = n0
    lib, h = solver._lib, solver._h
    saved = solver.options()
    tight = min(min(float(s.gap_tol) for s in specs) / 10.0, saved.eps)
    solver.set_options(eps=tight, eps_obj=min(tight, saved.eps_obj) if saved.eps_obj > 0 else tight)
    try:
        while len(ids):
            count = len(ids)
            pb, groups, firsts = res_dev.build(ids, n_cand, E, P)
            solver.solve_packed(pb)
            syncs = solver.host_syncs() if hasattr(solver, "host_syncs") else None
            wc = res_dev.cuts(pb, groups, firsts, count, n_cand)
            E2 = torch.empty(count * C, dtype=torch.float64, device=dev)
            P2, P3 = torch.empty_like(E2), torch.empty_like(E2)
            ids32 = ids.to(torch.int32)
            torch.cuda.synchronize(dev)
            a = _lib.ValueMasterArgs()
            a.count, a.n_cases, a.W, a.n_cand, a.n_next, a.cut_cap = count, N, len(groups), n_cand, C, cap
            a.spec_host = ctypes.cast(spec_host, ctypes.POINTER(_lib.ValueSpec))
            a.spec, a.case_ids, a.window_cuts = spec_dev.data_ptr(), ids32.data_ptr(), wc.data_ptr()
            a.E_in, a.P_in, a.cuts, a.state, a.flags = E.data_ptr(), P.data_ptr(), cuts.data_ptr(), state.data_ptr(), flags.data_ptr()
            a.E_out, a.pch_out, a.pdis_out = E2.data_ptr(), P2.data_ptr(), P3.data_ptr()
            solver._check(lib.dvh_value_master(h, ctypes.byref(a), None), "dvh_value_master")
            solver._check(lib.dvh_synchronize(h), "dvh_synchronize")
            done = flags[ids, 0].cpu().numpy() != 0   # the round's only read-back
            if log is not None:
                log.append(dict(cases=count, n_cand=n_cand, windows=pb.count, solve_host_syncs=syncs,
                                finished=int(done.sum())))
            keep = torch.as_tensor(~done, device=dev)
            ids = ids[keep]
            E = E2.view(count, C)[keep].reshape(-1).contiguous()
            P = P2.view(count, C)[keep].reshape(-1).contiguous()
            n_cand = C
        st, fl = state.cpu().numpy(), flags.cpu().numpy()
        out = []
        for k, s in enumerate(specs):
            r = ValueSizingResult(lower=float(st[k, 0]), upper=float(st[k, 1]), energy_lp=float(st[k, 2]),
                                  power_lp=float(st[k, 3]), rounds=int(fl[k, 4]), n_cuts=int(fl[k, 3]),
                                  lp_iters=int(fl[k, 5]), status=int(fl[k, 1]), lp_status=int(fl[k, 2]))
            if r.status in (SIZED, ROUND_LIMIT):
                _round_up(r, s)
            out.append(r)
        # the final solve at the rounded sizes: its objective and dispatch are the result
        fin = [k for k, r in enumerate(out) if r.status in (SIZED, ROUND_LIMIT)]
        if fin:
            ids = torch.as_tensor(fin, device=dev)
            E = torch.as_tensor(np.array([out[k].energy for k in fin], np.float64)).to(dev)
            P = torch.as_tensor(np.array([out[k].power for k in fin], np.float64)).to(dev)
            pb, groups, firsts = res_dev.build(ids, 1, E, P)
            solver.solve_packed(pb)
            wc = res_dev.cuts(pb, groups, firsts, len(fin), 1)
            solver._check(lib.dvh_synchronize(h), "dvh_synchronize")
            wch = wc.cpu().numpy()[:, :, 0, :]  # [W, cases, cols]
            xh = pb.x.cpu().numpy() if dispatch else None
            desc = pb.desc.cpu().numpy() if dispatch else None
            for i, k in enumerate(fin):
                r, s = out[k], specs[k]
                V = 0.0
                for w in range(wch.shape[0]):
                    V = V + wch[w, i, POBJ]
                    r.lp_iters += int(wch[w, i, ITERS])
                    if wch[w, i, FLAG] != 0 or int(wch[w, i, STATUS]) != _lib.OPTIMAL:
                        r.status, r.lp_status = LP_FAILED, (-1 if wch[w, i, FLAG] != 0 else int(wch[w, i, STATUS]))
                r.terms = dict(energy=s.c_energy * r.energy, power=s.c_power * r.power, fixed=float(s.ccost),
                               windows=s.alpha * V, window_objectives=[float(v) for v in wch[:, i, POBJ]])
                r.objective = ((s.c_energy * r.energy + s.c_power * r.power) + s.alpha * V) + s.ccost
                if dispatch:
                    r.dispatch = [xh[int(desc[f + i, 6]):int(desc[f + i, 6]) + int(desc[f + i, 0])].copy() for f in firsts]
    finally:
        solver.set_options(eps=saved.eps, eps_obj=saved.eps_obj)
    return out
