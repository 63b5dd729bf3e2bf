"""Scenario valuation: the monthly bill of every solved window, and per scenario the pro forma, its present values,
payback and IRR (dervet/CBA.py:215-233, 299-346, 479-523 on storagevet's Financial, which is absent; restated as far
as the Usecase 2 goldens simple_monthly_bill / pro_forma / npv / payback / cost_benefit pin it).

Two forms of the same operations (csrc/dvh_cba.h is the third, the one the kernels compile):

  * on the device -- ``bill_windows`` (dvh_bill_windows, one workgroup per window reading the dispatch where the solve
    left it), ``value_scenarios`` (dvh_value_scenarios, one thread per scenario) and ``value_sweep``, which values a
    ``sweep.SeededSweep``: only [S, 7] numbers come back to the host, not the dispatch;
  * on the host in numpy -- ``bill_windows_host`` and ``value_scenarios_host``, the parity reference of the kernels
    (as ``degradation.cycle_damage`` is for the rainflow kernel): every product, sum and comparison in the kernels'
    order, the bill's sums in the order a 256-thread workgroup forms them, so peaks and bills agree bit for bit.

The bill bills the dispatch's own peaks, not the LP's tau columns (the reference bills from the time series, and tau is
only within solver tolerance of the peak).  Not restated (zero in every golden; pass them through ``Financials.extra``):
taxes and MACRS, replacement, salvage and decommissioning, ECC.  With several opt years a year that is not an opt year
takes the nearest earlier opt year's value escalated by the column's growth rate (UNPINNED: every golden has one).
The golden payback file's "Cost-Benefit Ratio" is cost / benefit, from an older reference version; ``bc_ratio`` is
benefit / cost as dervet/CBA.py:510-523 has it, and the two present values are what the tests pin.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _lib

BILL_ROWS, BILL_MAX_J, LANES, WAVE = _lib.BILL_ROWS, _lib.BILL_MAX_J, 256, 64
MAX_YEARS, MAX_EXTRA, FIXED_COLS, VALUE_COLS = _lib.CBA_MAX_YEARS, _lib.CBA_MAX_EXTRA, _lib.CBA_FIXED_COLS, _lib.VALUE_COLS
RETAIL, DEMAND, DA, VAR_OM, FUEL, ORIG_RETAIL, ORIG_DEMAND, ORIG_DA = range(BILL_ROWS)
BILL_NAMES = ("energy_charge", "demand_charge", "da_cost", "var_om", "fuel", "original_energy_charge",
              "original_demand_charge", "original_da_cost")
PROFORMA_COLS = ("Capital Cost", "Avoided Energy Charge", "Avoided Demand Charge", "DA Value", "Variable O&M Cost",
                 "Fuel Cost", "Fixed O&M Cost")
VALUE_NAMES = ("npv", "pv_cost", "pv_benefit", "bc_ratio", "payback", "discounted_payback", "irr")
BAD_WINDOW, BAD_ROW = 1, 2
IRR_STEP, IRR_GRID = 1.0625, 128


@dataclass
class Financials:
    """The financial inputs of a valuation.  years: pro forma years after the CAPEX row (Y); opt_years: their indices
    (0 = the first year after the CAPEX row) that were optimised, ascending; rate: npv discount rate (fraction);
    growth: %/yr of the bill-derived columns (avoided energy, avoided demand, DA value, variable O&M, fuel; one number
    for all, or five); capex [S] $, fixed_om [S] $/yr (scalars broadcast); extra [n_extra, Y + 1] $: yearly columns
    shared by the scenarios, added verbatim (the golden's Tax Credit, Other Incentives, User Constraints Value).
    windows_per_year: a sweep's window tag w belongs to opt year opt_years[w // windows_per_year] (value_sweep)."""
    years: int
    opt_years: tuple = (0,)
    rate: float = 0.0
    growth: object = 0.0
    capex: object = 0.0
    fixed_om: object = 0.0
    extra: object = None
    windows_per_year: int = 12

    def arrays(self, S):
        Y = int(self.years)
        if not 1 <= Y <= MAX_YEARS:
            raise ValueError(f"years = {Y} (1 .. {MAX_YEARS})")
        opt = np.asarray(self.opt_years, np.int32).reshape(-1)
        growth = np.array(np.broadcast_to(np.asarray(self.growth, np.float64), (5,)))
        extra = np.zeros((0, Y + 1)) if self.extra is None else np.ascontiguousarray(self.extra, np.float64)
        if extra.ndim != 2 or extra.shape[1] != Y + 1 or extra.shape[0] > MAX_EXTRA:
            raise ValueError(f"extra must be [n_extra <= {MAX_EXTRA}, years + 1]")
        bc = lambda a: np.array(np.broadcast_to(np.asarray(a, np.float64), (S,)))  # noqa: E731
        return Y, opt, float(self.rate), growth, bc(self.capex), bc(self.fixed_om), extra


@dataclass
class BillInputs:
    """What the bill reads of one window group (the compact series of dvh_battery_group plus orig)."""
    T: int
    J: int
    dt: float
    dcm_t: np.ndarray
    dcm_j: np.ndarray
    base: object            # [G, T]
    retail: object = None   # [G, T] or None
    da: object = None
    demand: object = None   # [G, J]
    om: object = None       # [G] $/MWh or None
    ice_cost: object = None  # [G] or None: no ICE block
    has_pv: bool = False    # a curtailable-PV block after tau
    orig: object = None     # [G, T] site load alone, or None: base
    has_ev: bool = False    # an EV block (ev_ch, ev_ene) after tau; not with has_pv / ice_cost

    @property
    def G(self):
        return self.base.shape[0]

    @property
    def need(self):
        return 3 * self.T + self.J + (self.T if self.has_pv else 0) + \
            (2 * self.T if self.ice_cost is not None else 0) + (2 * self.T if self.has_ev else 0)


def bill_inputs(g, orig=None):
    """BillInputs of a gpu_builder.BatteryGroupSpec, of a builder.WindowGroup built by battery_group (its ``inputs``),
    or of a BillInputs (orig replaced when given)."""
    if isinstance(g, BillInputs):
        return g if orig is None else BillInputs(**{**g.__dict__, "orig": orig})
    if hasattr(g, "scal"):  # BatteryGroupSpec
        return BillInputs(T=g.T, J=g.J, dt=g.dt, dcm_t=g.dcm_t, dcm_j=g.dcm_j, base=g.base, retail=g.retail, da=g.da,
                          demand=g.demand, om=g.scal["om"], ice_cost=g.ice["cost"] if g.ice else None, orig=orig,
                          has_ev=g.ev is not None)
    inp = getattr(g, "inputs", None)
    if getattr(g, "ctrl_load", None) is not None:
        raise NotImplementedError("bill: windows with a controllable load are not valued")
    if getattr(g, "chp", None) is not None:
        raise NotImplementedError("bill: windows with a CHP are not valued")
    if inp is None:
        raise ValueError("bill: the window group carries no series (builder.battery_group records them in .inputs)")
    # (an EV group's inputs also carry what the device builder reads: ev_ch_max, ev_target, ev_code, ev_fixed_om)
    return BillInputs(**{k: v for k, v in inp.items() if k in BillInputs.__dataclass_fields__}, orig=orig)


# ---- host form of bill_kernel

def _block_sum(a):
    """Row sums of a [G, T] in the bill workgroup's order: lane l adds the terms l, l + 256, .. in step order, each
    wave halves its 64 partials five times, the four wave sums are added in wave order."""
    G, T = a.shape
    K = -(-T // LANES)
    p = np.zeros((G, K * LANES))
    p[:, :T] = a
    p = p.reshape(G, K, LANES)
    acc = np.zeros((G, LANES))
    for k in range(K):
        acc = acc + p[:, k, :]
    v = acc.reshape(G, LANES // WAVE, WAVE)
    o = WAVE // 2
    while o > 0:
        v = v[:, :, :o] + v[:, :, o:2 * o]
        o //= 2
    r = v[:, 0, 0]
    for w in range(1, LANES // WAVE):
        r = r + v[:, w, 0]
    return r


def bill_windows_host(inp, x, status=None):
    """The bill of one group's G windows from their solutions, in bill_kernel's operations.  x: [G, n] array, or a
    list of G vectors (None, or one shorter than the layout needs: a bad window); status [G] (0 = optimal) or None.
    Returns (bills [G, BILL_ROWS], peaks [G, J] kW, bad [G] int32)."""
    inp = bill_inputs(inp)
    G, T, J, dt = inp.G, inp.T, inp.J, inp.dt
    if J > BILL_MAX_J:
        raise ValueError(f"bill: J = {J} demand-charge columns (at most {BILL_MAX_J})")
    has_ice = inp.ice_cost is not None
    ok = np.ones(G, bool) if status is None else np.asarray(status) == 0
    X = np.zeros((G, inp.need))
    for k in range(G):
        xk = None if x is None else x[k]
        if xk is None or len(xk) < inp.need:
            ok[k] = False
        elif ok[k]:
            X[k] = np.asarray(xk, np.float64)[:inp.need]
    base = np.asarray(inp.base, np.float64)
    orig = base if inp.orig is None else np.asarray(inp.orig, np.float64)
    ch, dis = X[:, :T], X[:, T:2 * T]
    net = (base + ch) - dis
    col = 3 * T + J
    if inp.has_pv:
        net = net - X[:, col:col + T]
        col += T
    if has_ice:
        elec = X[:, col:col + T]
        net = net - elec
    if inp.has_ev:  # the EV's charging is net load
        net = net + X[:, col:col + T]
    bills = np.zeros((G, BILL_ROWS))
    for price, row, orow in ((inp.retail, RETAIL, ORIG_RETAIL), (inp.da, DA, ORIG_DA)):
        if price is not None:
            pr = np.asarray(price, np.float64) * dt
            bills[:, row] = _block_sum(pr * net)
            bills[:, orow] = _block_sum(pr * orig)
    om = np.zeros(G) if inp.om is None else np.asarray(inp.om, np.float64)
    bills[:, VAR_OM] = (om / 1000.0 * dt) * _block_sum(dis)
    if has_ice:
        bills[:, FUEL] = np.asarray(inp.ice_cost, np.float64) * _block_sum(elec)
    dcm_t, dcm_j = np.asarray(inp.dcm_t, np.int64), np.asarray(inp.dcm_j, np.int64)
    good = (dcm_j >= 0) & (dcm_j < J) & (dcm_t >= 0) & (dcm_t < T)
    peaks = np.zeros((G, J))
    dem, odem = np.zeros(G), np.zeros(G)
    demand = np.zeros((G, J)) if inp.demand is None else np.asarray(inp.demand, np.float64).reshape(G, J)
    for j in range(J):
        rows = dcm_t[good & (dcm_j == j)]
        if len(rows):
            peaks[:, j] = net[:, rows].max(axis=1)
            odem = odem + demand[:, j] * orig[:, rows].max(axis=1)
        else:
            odem = odem + demand[:, j] * 0.0
        dem = dem + demand[:, j] * peaks[:, j]
    bills[:, DEMAND], bills[:, ORIG_DEMAND] = dem, odem
    bills[~ok, :ORIG_RETAIL] = np.nan
    peaks[~ok] = np.nan
    bad = np.where(ok, 0, BAD_WINDOW).astype(np.int32) | (0 if good.all() else BAD_ROW)
    return bills, peaks, bad.astype(np.int32)


# ---- host form of valuation_kernel

def _pw(b, k):
    r = 1.0
    for _ in range(k):
        r = r * b
    return r


def _npv_at(net, x):
    acc = net[:, -1].copy()
    for k in range(net.shape[1] - 2, -1, -1):
        acc = acc / x + net[:, k]
    return acc


def _irr(net):
    """cba::irr over the rows of net [S, Y + 1]: the bracket nearest rate 0 on the grid 1 + rate = (17/16)^i, searched
    outward (the upper interval of a pair first), bisected to 1e-13; NaN without a bracket."""
    S = net.shape[0]
    out = np.full(S, np.nan)
    with np.errstate(all="ignore"):
        f1 = _npv_at(net, 1.0)
        done = (f1 == 0.0) | np.isnan(f1)
        out[f1 == 0.0] = 0.0
        lo, flo, hi = np.zeros(S), np.zeros(S), np.zeros(S)
        brack = np.zeros(S, bool)
        xu = xd = 1.0
        fu, fd = f1.copy(), f1.copy()
        for _ in range(IRR_GRID):
            for up in (True, False):
                xa = xu if up else xd
                fa = fu if up else fd
                xn = xa * IRR_STEP if up else xa / IRR_STEP
                fn = _npv_at(net, xn)
                live = ~done
                z = live & (fn == 0.0)
                out[z] = xn - 1.0
                done = done | z | (live & np.isnan(fn))
                live = ~done
                b = live & ((fn < 0.0) != (fa < 0.0))
                if up:
                    lo[b], flo[b], hi[b] = xa, fa[b], xn
                else:
                    lo[b], flo[b], hi[b] = xn, fn[b], xa
                brack |= b
                done = done | b
                if up:
                    xu, fu = xn, fn
                else:
                    xd, fd = xn, fn
        act = brack.copy()
        while act.any():
            act = act & (hi - lo > 1e-13)
            mid = 0.5 * (lo + hi)
            act = act & (mid > lo) & (mid < hi)
            if not act.any():
                break
            fm = _npv_at(net, np.where(act, mid, 1.0))
            z = act & (fm == 0.0)
            out[z] = mid[z] - 1.0
            brack = brack & ~z
            act = act & ~z
            same = (fm < 0.0) == (flo < 0.0)
            a = act & same
            lo[a], flo[a] = mid[a], fm[a]
            a = act & ~same
            hi[a] = mid[a]
        out[brack] = 0.5 * (lo[brack] + hi[brack]) - 1.0
    return out


def value_scenarios_host(bills, bad, win_ptr, win_idx, win_year, fin):
    """valuation_kernel's operations in numpy.  bills [n_bills, BILL_ROWS], bad [n_bills] or None; the CSR map
    win_ptr [S + 1], win_idx, win_year (see dvh_value_scenarios).  Returns a Valuation of numpy arrays, proforma
    [S, Y + 1, 7 + n_extra] included."""
    bills = np.asarray(bills, np.float64).reshape(-1, BILL_ROWS)
    win_ptr, win_idx, win_year = (np.asarray(a, np.int64) for a in (win_ptr, win_idx, win_year))
    S = len(win_ptr) - 1
    Y, opt, rate, growth, capex, fixed_om, extra = fin.arrays(S)
    nb, C = len(bills), FIXED_COLS + len(extra)
    x1 = 1.0 + rate
    cnt = np.diff(win_ptr)
    inr = (win_idx >= 0) & (win_idx < nb)
    sid = np.repeat(np.arange(S), cnt)
    valid = np.ones(S, bool)
    bad_e = ~inr | ~np.isin(win_year, opt)
    if bad is not None:
        bad_e = bad_e | (np.asarray(bad)[np.where(inr, win_idx, 0)] != 0)
    valid[sid[bad_e]] = False
    for o in opt:
        has = np.zeros(S, bool)
        has[sid[win_year == o]] = True
        valid &= has
    safe = np.where(inr, win_idx, 0)
    with np.errstate(all="ignore"):
        r = bills[safe] if nb else np.zeros((len(win_idx), BILL_ROWS))
        term = np.stack([r[:, ORIG_RETAIL] - r[:, RETAIL], r[:, ORIG_DEMAND] - r[:, DEMAND], r[:, ORIG_DA] - r[:, DA],
                         -r[:, VAR_OM], -r[:, FUEL]], axis=1)
        # opt-year values: each scenario's entries added in CSR order (position by position across the scenarios)
        V = np.zeros((len(opt), 5, S))
        for p in range(int(cnt.max()) if S else 0):
            live = cnt > p
            e = win_ptr[:-1][live] + p
            for oi, o in enumerate(opt):
                take = inr[e] & (win_year[e] == o)
                V[oi][:, np.nonzero(live)[0][take]] += term[e[take]].T
        pf = np.zeros((S, Y + 1, C))
        pf[:, 0, 0] = -capex
        for b in range(5):
            g1 = 1.0 + growth[b] / 100.0
            for y in range(Y):
                o = max(0, int(np.searchsorted(opt, y, side="right")) - 1)
                d = y - int(opt[o])
                pf[:, y + 1, 1 + b] = V[o, b] * _pw(g1, d) if d >= 0 else V[o, b] / _pw(g1, -d)
        pf[:, 1:, FIXED_COLS - 1] = -fixed_om[:, None]
        pf[:, :, FIXED_COLS:] = extra.T[None]
        disc = np.ones(Y + 1)
        for k in range(1, Y + 1):
            disc[k] = disc[k - 1] * x1
        net = np.zeros((S, Y + 1))
        cost, ben = np.zeros(S), np.zeros(S)
        for c in range(C):
            pv = np.zeros(S)
            for k in range(Y + 1):
                if (c == 0 and k > 0) or (0 < c < FIXED_COLS and k == 0):
                    continue  # (entries the kernel does not add: the capex column's years, the yearly columns' row 0)
                pv = pv + pf[:, k, c] / disc[k]
                net[:, k] = net[:, k] + pf[:, k, c]
            nan = np.isnan(pv)
            cost = np.where(nan, np.nan, cost + np.where(pv < 0.0, -pv, 0.0))
            ben = np.where(nan, np.nan, ben + np.where(pv > 0.0, pv, 0.0))
        npv = np.zeros(S)
        for k in range(Y + 1):
            npv = npv + net[:, k] / disc[k]
        values = np.full((S, VALUE_COLS), np.nan)
        values[:, 0], values[:, 1], values[:, 2] = npv, cost, ben
        values[:, 3] = np.where(np.abs(cost) <= 1e-8, np.nan, ben / cost)
        cap, net1 = -net[:, 0], net[:, 1]
        pos = net1 > 0.0
        values[:, 4] = np.where(pos, cap / net1, np.nan)
        if rate == 0.0:
            values[:, 5] = values[:, 4]
        else:
            arg = 1.0 - cap * rate / net1
            values[:, 5] = np.where(pos & (arg > 0.0), np.log(1.0 / arg) / np.log(x1), np.nan)
        values[:, 6] = _irr(net)
    return Valuation(values=values, valid=valid.astype(np.int32), proforma=pf)


@dataclass
class Valuation:
    """values [S, VALUE_COLS], valid [S] int32, proforma [S, Y + 1, C] or None: device tensors from value_scenarios /
    value_sweep (``numpy()`` copies them to the host), numpy arrays from value_scenarios_host."""
    values: object
    valid: object
    proforma: object = None
    scenarios: object = None   # value_sweep: the scenario id of each row
    bills: object = None       # value_sweep: the Bills it valued

    def numpy(self):
        h = lambda v: v if v is None or isinstance(v, np.ndarray) else v.detach().cpu().numpy()  # noqa: E731
        return Valuation(h(self.values), h(self.valid), h(self.proforma), self.scenarios, self.bills)



for _i, _name in enumerate(VALUE_NAMES):  # .npv, .pv_cost, .pv_benefit, .bc_ratio, .payback, .discounted_payback, .irr
    setattr(Valuation, _name, property(lambda self, _i=_i: self.values[:, _i]))


# ---- device

@dataclass
class Bills:
    """bills [count, BILL_ROWS], bad [count] int32 (device tensors); peaks: per group [G, J] or None; series: per group
    the device tensors the kernel read (the builder's own where the batch was built from specs on the device)."""
    bills: object
    bad: object
    peaks: list = None
    series: list = field(default_factory=list)


_SERIES = ("dcm_t", "dcm_j", "base", "retail", "da", "demand", "om", "ice_cost")


def bill_windows(solver, dev, groups_or_specs, orig=None, first=0, peaks=False):
    """The bill of the solved windows first .. of the device PackedBatch ``dev``, group after group in packing order
    (dvh_bill_windows), ordered with torch's current stream; nothing is waited for.  groups_or_specs: the groups the
    windows were built from (BatteryGroupSpec, WindowGroup of battery_group, or BillInputs); orig: per group the site
    load alone [G, T] (array or device tensor), or None: the group's base.  Where ``dev`` was built from specs on the
    device (gpu_builder.pack_specs_device) the kernel reads the series the builder uploaded (``dev.series``); any other
    group uploads its series once.  Returns a Bills."""
    import torch
    from .degradation import _enqueue
    groups = list(groups_or_specs)
    device = dev.x.device
    count = sum(bill_inputs(g).G for g in groups)
    if first < 0 or first + count > dev.count:
        raise ValueError(f"bill: windows {first} .. {first + count - 1} outside the batch of {dev.count}")
    out = torch.empty((count, BILL_ROWS), dtype=torch.float64, device=device)
    bad = torch.empty(count, dtype=torch.int32, device=device)
    resident = getattr(dev, "series", None)
    if resident is not None and (first != 0 or len(resident) != len(groups)):
        resident = None
    p = dev.as_ctypes()
    pk_out, used, calls = [], [], []
    k = 0
    for gi, g in enumerate(groups):
        inp = bill_inputs(g, None if orig is None else orig[gi])
        ser = {}
        for name in _SERIES:
            t = resident[gi].get(name) if resident is not None and hasattr(g, "scal") else None
            if t is None and getattr(inp, name) is not None:
                dt_ = torch.int32 if name.startswith("dcm") else torch.float64
                t = torch.as_tensor(np.array(getattr(inp, name))).to(device=device, dtype=dt_)  # (a copy: may be read-only)
            ser[name] = t
        o = inp.orig
        if o is not None and not isinstance(o, torch.Tensor):
            o = torch.as_tensor(np.array(o, np.float64)).to(device)
        if o is not None and (o.numel() != inp.G * inp.T or o.dtype != torch.float64 or not o.is_contiguous()):
            raise ValueError("bill: orig must be a contiguous float64 [G, T]")
        ser["orig"] = o
        bg = _lib.BillGroup()
        bg.T, bg.J, bg.G, bg.mI, bg.dt = inp.T, inp.J, inp.G, len(inp.dcm_t), inp.dt
        bg.has_pv, bg.has_ice, bg.has_ev = int(inp.has_pv), int(inp.ice_cost is not None), int(inp.has_ev)
        for name, t in ser.items():
            setattr(bg, name, None if t is None or t.numel() == 0 else t.data_ptr())
        pk = torch.empty((inp.G, inp.J), dtype=torch.float64, device=device) if peaks else None
        calls.append((bg, first + k, out[k:].data_ptr(), None if pk is None or pk.numel() == 0 else pk.data_ptr(),
                      bad[k:].data_ptr()))
        pk_out.append(pk)
        used.append(ser)
        k += inp.G

    def launch(stream):  # one launch per group, all between one pair of stream waits
        for bg, w0, po, pp, pf in calls:
            solver._check(solver._lib.dvh_bill_windows(solver._h, ctypes.byref(bg), ctypes.byref(p), w0, po, pp, pf,
                                                       stream), "dvh_bill_windows")
    _enqueue(device, launch)
    return Bills(bills=out, bad=bad, peaks=pk_out if peaks else None, series=used)


def value_scenarios(solver, bills, bad, win_ptr, win_idx, win_year, fin, proforma=False):
    """dvh_value_scenarios: bills [n_bills, BILL_ROWS] / bad [n_bills] (or None) device tensors, the CSR map as host
    arrays.  Ordered with torch's current stream; nothing is waited for.  Returns a Valuation of device tensors."""
    import torch
    from .degradation import _enqueue
    device = bills.device
    wp = np.ascontiguousarray(win_ptr, np.int64)
    S = len(wp) - 1
    Y, opt, rate, growth, capex, fixed_om, extra = fin.arrays(S)
    opt = np.ascontiguousarray(opt, np.int32)
    up = lambda a, t: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=t)  # noqa: E731
    d = dict(win_ptr=up(wp, torch.int64), win_idx=up(win_idx, torch.int32), win_year=up(win_year, torch.int32),
             capex=up(capex, torch.float64), fixed_om=up(fixed_om, torch.float64), extra=up(extra, torch.float64))
    v = _lib.ValuationArgs()
    v.S, v.Y, v.n_opt, v.n_extra = S, Y, len(opt), len(extra)
    v.n_win, v.n_bills = len(d["win_idx"]), bills.shape[0]
    v.opt_years = opt.ctypes.data_as(_lib.c_int32_p)
    v.win_ptr_host = wp.ctypes.data_as(_lib.c_int64_p)
    for name, t in d.items():
        setattr(v, name, t.data_ptr() if t.numel() else None)
    v.win_ptr = d["win_ptr"].data_ptr()
    v.bills = bills.data_ptr() if bills.numel() else None
    v.bad = None if bad is None else bad.data_ptr()
    v.rate = rate
    v.growth = (ctypes.c_double * 5)(*growth)
    values = torch.empty((S, VALUE_COLS), dtype=torch.float64, device=device)
    valid = torch.empty(S, dtype=torch.int32, device=device)
    pf = torch.empty((S, Y + 1, FIXED_COLS + len(extra)), dtype=torch.float64, device=device) if proforma else None
    _enqueue(device, lambda stream: solver._check(solver._lib.dvh_value_scenarios(
        solver._h, ctypes.byref(v), values.data_ptr(), valid.data_ptr(), None if pf is None else pf.data_ptr(), stream),
        "dvh_value_scenarios"))
    return Valuation(values=values, valid=valid, proforma=pf)


def sweep_map(tags, fin):
    """The CSR map of a sweep's windows from their (scenario, window) tags in packing order: scenarios in ascending id,
    each one's windows in (opt year, window) order.  Returns (scenario ids, win_ptr, win_idx, win_year)."""
    sc = np.array([t[0] for t in tags], np.int64)
    w = np.array([t[1] for t in tags], np.int64)
    ids, inv = np.unique(sc, return_inverse=True)
    order = np.lexsort((w, inv))
    opt = np.asarray(fin.opt_years, np.int64)
    o = w[order] // int(fin.windows_per_year)
    year = np.where(o < len(opt), opt[np.minimum(o, len(opt) - 1)], -1)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(ids)))]).astype(np.int64)
    return ids, ptr, order.astype(np.int32), year.astype(np.int32)


def value_sweep(sweep, solver, dev, fin, orig=None, groups=None, proforma=False):
    """Bills and values a solved ``sweep.SeededSweep`` on the device: ``dev`` is its packed batch after
    ``sweep.solve``.  A sweep packs its seeds first, so a scenario's windows are scattered over the batch: the CSR map
    comes from ``sweep.tags``.  fin.capex / fixed_om: scalars, or [S] in ascending scenario id (``.scenarios``).
    groups: the window groups of a host-built sweep in packing order (a spec-built sweep has its own)."""
    groups = sweep.specs if groups is None else groups
    if groups is None:
        raise ValueError("value_sweep: a host-built sweep needs its window groups (packing order)")
    b = bill_windows(solver, dev, groups, orig=orig)
    ids, ptr, idx, year = sweep_map(sweep.tags, fin)
    val = value_scenarios(solver, b.bills, b.bad, ptr, idx, year, fin, proforma=proforma)
    val.scenarios, val.bills = ids, b
    return val


def last_ms(solver):
    """Kernel times of the solver's most recent bill and valuation calls: {bill_ms, valuation_ms} (waits for them)."""
    ms = (ctypes.c_double * 2)()
    solver._check(solver._lib.dvh_last_valuation_ms(solver._h, ms), "dvh_last_valuation_ms")
    return {"bill_ms": ms[0], "valuation_ms": ms[1]}
