"""Battery cycle / calendar degradation and the degradation-coupled window sweep (SURVEY.md 8b eligibility, 8e:
"with degradation on, windows of one scenario are solved as sequential batched steps").

DER-VET's Battery (dervet/MicrogridDER/Battery.py:69-110) degrades its energy capacity after every optimization
window through storagevet's BatteryTech degradation module (absent from the reference snapshot, so the model below
is a restatement of its published behaviour; parity UNPINNED):

  * calendar: yearly_degrade % per year, pro rata over the window's days (Model_Parameters_Template_DER.csv:63);
  * cycling (incl_cycle_degrade, :64): rainflow counting of the window's SOE profile (the `rainflow` 3.0.0 package,
    requirements.txt:22; ASTM E1049-85), each cycle's depth = range / rated energy looked up in the cycle-life
    table (data/battery_cycle_life.csv: "Cycle Depth Upper Limit", "Cycle Life Value" -- the first row whose upper
    limit is >= the depth), damage = sum of count / cycle life, scaled by the capacity the table's end-of-life
    condition stands for (1 - cycle_life_table_eol_condition / 100, :65);
  * degrade_perc accumulates; the effective energy capacity is rated x (1 - degrade_perc) (its SOE bounds and
    target follow); when it falls to state_of_health x rated (:90) a replaceable battery is reset to nameplate
    (Battery.py:100-110).

Window k of a scenario therefore depends on the dispatch of its windows 0..k-1, but scenarios are independent:
``DegradationSweep`` solves window position k of EVERY scenario in one batched GPU call, updates every scenario's
capacity from its solved SOE profile (vectorised across scenarios), and only then builds position k + 1 -- the
lockstep loop the drop-in runs for CVXPY windows (dropin.batched_cases_loop), here with the native builder.
"""
import ctypes
import os

import numpy as np

from . import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


def cycle_life_table(path=None):
    """(upper limits, cycle life values) of a DER-VET cycle-life CSV (default: the reference's default table,
    data/battery_cycle_life.csv -- Model_Parameters_Template_DER.csv:66 -- shipped as dervet_hip/data/)."""
    if path is None:
        path = os.path.join(HERE, "data", "battery_cycle_life.csv")
    d = np.loadtxt(path, delimiter=",", skiprows=1)
    return d[:, 0].copy(), d[:, 1].copy()


def _life(depth, upper, life):
    idx = np.minimum(np.searchsorted(upper, depth, side="left"), len(upper) - 1)
    return life[idx]


def cycle_damage(ene, e_rated, upper, life):
    """Sum over rainflow cycles of count / cycle_life(range / e_rated) for every row of ene [S, T] (SOE profiles,
    kWh), cycles taken in extraction order (oracle/rainflow_ref.py restates the counting scalar-wise).  All rows are
    counted in lock step: one pass over the T columns with per-row stacks."""
    x = np.asarray(ene, np.float64)
    S, T = x.shape
    e_rated = np.broadcast_to(np.asarray(e_rated, np.float64), (S,))
    dmg = np.zeros(S)
    if T < 2:
        return dmg
    rows = np.arange(S)
    stack = np.empty((S, T + 1))
    base = np.zeros(S, np.int64)   # first live stack slot (half cycles drop the first point)
    top = np.zeros(S, np.int64)    # one past the last

    def add(mask, rng, count):
        dmg[mask] += count / _life(rng / e_rated[mask], upper, life)

    def emit(mask, vals):
        """Push vals (rows in mask) and apply the three-point rule until it stops for every row."""
        r = rows[mask]
        stack[r, top[r]] = vals
        top[r] += 1
        act = r
        while len(act):
            act = act[top[act] - base[act] >= 3]
            if not len(act):
                break
            t = top[act]
            X = np.abs(stack[act, t - 1] - stack[act, t - 2])
            Y = np.abs(stack[act, t - 2] - stack[act, t - 3])
            go = X >= Y
            act, t, Y = act[go], t[go], Y[go]
            if not len(act):
                break
            half = (t - base[act]) == 3
            m = np.zeros(S, bool)
            m[act[half]] = True
            if half.any():
                add(m, Y[half], 0.5)
                base[act[half]] += 1
            full = ~half
            if full.any():
                f = act[full]
                m[:] = False
                m[f] = True
                add(m, Y[full], 1.0)
                tf = top[f]
                stack[f, tf - 3] = stack[f, tf - 1]
                top[f] -= 2

    # reversals, streamed: the first point, every confirmed turning point, the last point
    emit(np.ones(S, bool), x[:, 0])
    cur = x[:, 1].copy()
    d_last = cur - x[:, 0]
    for j in range(2, T):
        xn = x[:, j]
        active = xn != cur
        d = xn - cur
        rev = active & (d_last * d < 0)
        if rev.any():
            emit(rev, cur[rev])
        cur = np.where(active, xn, cur)
        d_last = np.where(active, d, d_last)
    emit(np.ones(S, bool), x[:, T - 1])
    # what is left on the stacks: half cycles, in order
    span = top - base
    for k in range(int(span.max()) - 1):
        m = span - 1 > k
        if not m.any():
            break
        r = rows[m]
        rng = np.abs(stack[r, base[r] + k + 1] - stack[r, base[r] + k])
        add(m, rng, 0.5)
    return dmg


class Degradation:
    """Degradation state of S batteries (vectorised).

    incl_cycle_degrade = False turns the whole module off, calendar loss included: dervet gates the degradation
    calls on it (Battery.py:82, :101), and the reference's own test pins it -- 041-no_Degradation_Test_MP.csv has
    yearly_degrade = 10 with incl_cycle_degrade = 0 and test_2finances.py:102-104 asserts the 2017 and 2022
    avoided energy charges are equal (tests/test_degradation_ref.py)."""

    def __init__(self, e_rated, yearly_degrade=0.0, incl_cycle_degrade=True, table=None, eol_condition=80.0,
                 state_of_health=73.0, replaceable=True):
        self.e_rated = np.asarray(e_rated, np.float64).copy()
        S = len(self.e_rated)
        self.yearly = np.broadcast_to(np.asarray(yearly_degrade, np.float64), (S,)).copy()
        self.cycle = bool(incl_cycle_degrade)
        self.upper, self.life = table if table is not None else cycle_life_table()
        self.eol = float(eol_condition)
        self.soh = np.broadcast_to(np.asarray(state_of_health, np.float64), (S,)).copy() / 100.0
        self.replaceable = np.broadcast_to(np.asarray(replaceable, bool), (S,)).copy()
        self.degrade_perc = np.zeros(S)
        self.replacements = np.zeros(S, np.int64)
        self.skipped = np.zeros(S, np.int64)  # windows whose dispatch was not used (status not OPTIMAL)
        self.years_degraded = [set() for _ in range(S)]  # Battery.py:104 years_system_degraded

    def capacity(self):
        """Effective energy capacity (kWh) the next window is built with."""
        return np.maximum(self.e_rated * (1.0 - self.degrade_perc), 0.0)

    def age(self, days):
        """Calendar loss only, e.g. from the operation year's start to the first window (Battery.py:84-85)."""
        if self.cycle and days > 0:
            self.degrade_perc += self.yearly / 100.0 * (days / 365.0)

    def update(self, ene, days, valid=None, year=None):
        """After a window of `days` days with SOE profiles ene [S, T]: returns this window's degradation [S].
        valid [S] (default all): rows whose dispatch is usable; the others take the calendar loss only (a window
        that is infeasible or failed numerically has no SOE profile to count) and are counted in ``skipped``.
        year: the window's first year, recorded when a battery reaches its state of health (Battery.py:102-104)."""
        S = len(self.e_rated)
        if not self.cycle:
            return np.zeros(S)
        d = self.yearly / 100.0 * (days / 365.0)
        ok = np.ones(S, bool) if valid is None else np.asarray(valid, bool)
        if ok.any():
            cyc = np.zeros(S)
            cyc[ok] = cycle_damage(np.asarray(ene)[ok], self.e_rated[ok], self.upper, self.life)
            d = d + cyc * (1.0 - self.eol / 100.0)
        self.skipped += ~ok
        self.degrade_perc += d
        reached = self.capacity() <= self.e_rated * self.soh
        if year is not None:
            for i in np.nonzero(reached)[0]:
                self.years_degraded[i].add(int(year))
        worn = reached & self.replaceable
        self.degrade_perc[worn] = 0.0
        self.replacements += worn
        return d


_side_streams = {}


def _enqueue(device, launch, events=None):
    """Run ``launch(hipStream_t)`` ordered with torch's current stream on ``device``, without a host wait.  The entry
    points take NULL for the handle's own stream, and torch's default stream IS the null stream, so the kernel goes
    to a side stream of this module bracketed by two device-side waits: it starts after everything enqueued on the
    current stream so far (the tensors' producers, earlier users of memory the allocator hands out again) and the
    current stream goes on after it.  events: a list that receives a (start, end) pair of timing events."""
    import torch
    cur = torch.cuda.current_stream(device)
    side = _side_streams.get(device)
    if side is None:
        side = _side_streams[device] = torch.cuda.Stream(device)
    side.wait_stream(cur)
    ev = None
    if events is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(side)
    with torch.cuda.device(device):
        launch(ctypes.c_void_p(side.cuda_stream))
    if ev is not None:
        ev[1].record(side)
        events.append(ev)
    cur.wait_stream(side)


def cycle_damage_device(ene, e_rated, upper, life, solver, T=None):
    """``cycle_damage`` on the GPU (dvh_cycle_damage): ene [S, row_stride] float64 device tensor, rows contiguous;
    T (default: the row length) leading entries of each row are counted.  e_rated: a number, an array or a device
    tensor [S].  Returns the damage as a device tensor [S], bit-identical to ``cycle_damage``, ordered with torch's
    current stream like any torch operation (``_enqueue``); nothing is waited for.  There is no host fallback: T above
    _lib.RAINFLOW_MAX_T raises."""
    import torch
    if ene.dim() != 2 or ene.dtype != torch.float64 or not ene.is_cuda or (ene.stride(1) != 1 and ene.shape[1] > 1):
        raise ValueError("cycle_damage_device needs a [S, T] float64 device tensor with contiguous rows")
    S, stride = ene.shape[0], (ene.stride(0) if ene.shape[0] > 1 else ene.shape[1])
    T = ene.shape[1] if T is None else int(T)
    f64 = dict(dtype=torch.float64, device=ene.device)
    e = e_rated if isinstance(e_rated, torch.Tensor) else \
        torch.as_tensor(np.array(np.broadcast_to(np.asarray(e_rated, np.float64), (S,)))).to(**f64)
    if e.shape != (S,) or e.dtype != torch.float64 or e.device != ene.device or not e.is_contiguous():
        raise ValueError("e_rated must broadcast to a contiguous float64 [S] on the profiles' device")
    up = torch.as_tensor(np.array(upper, np.float64)).to(**f64)
    lf = torch.as_tensor(np.array(life, np.float64)).to(**f64)
    out = torch.empty(S, **f64)
    _enqueue(ene.device, lambda stream: solver._check(
        solver._lib.dvh_cycle_damage(solver._h, ene.data_ptr(), stride, S, T, e.data_ptr(), up.data_ptr(),
                                     lf.data_ptr(), len(up), out.data_ptr(), stream), "dvh_cycle_damage"))
    return out


class DeviceDegradation:
    """A ``Degradation``'s state in device tensors, updated by dvh_degradation_update from a solved packed batch
    that never leaves HBM: ``capacity`` is the tensor the next position's builder reads its E from.

    deg: the host object whose state is mirrored (read here, written back only by ``sync_to``); solver: the
    BatchSolver whose handle runs the kernel.  Every update is ordered with torch's current stream (``_enqueue``) --
    the stream that owns the tensors involved, so their allocation, reuse and the final gather are ordered with it --
    after a solve that has returned (``solve_packed`` on the solver's own stream waits for its results) and before a
    builder that waits for the device (lp/gpu_builder.pack_specs_device); the solver's own stream would order it with
    neither.  timed: HIP events around every update (``update_ms``)."""

    def __init__(self, deg, solver, device="cuda:0", timed=False):
        import torch
        self.solver, self.dev, self.timed = solver, torch.device(device), bool(timed)
        self.cycle, self.eol = deg.cycle, deg.eol
        if len(deg.upper) > _lib.RAINFLOW_MAX_TABLE:
            raise ValueError(f"cycle-life table of {len(deg.upper)} rows (at most {_lib.RAINFLOW_MAX_TABLE})")
        up = lambda a, t=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(device=self.dev, dtype=t)
        self.e_rated, self.yearly, self.soh = up(deg.e_rated), up(deg.yearly), up(deg.soh)
        self.replaceable = up(deg.replaceable, torch.int32)
        self.degrade_perc = up(deg.degrade_perc)
        self.replacements, self.skipped = up(deg.replacements, torch.int64), up(deg.skipped, torch.int64)
        self.upper, self.life = up(deg.upper), up(deg.life)
        self.capacity = up(deg.capacity())
        self.degradation = self.reached = None  # the last update's outputs
        self.history = []                       # (reached [S], year) of every update, for sync_to
        self.events = []

    def update(self, dev_batch, T, days, year=None, first=0):
        """After the solve of ``dev_batch`` (a device PackedBatch whose windows first .. first + S - 1 are the S
        batteries' windows of T steps): ``Degradation.update`` on the device.  Returns this window's degradation
        (device tensor [S]); ``capacity`` becomes a new tensor (the one before stays valid for whoever holds it),
        ``reached`` the window's flags."""
        import torch
        S = len(self.e_rated)
        st = _lib.DegradationState()
        st.incl_cycle_degrade = int(self.cycle)
        for f in ("e_rated", "yearly", "soh", "replaceable", "degrade_perc", "replacements", "skipped"):
            setattr(st, f, getattr(self, f).data_ptr())
        cap = torch.empty(S, dtype=torch.float64, device=self.dev)
        d = torch.empty(S, dtype=torch.float64, device=self.dev)
        reached = torch.empty(S, dtype=torch.int32, device=self.dev)
        st.capacity, st.degradation, st.reached = cap.data_ptr(), d.data_ptr(), reached.data_ptr()
        p = dev_batch.as_ctypes()
        lib, h = self.solver._lib, self.solver._h
        _enqueue(self.dev, lambda stream: self.solver._check(
            lib.dvh_degradation_update(h, ctypes.byref(p), int(first), S, int(T), 2 * int(T), float(days),
                                       float(self.eol), self.upper.data_ptr(), self.life.data_ptr(), len(self.upper),
                                       ctypes.byref(st), stream), "dvh_degradation_update"),
                 self.events if self.timed else None)
        self.capacity, self.degradation, self.reached = cap, d, reached
        self.history.append((reached, year))
        return d

    def update_ms(self):
        """Kernel time of every update so far (HIP events, ms; waits for them).  timed=True only."""
        import torch
        torch.cuda.synchronize(self.dev)
        return [a.elapsed_time(b) for a, b in self.events]

    def sync_to(self, deg):
        """Write degrade_perc, replacements, skipped and (from every update's reached flags and year)
        years_degraded back into the host object: one transfer."""
        import torch
        rows = [self.degrade_perc, self.replacements.to(torch.float64), self.skipped.to(torch.float64)] + \
            [r.to(torch.float64) for r, _ in self.history]
        h = torch.stack(rows).cpu().numpy()   # (counts are exact in float64)
        deg.degrade_perc[:] = h[0]
        deg.replacements[:] = h[1].astype(np.int64)
        deg.skipped[:] = h[2].astype(np.int64)
        for flags, (_, year) in zip(h[3:], self.history):
            if year is not None:
                for i in np.nonzero(flags)[0]:
                    deg.years_degraded[i].add(int(year))
        return deg


class DegradationSweep:
    """Window positions solved in order, every scenario's window of a position in one batched solve.

    build(k, capacity [S]) -> list of WindowGroup for window position k (the scenarios' windows, in scenario order,
    e.g. ``lambda k, E: scenarios.config4(ids, E=E, only=[k])``); positions: the window ids in time order; dt: hours
    per step."""

    def __init__(self, build, positions, degradation, dt=1.0, builder=None, years=None):
        self.build, self.positions, self.deg, self.dt = build, list(positions), degradation, float(dt)
        self.builder = builder
        self.years = years  # position -> the window's first year (replacement years, Battery.py:104), optional

    def run(self, solver, device="cuda:0", resident=False, keep_x=True, timed=False):
        """Returns per position {k, iters [S], status [S], obj [S], degradation [S], capacity_before [S], ene [S, T],
        x (each window's primal solution)}.
        A solver with ``solve_packed`` (BatchSolver) gets the position's batch resident in HBM; any other solver
        with ``solve(lps)`` (e.g. the CPU restatement) gets WindowLPs.  When build returns device-builder specs
        (``scenarios.config4(..., spec=True)``) the windows are expanded on the GPU (lp/gpu_builder.py; ``builder``
        then names the BatchSolver whose handle builds them, default: solver).
        resident=True (``_run_resident``): the wear update runs on the GPU too and the capacities stay in HBM between
        the positions; same results, gathered once at the end.  keep_x=False leaves ``x`` out of them; timed: HIP
        events around the update kernels (``self.device_deg.update_ms()``)."""
        from .lp import builder, gpu_builder
        if resident:
            return self._run_resident(solver, device, keep_x, timed)
        out = []
        for k in self.positions:
            cap = self.deg.capacity()
            groups = self.build(k, cap)
            if hasattr(solver, "solve_packed") and device is not None:
                import torch
                if groups and isinstance(groups[0], gpu_builder.BatteryGroupSpec):
                    dev = gpu_builder.pack_specs_device(groups, self.builder or solver, device)
                    d = gpu_builder.desc_of(groups)[0]
                else:
                    pb = builder.pack_groups(groups)
                    dev = pb.to_torch(device).alloc_outputs()
                    d = np.asarray(pb.desc)
                solver.solve_packed(dev)
                torch.cuda.synchronize()
                x = dev.x.cpu().numpy()
                ist = dev.istats.cpu().numpy()
                obj = dev.stats.cpu().numpy()[:, 0]
                del dev
                T = int(d[0, 2]) - 1
                ene = np.stack([x[int(r[6]) + 2 * T:int(r[6]) + 3 * T] for r in d])
                xs = [x[int(r[6]):int(r[6]) + int(r[0])] for r in d]
            else:
                lps = [lp for g in groups for lp in builder.group_window_lps(g)]
                res = solver.solve(lps)
                ist = np.array([[r.status, r.iters] for r in res])
                obj = np.array([r.obj for r in res])
                T = lps[0].m_eq - 1
                ene = np.stack([r.x[2 * T:3 * T] for r in res])
                xs = [np.asarray(r.x) for r in res]
            # only OPTIMAL dispatch is counted (an infeasible window's x is no SOE profile; VERDICT r04:
            # nor is an ITER_LIMIT one, which failed the KKT test) -- the others are counted in Degradation.skipped
            valid = ist[:, 0] == 0
            if not valid.all():  #  a skipped window gets calendar loss only: say so, it biases wear low
                import warnings
                warnings.warn(f"degradation sweep, window position {k}: {int((~valid).sum())} of {len(valid)} windows "
                              f"not OPTIMAL (statuses {sorted(set(int(v) for v in ist[~valid, 0]))}); their cycle wear "
                              "is not counted (Degradation.skipped)", RuntimeWarning, stacklevel=2)
            deg = self.deg.update(ene, T * self.dt / 24.0, valid=valid,
                                  year=None if self.years is None else self.years[k])
            out.append(dict(k=k, iters=ist[:, 1], status=ist[:, 0], obj=obj, degradation=deg, capacity_before=cap,
                            ene=ene, x=xs))
        return out

    def _run_resident(self, solver, device, keep_x, timed):
        """The sweep with nothing crossing to the host between the positions.  ``build`` must return device-builder
        specs of one window length, and is called with the RATED capacities: a spec depends on the capacity through
        ``scal["E"]`` alone (lp/gpu_builder.battery_group_spec copies bat["E"] there and uses it nowhere else; the
        builder, csrc/dvh_build.hip, reads it from device memory), so each spec's E is replaced by the matching slice
        of the device capacity tensor.  A build whose other inputs depend on its capacity argument (power ratings
        scaled with it, an SOE requirement clipped to it) does not fit this contract and keeps the host path.
        Per position the batch is built, solved and handed to ``DeviceDegradation.update``; the position's device
        tensors are kept, and one transfer after the last position (``_gather``) produces the host path's list;
        ``self.deg`` is brought up to date then (``sync_to``)."""
        import torch
        from .lp import gpu_builder
        if not hasattr(solver, "solve_packed") or device is None:
            raise ValueError("resident=True needs a GPU solver (solve_packed) and a device")
        handle = self.builder or solver
        dd = self.device_deg = DeviceDegradation(self.deg, handle, device, timed=timed)
        rated = self.deg.e_rated.copy()
        rated.flags.writeable = False
        kept = []
        for k in self.positions:
            specs = self.build(k, rated)
            if not specs or not all(isinstance(g, gpu_builder.BatteryGroupSpec) for g in specs):
                raise ValueError("resident=True needs device-builder specs (gpu_builder.BatteryGroupSpec, e.g. "
                                 "scenarios.config4(..., spec=True)); host-built groups keep resident=False")
            if len({g.T for g in specs}) != 1 or sum(g.G for g in specs) != len(rated):
                raise ValueError("resident=True needs one window of one length per battery at every position")
            cap, first = dd.capacity, 0
            for g in specs:
                g.scal = dict(g.scal, E=cap[first:first + g.G])
                first += g.G
            dev = gpu_builder.pack_specs_device(specs, handle, device)
            solver.solve_packed(dev)
            T = specs[0].T
            deg = dd.update(dev, T, T * self.dt / 24.0, year=None if self.years is None else self.years[k])
            n = {g.n for g in specs}
            if len(n) == 1:  # equal windows: the SOE columns are a strided view of x
                ene = dev.x.view(len(rated), n.pop())[:, 2 * T:3 * T]
            else:
                ene = dev.x[dev.desc[:, 6:7] + torch.arange(2 * T, 3 * T, device=dev.x.device)]
            kept.append(dict(k=k, ene=ene if keep_x else ene.clone(), istats=dev.istats, obj=dev.stats.view(-1, 4)[:, 0],
                             degradation=deg, capacity_before=cap, x=dev.x if keep_x else None,
                             desc=gpu_builder.desc_of(specs)[0] if keep_x else None))
            del dev
        self.device_results = kept   # (device tensors until _gather: nothing was read back inside the loop)
        dd.sync_to(self.deg)         # the host object ends where the host path leaves it
        return self._gather(kept)

    def _gather(self, kept):
        """The kept device tensors as the host path's list of dicts: one transfer (float64; status and iteration
        counts are exact in it), plus one per position for x when it was kept.  Issues the not-OPTIMAL warnings."""
        import torch
        import warnings
        if not kept:
            return []
        f64 = torch.float64
        cols = [torch.cat([p["ene"], p["obj"][:, None], p["degradation"][:, None], p["capacity_before"][:, None],
                           p["istats"].view(-1, 2).to(f64)], dim=1) for p in kept]
        h = torch.cat([c.reshape(-1) for c in cols]).cpu().numpy()   # (the positions' T differ: months)
        ends = np.cumsum([c.numel() for c in cols])
        out = []
        for p, c, end in zip(kept, cols, ends):
            a = h[end - c.numel():end].reshape(c.shape)
            T = a.shape[1] - 5
            status, iters = a[:, T + 3].astype(np.int32), a[:, T + 4].astype(np.int32)
            valid = status == 0
            if not valid.all():
                warnings.warn(f"degradation sweep, window position {p['k']}: {int((~valid).sum())} of {len(valid)} "
                              f"windows not OPTIMAL (statuses {sorted(set(int(v) for v in status[~valid]))}); their "
                              "cycle wear is not counted (Degradation.skipped)", RuntimeWarning, stacklevel=4)
            r = dict(k=p["k"], iters=iters, status=status, obj=a[:, T].copy(), degradation=a[:, T + 1].copy(),
                     capacity_before=a[:, T + 2].copy(), ene=a[:, :T].copy())
            if p["x"] is not None:
                x = p["x"].cpu().numpy()
                r["x"] = [x[int(d[6]):int(d[6]) + int(d[0])] for d in p["desc"]]
            out.append(r)
        return out
