"""Timing probe of the degradation-coupled sweep: the existing path (every position's x copied to the host, rainflow
wear in numpy, capacities handed back as host arrays) against the resident path (DegradationSweep.run(resident=True):
dvh_degradation_update on the GPU, capacities in HBM from one position to the next, one gather at the end).

In one process, per size: the config-4 sweep of bench_configs.degradation_sweep (12 monthly positions, windows built
on the device, cycle + calendar degradation at 2 %/yr) through both paths, a warm-up and `--reps` repeats each.
Prints the wall medians and min-max, the solves' time summed over the positions (the solver's HIP events), the update
kernels' time (HIP events) next to the solve of the same position, and checks that the two paths return the same
results.  The keep-criterion (profiles/INDEX.md): the resident path's slowest repeat is faster than the existing
path's fastest.

Usage: python scripts/probe_degradation.py [--sizes 1000 10000] [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "der-vet_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from dervet_hip import BatchSolver, degradation  # noqa: E402
from dervet_hip.lp import scenarios  # noqa: E402

POSITIONS = range(12)
FIELDS = ("ene", "iters", "status", "obj", "degradation", "capacity_before")


class Timed:
    """The solver, recording every solve's HIP-event time (dvh_last_timing)."""

    def __init__(self, s):
        self.s, self.ms = s, []

    def solve_packed(self, dev):
        self.s.solve_packed(dev)
        self.ms.append(self.s.timing()["total_ms"])


def one_run(s, ids, E, **kw):
    deg = degradation.Degradation(E, yearly_degrade=2.0)
    sw = degradation.DegradationSweep(lambda k, cap: scenarios.config4(ids, E=cap, only=[k], spec=True), POSITIONS, deg,
                                      builder=s)
    solver = Timed(s)
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = sw.run(solver, **kw)
    wall = time.perf_counter() - t
    upd = sw.device_deg.update_ms() if kw.get("timed") else None
    return dict(out=out, deg=deg, wall=wall, solve_ms=solver.ms, update_ms=upd)


def repeat(s, ids, E, reps, **kw):
    one_run(s, ids, E, **kw)  # warm-up: code objects, the allocator's blocks, the scenario series
    runs = [one_run(s, ids, E, **kw) for _ in range(reps)]
    for r in runs[:-1]:
        r["out"] = None  # (each holds every window's x on the host: only the last run's is compared)
    return runs


def line(name, runs, windows):
    w = np.array([r["wall"] for r in runs])
    sv = np.array([sum(r["solve_ms"]) for r in runs])
    print(f"  {name:34s} wall s {[round(float(v), 3) for v in w]} median {np.median(w):.3f} min {w.min():.3f} max "
          f"{w.max():.3f} = {windows / np.median(w):,.0f} windows/s end to end; solves {np.median(sv):.1f} ms summed "
          f"({np.median(sv) / len(POSITIONS):.2f} ms per position)", flush=True)
    return w


def same(a, b):
    bad = [f"{p['k']}:{f}" for p, q in zip(a["out"], b["out"]) for f in FIELDS if not np.array_equal(p[f], q[f])]
    for f in ("degrade_perc", "replacements", "skipped"):
        if not np.array_equal(getattr(a["deg"], f), getattr(b["deg"], f)):
            bad.append(f)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ok = True
    with BatchSolver(0) as s:
        for n in a.sizes:
            ids = list(range(n))
            E = scenarios.sweep_parameters(ids)["E"]
            windows = n * len(POSITIONS)
            print(f"{n} config-4 scenarios x {len(POSITIONS)} positions = {windows} windows, warm-up + {a.reps} repeats",
                  flush=True)
            host = repeat(s, ids, E, a.reps)
            wh = line("existing path (host wear update)", host, windows)
            res = repeat(s, ids, E, a.reps, resident=True, timed=True)
            wr = line("resident, x kept", res, windows)
            lean = repeat(s, ids, E, a.reps, resident=True, keep_x=False, timed=True)
            wl = line("resident, keep_x=False", lean, windows)
            r = res[int(np.argsort(wr)[len(wr) // 2])]
            u, sv = np.array(r["update_ms"]), np.array(r["solve_ms"])
            print(f"  update kernels (HIP events, the median resident run): {u.sum():.3f} ms summed, per position "
                  f"{[round(float(v), 3) for v in u]}; that position's solve {[round(float(v), 2) for v in sv]} ms: the "
                  f"update is {100 * u.sum() / sv.sum():.2f} % of the solves", flush=True)
            bad = same(host[-1], res[-1]) + same(host[-1], lean[-1])
            keep = bool(wr.max() < wh.min())
            xs = all(np.array_equal(p, q) for pa, pb in zip(host[-1]["out"], res[-1]["out"])
                     for p, q in zip(pa["x"], pb["x"]))
            print(f"  results equal (ene, iters, status, obj, degradation, capacity_before, final state): "
                  f"{'yes' if not bad else 'NO ' + str(bad[:8])}; x equal: {'yes' if xs else 'NO'}", flush=True)
            print(f"  keep-criterion (resident max {wr.max():.3f} s < existing min {wh.min():.3f} s): "
                  f"{'met' if keep else 'NOT met'}; speed-up of the medians {np.median(wh) / np.median(wr):.2f}x "
                  f"(keep_x=False {np.median(wh) / np.median(wl):.2f}x)", flush=True)
            ok = ok and keep and not bad and xs
            del host, res, lean
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
