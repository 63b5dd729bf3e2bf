"""Timing probe of reliability sizing (dervet_hip.reliability.size_for_reliability, dvh_size_reliability) against the
CPU restatement of the reference's loop (tests/sizing_ref.py: HiGHS + the oracle's Python outage simulation).

Two workloads: the reference's golden no-shedding case alone, and a sweep of `--cases` cases -- the golden critical
load x a seeded lognormal scale, targets of 2-8 h.  The library call is warmed once and timed `--reps` times (host
clock around the blocking call, plus the call's own HIP-event split); the CPU loop runs once over the first
`--cpu-cases` sweep cases (it is serial Python: its time per case is what is reported).  Prints rounds and PDHG
iterations per round, and checks that both give the same sizes.

Usage: python scripts/probe_sizing.py [--cases 256] [--cpu-cases 256] [--reps 3]
"""
import argparse
import os
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "der-vet_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import sizing_ref  # noqa: E402
from dervet_hip import BatchSolver, reliability  # noqa: E402


def sweep(n, seed=2024):
    case, spec, _ = sizing_ref.golden_cases()["wo_ls1"]
    rng = np.random.default_rng(seed)
    scale = rng.lognormal(0.0, 0.25, n)
    hours = rng.integers(2, 9, n)
    cases = [replace(case, critical_load=(np.asarray(case.critical_load) * s).round(5)) for s in scale]
    specs = [replace(spec, target_hours=float(h)) for h in hours]
    return cases, specs


def time_gpu(solver, cases, specs, reps):
    reliability.size_for_reliability(cases, specs, solver)  # warm-up: code objects, buffers
    walls, parts = [], []
    for _ in range(reps):
        t = time.perf_counter()
        res = reliability.size_for_reliability(cases, specs, solver)
        walls.append(1e3 * (time.perf_counter() - t))
        parts.append(reliability.last_sizing_ms(solver))
    i = int(np.argsort(walls)[len(walls) // 2])
    return res, walls, parts[i]


def report(name, solver, cases, specs, reps, cpu_cases):
    res, walls, part = time_gpu(solver, cases, specs, reps)
    rounds = np.array([r.rounds for r in res])
    iters = np.array([r.lp_iters for r in res])
    status = {s: sum(r.status == s for r in res) for s in sorted({r.status for r in res})}
    print(f"{name}: {len(cases)} cases, library call wall ms {[round(w, 2) for w in walls]} (median "
          f"{np.median(walls):.2f}); HIP events of the median call: total {part['total_ms']:.2f} ms, LP builds + solves "
          f"{part['lp_ms']:.2f} ms, scans {part['scan_ms']:.3f} ms, {part['rounds']} case-rounds")
    print(f"  status {status}; rounds per case min / mean / max {rounds.min()} / {rounds.mean():.2f} / {rounds.max()}; "
          f"PDHG iterations per round min / mean / max {(iters / rounds).min():.0f} / {(iters.sum() / rounds.sum()):.0f} "
          f"/ {(iters / rounds).max():.0f}")
    m = min(cpu_cases, len(cases))
    t = time.perf_counter()
    refs = [sizing_ref.size_for_reliability(c, s) for c, s in zip(cases[:m], specs[:m])]
    cpu = time.perf_counter() - t
    same = sum((r.energy, r.power, r.status, r.rounds) == (g.energy, g.power, g.status, g.rounds)
               for r, g in zip(refs, res))
    near = sum(sizing_ref.near_integer(r, s) for r, s in zip(refs, specs))
    print(f"  CPU loop (HiGHS + Python simulation), {m} cases: {cpu:.2f} s = {1e3 * cpu / m:.1f} ms per case; "
          f"same size, status and rounds as the library on {same} of {m} ({near} with an LP optimum within 1e-3 above "
          f"an integer)")
    print(f"  per case: library {np.median(walls) / len(cases):.3f} ms, CPU loop {1e3 * cpu / m:.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=256)
    ap.add_argument("--cpu-cases", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    case, spec, _ = sizing_ref.golden_cases()["wo_ls1"]
    with BatchSolver(0) as s:
        report("golden wo_ls1", s, [case], [spec], a.reps, 1)
        cases, specs = sweep(a.cases)
        report("sweep", s, cases, specs, a.reps, a.cpu_cases)


if __name__ == "__main__":
    main()
