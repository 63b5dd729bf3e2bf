"""Timing probe of the economic sizing (dervet_hip.size_for_value: dvh_solve_packed_device + dvh_value_cuts +
dvh_value_master per round) on the reference's Usecase 1 `es` case (tests/golden/uc1_sizing.*):
  (a) the case as the reference demands it, one year window (T = 8,760, the chain tier): rounds, PDHG iterations,
      the sizes and the objective gap to the golden total, with 1 and 4 candidates per round;
  (b) a sweep of seeded load scales (lognormal, sigma 0.2) with twelve monthly windows each, 4 candidates per round;
  (c) the CPU restatement (value_sizing.loop_host: HiGHS window duals, HiGHS master) on (a) and on the first
      `--cpu-cases` cases of (b).
Per run: wall time, the solves' HIP-event time (dvh_last_timing summed over the rounds; the wall time beyond it is the
device builder, the cut and master kernels and the host's part of a round), and the host waits per round
(dvh_last_host_syncs of the round's solve + the flag read-back).
No time here is a pass / fail bar.

Usage: python scripts/probe_value_sizing.py [--cases 256] [--cpu-cases 2] [--seed 7]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "der-vet_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import value_sizing_cases as C  # noqa: E402
import value_sizing_ref as R  # noqa: E402
from dervet_hip import BatchSolver, size_for_value  # noqa: E402
from dervet_hip import value_sizing as VS  # noqa: E402


class Timed:
    """The solver with its solves' HIP-event times summed."""

    def __init__(self, solver):
        self.s, self.solve_ms = solver, 0.0
        self._solve = solver.solve_packed

    def __enter__(self):
        s = self.s

        def solve(pb, *a, **k):
            r = self._solve(pb, *a, **k)
            self.solve_ms += s.timing()["total_ms"]
            return r
        s.solve_packed = solve
        return self

    def __exit__(self, *a):
        self.s.solve_packed = self._solve


def run_gpu(tag, positions, specs, solver):
    log = []
    with Timed(solver) as t:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = size_for_value(positions, specs, solver, log=log)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    st = [r.status_name for r in res]
    rounds = len(log) + 1   # (+ the final solve at the rounded sizes)
    syncs = [e["solve_host_syncs"] for e in log]
    print(f"[{tag}] GPU: {len(specs)} case(s) x {len(positions)} window(s), C = {specs[0].candidates}: wall {wall * 1e3:.1f} ms, "
          f"solves {t.solve_ms:.1f} ms (HIP events), {rounds} batched solves, windows per round "
          f"{[e['windows'] for e in log][:6]}{'..' if len(log) > 6 else ''}, host waits per round: solve {syncs[:4]} + 1 flag read-back; "
          f"statuses { {s: st.count(s) for s in set(st)} } (window statuses of the failed: {[r.lp_status for r in res if r.status == VS.LP_FAILED]}), case rounds {min(r.rounds for r in res)} .. {max(r.rounds for r in res)}, "
          f"PDHG iterations {sum(r.lp_iters for r in res)}")
    return res, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=256)
    ap.add_argument("--cpu-cases", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    print("device", torch.cuda.get_device_name(0))
    with BatchSolver(0) as solver:
        # ---- (a) the golden case, one year window
        for cand in (1, 4):
            positions, specs, meta = C.uc1("es", candidates=cand)
            g = meta["golden_objective"]
            total = sum(g.values())
            run_gpu(f"a C={cand} warm-up", positions, specs, solver)
            res, wall = run_gpu(f"a C={cand}", positions, specs, solver)
            r = res[0]
            print(f"[a C={cand}] sizes {r.energy:.0f} kWh / {r.power:.0f} kW (relaxed {r.energy_lp:.3f} / {r.power_lp:.3f}; golden "
                  f"{meta['golden_size']['Energy Rating (kWh)']:.0f} / {meta['golden_size']['Discharge Rating (kW)']:.0f}), "
                  f"lower {r.lower!r} upper {r.upper!r} objective at the rounded size {r.objective!r}, golden total {total!r}: "
                  f"relative gap {(r.objective - total) / total:.3e}; rounds {r.rounds}, cuts {r.n_cuts}, iterations {r.lp_iters}")
        # ---- (c) on (a)
        positions, specs, meta = C.uc1("es", candidates=4)
        t0 = time.perf_counter()
        rc = VS.loop_host(R.evaluate_highs(positions, 0), specs[0])
        print(f"[c on a] CPU restatement (HiGHS duals, C = 4): wall {time.perf_counter() - t0:.1f} s, rounds {rc.rounds}, cuts {rc.n_cuts}, "
              f"sizes {rc.energy:.0f} / {rc.power:.0f}, lower {rc.lower!r} upper {rc.upper!r}")
        # ---- (b) the sweep
        rng = np.random.default_rng(a.seed)
        scales = np.exp(0.2 * rng.standard_normal(a.cases))
        positions, specs, _ = C.uc1("es", candidates=4, monthly=True, scales=scales)
        run_gpu("b warm-up", positions, specs, solver)
        res, wall = run_gpu("b", positions, specs, solver)
        E = np.array([r.energy for r in res])
        P = np.array([r.power for r in res])
        print(f"[b] sizes: energy {np.nanmin(E):.0f} .. {np.nanmax(E):.0f} kWh, power {np.nanmin(P):.0f} .. {np.nanmax(P):.0f} kW; "
              f"{wall * 1e3 / a.cases:.2f} ms per case")
        # ---- (c) on the first cases of (b)
        for k in range(min(a.cpu_cases, a.cases)):
            t0 = time.perf_counter()
            rc = VS.loop_host(R.evaluate_highs(positions, k), specs[k])
            dt = time.perf_counter() - t0
            m = R.monolithic(positions, k, specs[k])
            print(f"[c on b, case {k}] CPU restatement: wall {dt:.1f} s, rounds {rc.rounds}, sizes {rc.energy:.0f} / {rc.power:.0f} "
                  f"(GPU {res[k].energy:.0f} / {res[k].power:.0f}); monolithic HiGHS optimum {m['obj']!r}: GPU upper - opt "
                  f"{(res[k].upper - m['obj']) / (1 + abs(m['obj'])):.3e}, lower - opt {(res[k].lower - m['obj']) / (1 + abs(m['obj'])):.3e} (relative)")


if __name__ == "__main__":
    main()
