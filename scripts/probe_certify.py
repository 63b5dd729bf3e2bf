#!/usr/bin/env python3
"""The certificate pass (csrc/dvh_certify.hip, dvh_options.certify) on a sweep with infeasible windows: 768 monthly POI
windows (builder.battery_group, T = 744, one demand period) of which 77 are made infeasible -- an overloaded step, a
month short of energy under the import limit, a minimum SOE the charger cannot reach, in turn.  Per kernel path
(default, interconnect): wall of the solve with certify 0, 1 and 2 (five timed repeats after a warm-up: fastest,
median, slowest), statuses, the pass's own time (HIP events) and counts, the in-kernel certificates of level 2; then
the screen (BatchSolver.certify) over the same windows and the histogram of its certificate-iteration counts.  With
DVH_LIB naming an earlier build of the library only the levels it knows run (none: certify = 0; no
dvh_last_certify_early: 0 and 1) and the screen is left out: the parent commit's times for the same batch, to be
taken in the same job.  [infeasible] = 0 gives the all-feasible sweep.

Usage: python scripts/probe_certify.py [windows] [infeasible]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "der-vet_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dervet_hip import BatchSolver  # noqa: E402
from dervet_hip.lp import builder  # noqa: E402

BAT = dict(E=2000.0, Pch=500.0, Pdis=500.0, rte=0.9, sdr=0.0, soc_target=0.5, ulsoc=1.0, llsoc=0.1, fixedOM=1.0,
           OMexpenses=0.0, hp=0.0)
POI = dict(max_import=-650.0, max_export=0.0)


def group(G, bad, T=744):
    rng = np.random.default_rng(20250217)
    load = rng.uniform(400.0, 600.0, (G, T))
    emin = np.zeros((G, T))
    kinds = {}
    for i, k in enumerate(np.linspace(0, G - 1, bad).astype(int)):
        kind = ("overload", "short", "min_soe")[i % 3]
        kinds[int(k)] = kind
        if kind == "overload":
            load[k, T // 2] = 650.0 + 500.0 + 150.0
        elif kind == "short":
            load[k] = rng.uniform(660.0, 700.0, T)
        else:
            emin[k, 1] = 1000.0 + 0.9 * 500.0 + 150.0
    g = builder.battery_group(T, 1.0, load, BAT, retail_price=rng.uniform(0.05, 0.15, (G, T)),
                              demand_masks=np.ones((1, T), bool), demand_prices=rng.uniform(8.0, 20.0, (G, 1)),
                              ene_min=emin, poi=POI)
    return g, kinds


def main(argv):
    G = int(argv[0]) if argv else 768
    bad = int(argv[1]) if len(argv) > 1 else 77
    g, kinds = group(G, bad)
    pb = builder.pack_groups([g])
    dev = pb.to_torch("cuda:0").alloc_outputs()
    s = BatchSolver(0)
    has_pass = hasattr(s._lib, "dvh_certify_batch") and hasattr(s._opts, "certify")
    has_early = has_pass and hasattr(s._lib, "dvh_last_certify_early")
    levels = (0, 1, 2) if has_early else (0, 1) if has_pass else (0,)
    print(json.dumps({"windows": pb.count, "infeasible": len(kinds), "n": g.n, "m": g.m,
                      "library": os.environ.get("DVH_LIB", "in-tree"), "certificate_pass": has_pass,
                      "levels": levels}), flush=True)
    for path in ("default", "interconnect"):
        s.set_kernel_path(path)
        for certify in levels:
            if has_pass:
                s.set_options(certify=certify)
            s.solve_packed(dev)
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t = time.perf_counter()
                s.solve_packed(dev)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            ist = dev.istats.cpu().numpy()
            ts.sort()
            out = {"path": path, "certify": certify, "ms": round(1e3 * ts[0], 2), "ms_median": round(1e3 * ts[2], 2),
                   "ms_max": round(1e3 * ts[-1], 2), "gpu_ms": s.timing(),
                   "status_counts": {int(k): int(v) for k, v in zip(*np.unique(ist[:, 0], return_counts=True))},
                   "bad_status_counts": {int(k): int(v) for k, v in
                                         zip(*np.unique(ist[np.array(sorted(kinds), int), 0], return_counts=True))},
                   "iters_max": int(ist[:, 1].max()), "host_syncs": s.host_syncs()}
            if has_pass:
                out["pass"] = s.certify_stats()
            print(json.dumps(out), flush=True)
    s.set_kernel_path("default")
    if has_pass and not os.environ.get("DVH_LIB"):
        lps = builder.group_window_lps(g)
        t = time.perf_counter()
        res = s.certify(lps)
        wall = time.perf_counter() - t
        it = np.array([r.iters for r in res if r.status in (1, 2)])
        edges = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
        hist = {f"<={e}": int(((it <= e) & (it > (edges[i - 1] if i else 0))).sum()) for i, e in enumerate(edges)}
        st = {int(k): int(v) for k, v in zip(*np.unique([r.status for r in res], return_counts=True))}
        wrong = [k for k, r in enumerate(res) if (r.status == 1) != (k in kinds)]
        print(json.dumps({"screen": {"wall_ms": round(1e3 * wall, 1), "status_counts": st, "pass": s.certify_stats(),
                                     "certificate_iterations": hist, "mismatch_with_construction": wrong}}), flush=True)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
