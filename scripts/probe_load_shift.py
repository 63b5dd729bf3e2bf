#!/usr/bin/env python3
"""Controllable-load windows (scenarios.config4_load_shift: the config-4 population with a 150 kW / 4 h load-shifting
load, dervet MicrogridDER/LoadControllable.py) through the band kernel's load-shift form vs the default cascade: S
scenarios x 12 monthly windows (default S = 64: 768 windows), device-resident, the two paths interleaved in one run,
5 timed solves each after a warm-up of both.  Prints one JSON line: per path the best and the spread (max - min) of
its five walls, status counts, iteration counts, the kernels the windows landed on, and the largest relative objective
difference between the two paths' optimal windows; "speedup" = default best / load_shift best.

Usage: python scripts/probe_load_shift.py [S] [rated_power] [duration]
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
from dervet_hip.lp import builder, scenarios  # noqa: E402

PATHS = ("load_shift", "default")
REPEATS = 5


def main(argv):
    S = int(argv[0]) if argv else 64
    P = float(argv[1]) if len(argv) > 1 else 150.0
    Dh = float(argv[2]) if len(argv) > 2 else 4.0
    groups = scenarios.config4_load_shift(range(S), rated_power=P, duration=Dh)
    pb = builder.pack_groups(groups)
    d = np.asarray(pb.desc)
    out = {"windows": pb.count, "scenarios": S, "rated_power": P, "duration": Dh, "n_max": int(d[:, 0].max()),
           "m_max": int(d[:, 1].max())}
    dev = {p: pb.to_torch("cuda:0").alloc_outputs() for p in PATHS}  # (each path keeps its own outputs)
    s = BatchSolver(0)
    walls = {p: [] for p in PATHS}
    stats = {}
    for rep in range(REPEATS + 1):  # rep 0: the warm-up of both paths
        for p in PATHS:
            s.set_kernel_path(p)
            torch.cuda.synchronize()
            t = time.perf_counter()
            s.solve_packed(dev[p])
            torch.cuda.synchronize()
            if rep:
                walls[p].append(time.perf_counter() - t)
            stats[p] = s.kernel_stats()
    s.set_kernel_path("default")
    objs = {}
    for p in PATHS:
        ist = dev[p].istats.cpu().numpy()
        st = dev[p].stats.cpu().numpy().reshape(pb.count, 4)
        objs[p] = (ist[:, 0], st[:, 0])
        ms = 1e3 * np.array(walls[p])
        out[p] = {"ms_best": round(float(ms.min()), 3), "ms_spread": round(float(ms.max() - ms.min()), 3),
                  "ms_all": [round(float(v), 3) for v in ms], "windows_per_s": round(pb.count / (ms.min() * 1e-3)),
                  "optimal": int((ist[:, 0] == 0).sum()), "iters_mean": round(float(ist[:, 1].mean()), 1),
                  "iters_max": int(ist[:, 1].max()), "variant": stats[p]["variant"],
                  "paths": {k: v for k, v in stats[p].items() if k.endswith("_windows") and v}}
    both = (objs[PATHS[0]][0] == 0) & (objs[PATHS[1]][0] == 0)
    a, b_ = objs[PATHS[0]][1][both], objs[PATHS[1]][1][both]
    out["objective_rel_diff_max"] = float(np.max(np.abs(a - b_) / (1.0 + np.abs(b_)))) if both.any() else None
    out["speedup"] = round(out["default"]["ms_best"] / out["load_shift"]["ms_best"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
