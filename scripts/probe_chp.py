#!/usr/bin/env python3
"""Combined-heat-and-power windows (scenarios.config4_chp: the config-4 population with a 300 kW unit and the site's
steam / hot-water loads, dervet MicrogridDER/CombinedHeatPower.py) through the band kernel's heat form vs the default
cascade: S scenarios x 12 monthly windows (default S = 64: 768 windows), device-resident, the two paths interleaved in
one run, REPEATS timed solves each (default 5) after a warm-up of both.  A monthly window has n = 7 T + J > 4096, so the
default cascade solves these windows one at a time on its grid-wide path (minutes for the whole run: every solve is
reported as it ends, a "#" line).  Prints one JSON line: per path every wall, the
best and the spread (max - min), status counts, iteration counts, the kernels the windows landed on, and the largest
relative objective difference between the two paths' optimal windows; "speedup" = default best / chp best,
"faster_in_every_repeat" = the form's wall below the default's in each of the interleaved repeats.

Usage: python scripts/probe_chp.py [S] [REPEATS]
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

PATHS = ("chp", "default")


def main(argv):
    S = int(argv[0]) if argv else 64
    repeats = int(argv[1]) if len(argv) > 1 else 5
    groups = scenarios.config4_chp(range(S))
    pb = builder.pack_groups(groups)
    d = np.asarray(pb.desc)
    out = {"windows": pb.count, "scenarios": S, "repeats": repeats, "n_max": int(d[:, 0].max()), "m_max": int(d[:, 1].max())}
    dev = {p: pb.to_torch("cuda:0").alloc_outputs() for p in PATHS}  # (each path keeps its own outputs)
    s = BatchSolver(0)
    walls = {p: [] for p in PATHS}
    stats = {}
    for rep in range(repeats + 1):  # rep 0: the warm-up of both paths
        for p in PATHS:
            s.set_kernel_path(p)
            torch.cuda.synchronize()
            t = time.perf_counter()
            s.solve_packed(dev[p])
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
            if rep:
                walls[p].append(wall)
            stats[p] = s.kernel_stats()
            print(f"# rep {rep} ({'timed' if rep else 'warm-up'}) {p}: {1e3 * wall:.3f} ms", flush=True)  # (progress)
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
    out["speedup"] = round(out["default"]["ms_best"] / out["chp"]["ms_best"], 2)
    out["faster_in_every_repeat"] = bool(np.all(np.array(walls["chp"]) < np.array(walls["default"])))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
