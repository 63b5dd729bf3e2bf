#!/usr/bin/env python3
"""Electric-vehicle windows (scenarios.config4_ev: the config-4 population with a 50 kW / 200 kWh EV plugged 18 -> 7,
dervet MicrogridDER/ElectricVehicles.py) through the band kernel's load-shift form vs the default cascade: S scenarios
x 12 monthly windows (default S = 64: 768 windows), device-resident, the two paths interleaved in one run, 5 timed
solves each after a warm-up of both.  Then the two ways to get the batch into HBM, 5 times each, interleaved: the host
builder + pack + upload against the device builder from its compact inputs (spec + upload + expansion).  Prints one
JSON line: per path the best and the spread (max - min) of its five walls, status counts, iteration counts, the
kernels the windows landed on, the largest relative objective difference between the two paths' optimal windows;
"speedup" = default best / load_shift best; "build" the two builders' walls and their ratio.

Usage: python scripts/probe_ev.py [S] [ch_max] [ene_target]
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
from dervet_hip.lp import builder, gpu_builder, scenarios  # noqa: E402

PATHS = ("load_shift", "default")
REPEATS = 5


def main(argv):
    S = int(argv[0]) if argv else 64
    chm = float(argv[1]) if len(argv) > 1 else 50.0
    tgt = float(argv[2]) if len(argv) > 2 else 200.0
    make = lambda spec: scenarios.config4_ev(range(S), ch_max=chm, ene_target=tgt, spec=spec)  # noqa: E731
    pb = builder.pack_groups(make(False))
    d = np.asarray(pb.desc)
    out = {"windows": pb.count, "scenarios": S, "ch_max": chm, "ene_target": tgt, "n_max": int(d[:, 0].max()),
           "m_max": int(d[:, 1].max()), "start_rows_max": int((d[:, 2] - 2 * (d[:, 0] // 5) - 1).max())}
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

    # ---- the batch into HBM: host builder + upload vs device builder (series generation is common to both and inside)
    def host_way():
        return builder.pack_groups(make(False)).to_torch("cuda:0")

    def device_way():
        return gpu_builder.pack_specs_device(make(True), s)

    ways = {"host_builder_upload": host_way, "device_builder": device_way}
    bw = {k: [] for k in ways}
    for rep in range(REPEATS + 1):
        for k, f in ways.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = f()
            torch.cuda.synchronize()
            if rep:
                bw[k].append(time.perf_counter() - t)
            if rep == 0 and k == "device_builder":
                out["device_built_equals_host_built"] = all(
                    bool(torch.equal(getattr(got, f_), getattr(dev["default"], f_)))
                    for f_ in ("desc", "indptr", "indices", "data", "c", "c0", "q", "l", "u"))
            del got
    out["build"] = {k: {"ms_best": round(1e3 * min(v), 2), "ms_spread": round(1e3 * (max(v) - min(v)), 2)}
                    for k, v in bw.items()}
    out["build"]["upload_bytes_host_way"] = int(sum(getattr(pb, f).nbytes for f in
                                                    ("desc", "indptr", "indices", "data", "c", "c0", "q", "l", "u")))
    out["build"]["ratio"] = round(out["build"]["host_builder_upload"]["ms_best"] /
                                  out["build"]["device_builder"]["ms_best"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
