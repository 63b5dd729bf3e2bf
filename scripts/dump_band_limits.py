#!/usr/bin/env python3
"""Digests of the three-step band form's results at iteration limits around the check period, for a bit-for-bit bar
across kernel changes that only move work (tests/test_gpu_band_reads.py).

The windows are those of tests/test_gpu_band_wave0.py (J = 1, non-zero soc_target and llsoc, forced "band3") at
T = 3, 193, 577, 768.  Each is solved at (check_every, max_iters) = (64,1) (64,2) (64,63) (64,64) (64,65) (64,129) (1,3)
(2,5) -- a loop left before, at and behind a check, and loops of one and no plain iteration -- cold, and from a carried
start: the window's neighbour (3 % more load) started from the window's own converged cold solution (warm_start 1).
Per case the SHA-256 of the returned x || y bytes with iterations and status; per T the digest of the LP's arrays and of
the carried start, so that a differing window or start is told from a differing kernel.

Run it with the library of the commit the bar refers to (DVH_LIB, or the default build of a checkout of that commit):
    [DVH_LIB=...] python scripts/dump_band_limits.py [OUT.json]      (default tests/golden/band_limits_parent.json)
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "der-vet_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

STEPS = (3, 193, 577, 768)
LIMITS = ((64, 1), (64, 2), (64, 63), (64, 64), (64, 65), (64, 129), (1, 3), (2, 5))
STATIC = 9002054  # kernel_stats()["band_variant"] of the single-demand-period instantiation


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def lp_digest(lp):
    return sha(lp.indptr, lp.indices, lp.data, lp.q, lp.c, lp.l, lp.u)


def windows():
    """{T: (window, neighbour)}"""
    from test_gpu_band_wave0 import SEEDS, _window
    return {T: (_window(T, 1, SEEDS[T])[0], _window(T, 1, SEEDS[T], load_scale=1.03)[0]) for T in STEPS}


def solve(s, lp, start=None, **options):
    opts = dict(check_every=64, kkt_every=1, kkt_predict=0, max_iters=100000, warm_start=0 if start is None else 1)
    opts.update(options)
    s.set_options(**opts)
    s.set_kernel_path("band3")
    r = s.solve([lp], start=start)[0]
    st = s.kernel_stats()
    assert st["band_windows"] == 1 and st["band_variant"] == STATIC, st
    return r


def digests(s, wins):
    """The record of every case with the library the solver s has loaded."""
    out = {}
    for T, (lp, nb) in wins.items():
        full = solve(s, lp)
        assert full.status == 0, (T, full.status_name)
        rec = dict(lp=lp_digest(lp), neighbour=lp_digest(nb), start=sha(full.x, full.y), start_iters=int(full.iters),
                   cases={})
        for ce, mi in LIMITS:
            for kind, r in (("cold", solve(s, lp, check_every=ce, max_iters=mi)),
                            ("carried", solve(s, nb, start=[(full.x, full.y)], check_every=ce, max_iters=mi))):
                rec["cases"][f"{kind} check_every {ce} max_iters {mi}"] = dict(
                    sha256=sha(r.x, r.y), iters=int(r.iters), status=int(r.status))
        out[str(T)] = rec
    return out


if __name__ == "__main__":
    from dervet_hip import BatchSolver
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "band_limits_parent.json")
    with BatchSolver(0) as s:
        rec = digests(s, windows())
    with open(dst, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(len(v["cases"]) for v in rec.values())
    print(f"{n} cases -> {dst} ({os.path.getsize(dst)} bytes)")
