#!/usr/bin/env python3
"""Record the three-step band form's results at iteration limits around the check period (tests/band_limits.py says
which windows and cases, and what is recorded), for the bit-for-bit bar of tests/test_gpu_band_reads.py.

Run it with the library of the commit the bar refers to (DVH_LIB, or the default build of a checkout of that commit):
    [DVH_LIB=...] python scripts/dump_band_limits.py [OUT.json]      (default tests/golden/band_limits_parent.json)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "der-vet_amd"), os.path.join(ROOT, "tests")]
import band_limits  # noqa: E402

if __name__ == "__main__":
    from dervet_hip import BatchSolver
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "band_limits_parent.json")
    with BatchSolver(0) as s:
        rec = band_limits.digests(s, band_limits.windows())
    with open(dst, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(len(v["cases"]) for v in rec.values())
    print(f"{n} cases -> {dst} ({os.path.getsize(dst)} bytes)")
