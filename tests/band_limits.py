"""Digests of the three-step band form's results at iteration limits around the check period, for a bit-for-bit bar
across kernel changes that only move work (tests/test_gpu_band_reads.py; scripts/dump_band_limits.py writes the record).

The windows are band_cases' wave0 windows (J = 1, non-zero soc_target and llsoc, forced "band3") at T = 3, 193, 577, 768.
Each is solved at (check_every, max_iters) = (64,1) (64,2) (64,63) (64,64) (64,65) (64,129) (1,3) (2,5) -- a loop left
before, at and behind a check, and loops of one and no plain iteration -- cold, and from a carried start: the window's
neighbour (3 % more load) started from the window's own converged cold solution (warm_start 1).  Per case the SHA-256 of
the returned x || y bytes with iterations and status; per T the digest of the LP's arrays and of the carried start, so
that a differing window or start is told from a differing kernel.
"""
import hashlib

import numpy as np

import band_cases as bc

STEPS = (3, 193, 577, 768)
LIMITS = ((64, 1), (64, 2), (64, 63), (64, 64), (64, 65), (64, 129), (1, 3), (2, 5))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def lp_digest(lp):
    return sha(lp.indptr, lp.indices, lp.data, lp.q, lp.c, lp.l, lp.u)


def windows():
    """{T: (window, neighbour)}"""
    cases = {T: (T, 1, bc.WAVE0_SEEDS[T]) for T in STEPS}
    return {T: (bc.case_window(c), bc.case_window(bc.neighbour(c))) for T, c in cases.items()}


def solve(s, lp, start=None, **options):
    options.setdefault("warm_start", 0 if start is None else 1)
    return bc.solve(s, [lp], band_variant=bc.STATIC, start=start, **options)[0]


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
