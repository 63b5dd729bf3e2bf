"""The band kernel's solve loop: plain iterations run in an inner loop of their own between two checks, so the
iteration counter, the check counter and the iteration limit must come out exactly as before -- for every check
period, for limits below, at and off a multiple of the period, for both wave kinds (the wave with the tau column and
the others), and with no state carried from one window of a persistent workgroup to the next.

Both battery forms run ("band3": three steps per lane, persistent grid; "band1": one step per lane) on battery + DCM
windows built as in test_gpu_configs.test_band_kernel_forms_agree (tests/band_cases.py: window, LOOP_WINDOWS).
Step counts: T = 2 (degenerate), 25 (padding
steps inside a lane), 200 (two waves of the three-step form hold steps, so both loop variants do real work), 600 (all
four waves); J = 0, 1 and 4 demand periods on the T = 200 window (no tau column / the straight-line tau path / the
per-column loop).  The reference is the numpy restatement of the algorithm (oracle/pdlp_ref.py) with the same options;
the bars against it are those of test_gpu_parity.test_iterates_match_host_restatement: iterations within 128,
objective within 1e-7 relative.
"""
import numpy as np
import pytest

import band_cases as bc
from oracle import pdlp_ref

pytestmark = pytest.mark.gpu

PATHS = (("band3", bc.GENERIC), ("band1", bc.ONE_STEP))
PERIODS = (1, 2, 3, 64, 100)
LIMITS = bc.LIMITS
ITER_LIMIT = 3


@pytest.fixture(scope="module")
def solver():
    yield from bc.open_solver()


@pytest.mark.parametrize("path,variant", PATHS)
def test_iteration_limit(solver, path, variant):
    """max_iters below, at and just past one and two check periods: the loop of plain iterations stops at the limit,
    not at the period, and the count comes back exact (as oracle/pdlp_ref.solve with the same options)."""
    lp = bc.case_window(bc.HARD)
    for mi in LIMITS:
        r = bc.solve(solver, [lp], path, variant, max_iters=mi)[0]
        print(f"{path} max_iters {mi}: status {r.status}, iters {r.iters}")
        assert r.status == ITER_LIMIT, f"{path} max_iters {mi}: {r.status_name}"
        assert r.iters == mi, f"{path} max_iters {mi}: {r.iters} iterations"


@pytest.mark.parametrize("path,variant", PATHS)
@pytest.mark.parametrize("ce", PERIODS)
def test_check_period(solver, path, variant, ce):
    """Every window of bc.LOOP_WINDOWS in one batch; pdlp_ref at the same period is shared by the two forms."""
    names = list(bc.LOOP_WINDOWS)
    res = bc.solve(solver, [bc.case_window(bc.LOOP_WINDOWS[k]) for k in names], path, variant, check_every=ce)
    for name, r in zip(names, res):
        bc.agrees(r, bc.reference(bc.LOOP_WINDOWS[name], ce)[0], ce, f"{path} check_every {ce} {name}")


def test_reproducible_and_order_free(solver):
    """1,100 windows on the persistent form -- 11 distinct T = 48 windows, 100 copies each, interleaved -- so that every
    workgroup slot takes at least two windows: every copy of a window is bit-identical in x, y, status and iterations
    (no loop state survives from one window to the next)."""
    base = [bc.window(48, 1 + (k % 2), 4800 + k)[0] for k in range(11)]
    lps = [base[i % 11] for i in range(1100)]
    res = bc.solve(solver, lps)
    for i, r in enumerate(res):
        f = res[i % 11]
        assert r.status == f.status == 0 and r.iters == f.iters, (i, r.status, r.iters, f.status, f.iters)
        assert np.array_equal(r.x, f.x) and np.array_equal(r.y, f.y), f"copy {i} of window {i % 11} differs"


@pytest.fixture(scope="module")
def warm_case():
    """(window, its neighbour's reference solution, the reference's warm solve from it), computed once."""
    a, b = bc.WARM_PAIR
    ra = bc.reference(a)[0]
    assert ra["status"] == 0
    b = bc.case_window(b)
    return b, ra, pdlp_ref.solve(bc.oracle_lp(b), dict(check_every=64, kkt_every=1, x0=ra["x"], y0=ra["y"]))


@pytest.mark.parametrize("path,variant", PATHS)
def test_warm_start(solver, warm_case, path, variant):
    """A window started from its neighbour's solution (warm_start = 1): the check-period assertions at period 64."""
    b, ra, ref = warm_case
    r = bc.solve(solver, [b], path, variant, start=[(ra["x"], ra["y"])], warm_start=1)[0]
    bc.agrees(r, ref, 64, f"{path} warm start")
