"""Wave 0 of the three-step band form's plain iteration: its dual half-step reads the next lane's ene, the tau x-bar and
the init row's ene_0 directly behind the first barrier, and the init row (row 0, ene_0 = target, held by lane 63 of
wave 0) is updated from that early read without a wait of its own.  The arithmetic and its order per value are the
parent's, so everything here is either a bar against the host restatement (oracle/pdlp_ref.py: iterations within 128,
objective within 1e-7 relative, as tests/test_gpu_band_loop.py), the result contract recomputed from the returned x, y
(tests/result_contract.py, tests/kkt_ref.py; reference optimum: HiGHS), or bit-for-bit equality of the static
single-demand-period instantiation with the forced generic one (DVH_BAND_J1=0, as tests/test_gpu_band_j1.py).

Every window (tests/band_cases.py: window, WAVE0_SEEDS) has a non-zero soc_target and llsoc, so the init row's dual is
non-zero at the optimum; that is asserted on the reference, otherwise nothing here would be about that row.  Step counts, all J = 1 on the forced "band3" path:
T = 2, 3, 4 (the init row and the end row one or two steps apart inside one lane), 192 / 193 (wave 0's last lane against
wave 1's first: the XE / YS hand-over next to the init lane), 576 / 577 (the last wave holds no step, then one),
766, 767, 768 (lane 63 of the last wave holds real steps).
"""
import numpy as np
import pytest

import band_cases as bc
import result_contract as rc
from oracle import pdlp_ref

pytestmark = pytest.mark.gpu

STATIC = bc.STATIC  # kernel_stats()["band_variant"]
SEEDS = bc.WAVE0_SEEDS
STEPS = tuple(SEEDS)
PERIODS = (1, 2, 64)
LIMITS = (1, 63, 65)


@pytest.fixture(scope="module")
def solver():
    yield from bc.open_solver()


@pytest.fixture(scope="module")
def windows():
    return {T: bc.case_window((T, 1, SEEDS[T])) for T in STEPS}


@pytest.fixture(scope="module")
def refs(windows):
    """The oracle dict, pdlp_ref at check period 64 and the HiGHS optimum of every window, computed once a session."""
    return {T: (bc.oracle_lp(lp), bc.reference((T, 1, SEEDS[T]))[0], bc.optimum((T, 1, SEEDS[T])))
            for T, lp in windows.items()}


@pytest.mark.parametrize("T", STEPS)
def test_against_the_host_restatement(solver, windows, refs, T):
    """The static instantiation against oracle/pdlp_ref.py, and the result contract on the returned x, y."""
    olp, ref, opt = refs[T]
    assert ref["y"][0] != 0.0, f"T {T}: the reference's init-row dual is zero"
    r = bc.solve(solver, [windows[T]], band_variant=STATIC)[0]
    bc.agrees(r, ref, 64, f"T {T}")
    assert r.y[0] != 0.0, f"T {T}: init-row dual is zero"
    rc.check_both(olp, r, opt, f"T {T}", "band3_J1")


@pytest.mark.parametrize("ce", PERIODS)
@pytest.mark.parametrize("T", STEPS)
def test_static_equals_generic(solver, windows, T, ce):
    """Iteration limits below, off and at the period (a loop entered and left every iteration at period 1), static
    against forced generic, bit for bit."""
    for mi in LIMITS:
        a, b = bc.both(solver, [windows[T]], check_every=ce, max_iters=mi)
        bc.same(a[0], b[0], f"T {T} check_every {ce} max_iters {mi}")
        assert a[0].iters <= mi


def test_warm_start_with_a_nonzero_init_row_dual(solver, windows, refs):
    """A window started from its neighbour's solution (3 % less load), whose init-row dual is non-zero."""
    _, ra, _ = refs[193]
    assert ra["y"][0] != 0.0
    nb = bc.case_window(bc.neighbour((193, 1, SEEDS[193])))
    ref = pdlp_ref.solve(bc.oracle_lp(nb), dict(check_every=64, kkt_every=1, x0=ra["x"], y0=ra["y"]))
    a, b = bc.both(solver, [nb], start=[(ra["x"], ra["y"])], warm_start=1)
    bc.same(a[0], b[0], "T 193 warm")
    bc.agrees(a[0], ref, 64, "T 193 warm")


def test_restarts(solver, windows):
    """Check period 4: the window restarts several times (the reference's trace: the iterations since the last restart
    fall back), the bars hold, and the two instantiations agree bit for bit."""
    lp = windows[193]
    ref, trace = bc.reference((193, 1, SEEDS[193]), 4)
    restarts = bc.restarts(trace)
    print(f"reference: {ref['iters']} iterations, {restarts} restarts")
    assert restarts >= 4, restarts
    a, b = bc.both(solver, [lp], check_every=4)
    bc.same(a[0], b[0], "T 193 check_every 4")
    bc.agrees(a[0], ref, 4, "T 193 check_every 4")


def test_no_state_survives_a_window(solver):
    """1,100 cheap windows, T = 2 and T = 200 alternating with different soc_target, so that every persistent workgroup
    takes several: every window equals its solo solve bit for bit."""
    base = [bc.window(2 if k % 2 == 0 else 200, 1, 9100 + k)[0] for k in range(10)]
    solo = [bc.solve(solver, [lp], band_variant=STATIC)[0] for lp in base]
    res = bc.solve(solver, [base[i % 10] for i in range(1100)], band_variant=STATIC)
    for i, r in enumerate(res):
        f = solo[i % 10]
        assert r.status == f.status == 0 and r.iters == f.iters, (i, r.status, r.iters, f.status, f.iters)
        assert np.array_equal(r.x, f.x) and np.array_equal(r.y, f.y), f"copy {i} of window {i % 10} differs from its solo solve"
