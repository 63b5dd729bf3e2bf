"""The band kernel's single-demand-period instantiation (three-step battery form, J a compile-time 1): the host
launches it for a batch without a J != 1 battery window, DVH_BAND_J1=0 keeps the generic instantiation (J read from the
descriptor), and both compute the same thing -- the static one only drops what J == 1 never uses (the tau update and the
init row on the waves without the tau column, the per-step period index, two of three XT reads).

Windows are built by band_cases.window (tests/band_cases.py: J1_SEEDS).  Statuses, iteration counts, the four
statistics, x and y are compared bit for bit: the arithmetic and its order are those of the generic instantiation's J == 1 path.

The defensive check (a J != 1 window handed to the static instantiation leaves through bail()) has no case here: the
host counts the J != 1 windows itself and no test hook launches the static instantiation over a list that has one.
"""
import numpy as np
import pytest

import band_cases as bc

pytestmark = pytest.mark.gpu

GENERIC, STATIC = bc.GENERIC, bc.STATIC  # kernel_stats()["band_variant"]; ["variant"] stays the form's code
SEEDS = bc.J1_SEEDS
STEPS = tuple(SEEDS)
PERIODS = (1, 3, 64)
LIMITS = (1, 63, 64, 65)


@pytest.fixture(scope="module")
def solver():
    yield from bc.open_solver()


@pytest.mark.parametrize("ce", PERIODS)
@pytest.mark.parametrize("T", STEPS)
def test_static_form_equals_generic_form(solver, T, ce):
    """Cold to the end, at iteration limits below, at and past the period-64 check, and warm-started from the
    neighbouring window's solution: the two instantiations agree bit for bit."""
    case = (T, 1, SEEDS[T])
    lp = bc.case_window(case)
    a, b = bc.both(solver, [lp], check_every=ce)
    bc.same(a[0], b[0], f"T {T} check_every {ce} cold")
    assert a[0].status == 0, f"T {T} check_every {ce}: {a[0].status_name} after {a[0].iters} iterations"
    for mi in LIMITS:
        la, lb = bc.both(solver, [lp], check_every=ce, max_iters=mi)
        bc.same(la[0], lb[0], f"T {T} check_every {ce} max_iters {mi}")
        assert la[0].iters <= mi
    nb = bc.case_window(bc.neighbour(case))
    wa, wb = bc.both(solver, [nb], start=[(a[0].x, a[0].y)], check_every=ce, warm_start=1)
    # (equality only: at check period 1 a warm start can run to the iteration limit, in both instantiations alike)
    bc.same(wa[0], wb[0], f"T {T} check_every {ce} warm")


def test_mixed_batch_takes_the_generic_form(solver):
    """J = 0, 1, 2 and 4 windows of T = 200 in one batch: the generic instantiation takes them all, and every window
    comes out as in a batch of its own (where the J = 1 window takes the static instantiation)."""
    lps = [bc.case_window((200, J, 5)) for J in (0, 1, 2, 4)]
    res = bc.solve(solver, lps, band_variant=GENERIC)
    for J, lp, r in zip((0, 1, 2, 4), lps, res):
        alone = bc.solve(solver, [lp], band_variant=STATIC if J == 1 else GENERIC)[0]
        assert r.status == 0
        bc.same(r, alone, f"J {J} in the mixed batch / alone")


def test_all_j1_batch_takes_the_static_form(solver):
    """40 J = 1 windows of mixed T, the first window again in the middle and at the end: the static instantiation is
    reported, the three copies agree bit for bit, every window equals the forced generic instantiation's result, and
    the choice costs no host wait."""
    Ts = (2, 25, 48, 96, 193, 200, 384, 600)
    lps = [bc.window(Ts[k % len(Ts)], 1, 7000 + k)[0] for k in range(38)]
    lps.insert(20, lps[0])
    lps.append(lps[0])
    res = bc.solve(solver, lps, band_variant=STATIC)
    syncs = solver.host_syncs()
    for k in (20, 39):
        bc.same(res[k], res[0], f"copy at position {k} / position 0")
    with bc.env("DVH_BAND_J1", "0"):
        gen = bc.solve(solver, lps, band_variant=GENERIC)
        assert solver.host_syncs() == syncs, (solver.host_syncs(), syncs)
    for k, (a, b) in enumerate(zip(res, gen)):
        assert a.status == 0, (k, a.status_name, a.iters)
        bc.same(a, b, f"window {k} static / generic")


def test_no_state_survives_a_window(solver):
    """1,100 J = 1 windows -- 11 distinct T = 48 windows, 100 copies each, interleaved -- so that every persistent
    workgroup takes at least two: every copy of a window is bit-identical (test_gpu_band_loop's check, on the static
    instantiation)."""
    base = [bc.window(48, 1, 4800 + k)[0] for k in range(11)]
    res = bc.solve(solver, [base[i % 11] for i in range(1100)], band_variant=STATIC)
    for i, r in enumerate(res):
        f = res[i % 11]
        assert r.status == f.status == 0 and r.iters == f.iters, (i, r.status, r.iters, f.status, f.iters)
        assert np.array_equal(r.x, f.x) and np.array_equal(r.y, f.y), f"copy {i} of window {i % 11} differs"
