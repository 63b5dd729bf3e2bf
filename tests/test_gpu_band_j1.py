"""The band kernel's single-demand-period instantiation (three-step battery form, J a compile-time 1): the host
launches it for a batch without a J != 1 battery window, DVH_BAND_J1=0 keeps the generic instantiation (J read from the
descriptor), and both compute the same thing -- the static one only drops what J == 1 never uses (the tau update and the
init row on the waves without the tau column, the per-step period index, two of three XT reads).

Windows are built as test_gpu_band_loop._window.  Statuses, iteration counts, the four statistics, x and y are compared
bit for bit: the arithmetic and its order are those of the generic instantiation's J == 1 path.

The defensive check (a J != 1 window handed to the static instantiation leaves through bail()) has no case here: the
host counts the J != 1 windows itself and no test hook launches the static instantiation over a list that has one.
"""
import contextlib
import os

import numpy as np
import pytest

from dervet_hip import BatchSolver
from dervet_hip.lp import builder

pytestmark = pytest.mark.gpu

GENERIC, STATIC = 9002004, 9002054  # kernel_stats()["band_variant"]; ["variant"] stays the form's code
STEPS = (2, 25, 193, 600)  # degenerate; padding steps inside a lane; both sides of the wave 0 / wave 1 boundary; 4 waves
PERIODS = (1, 3, 64)
LIMITS = (1, 63, 64, 65)
SEEDS = {2: 2, 25: 4, 193: 5, 600: 4}


def _window(T, J, seed, G=1, load_scale=1.0):
    """G battery windows of T steps with J demand periods (test_gpu_band_loop._window)."""
    rng = np.random.default_rng(seed)
    load = load_scale * (400 + 200 * rng.random((G, T)))
    bat = dict(E=rng.uniform(500, 2000, G), Pch=rng.uniform(100, 400, G), Pdis=rng.uniform(100, 400, G),
               rte=rng.uniform(0.8, 0.95, G), sdr=rng.uniform(0, 1, G), soc_target=rng.uniform(0.3, 0.9, G),
               ulsoc=0.95, llsoc=0.05, fixedOM=10.0, OMexpenses=rng.uniform(0, 5, G))
    price = rng.uniform(0.03, 0.2, (G, T))
    if J == 0:
        g = builder.battery_group(T, 1.0, load, bat, retail_price=price)
    else:
        masks = np.zeros((J, T), bool)
        if J == 1:
            masks[0, : (T + 1) // 2] = True
        else:
            for j in range(J):
                masks[j, j::J] = True
        g = builder.battery_group(T, 1.0, load, bat, retail_price=price, demand_masks=masks,
                                  demand_prices=rng.uniform(5, 20, (G, J)))
    return builder.group_window_lps(g)


@pytest.fixture(scope="module")
def solver():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no GPU is visible (run with -m 'not gpu' on CPU hosts)")
    with BatchSolver(0) as s:
        yield s


@contextlib.contextmanager
def _generic_forced():
    """DVH_BAND_J1=0 (read by the library at every launch) for the solves inside."""
    old = os.environ.get("DVH_BAND_J1")
    os.environ["DVH_BAND_J1"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["DVH_BAND_J1"]
        else:
            os.environ["DVH_BAND_J1"] = old


def _solve(s, lps, band_variant, start=None, **options):
    opts = dict(check_every=64, kkt_every=1, kkt_predict=0, max_iters=100000, warm_start=0)
    opts.update(options)
    s.set_options(**opts)
    s.set_kernel_path("band3")
    res = s.solve(lps, start=start)
    st = s.kernel_stats()
    assert st["band_windows"] == len(lps) and st["variant"] == GENERIC and st["band_variant"] == band_variant, st
    return res


def _both(s, lps, **kw):
    """The same solve by the static instantiation and, forced, by the generic one."""
    a = _solve(s, lps, STATIC, **kw)
    with _generic_forced():
        b = _solve(s, lps, GENERIC, **kw)
    return a, b


def _same(a, b, what):
    print(f"{what}: status {a.status} / {b.status}, iterations {a.iters} / {b.iters}, obj {a.obj!r} / {b.obj!r}")
    assert (a.status, a.iters) == (b.status, b.iters), f"{what}: status, iterations {a.status, a.iters} vs {b.status, b.iters}"
    sa = np.array([a.obj, a.primal_res_rel, a.dual_res_rel, a.gap_rel])
    sb = np.array([b.obj, b.primal_res_rel, b.dual_res_rel, b.gap_rel])
    assert np.array_equal(sa, sb, equal_nan=True), f"{what}: stats {sa} vs {sb}"
    assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y), f"{what}: x or y differ"


@pytest.mark.parametrize("ce", PERIODS)
@pytest.mark.parametrize("T", STEPS)
def test_static_form_equals_generic_form(solver, T, ce):
    """Cold to the end, at iteration limits below, at and past the period-64 check, and warm-started from the
    neighbouring window's solution: the two instantiations agree bit for bit."""
    lp = _window(T, 1, SEEDS[T])[0]
    a, b = _both(solver, [lp], check_every=ce)
    _same(a[0], b[0], f"T {T} check_every {ce} cold")
    assert a[0].status == 0, f"T {T} check_every {ce}: {a[0].status_name} after {a[0].iters} iterations"
    for mi in LIMITS:
        la, lb = _both(solver, [lp], check_every=ce, max_iters=mi)
        _same(la[0], lb[0], f"T {T} check_every {ce} max_iters {mi}")
        assert la[0].iters <= mi
    nb = _window(T, 1, SEEDS[T], load_scale=1.03)[0]
    wa, wb = _both(solver, [nb], start=[(a[0].x, a[0].y)], check_every=ce, warm_start=1)
    # (equality only: at check period 1 a warm start can run to the iteration limit, in both instantiations alike)
    _same(wa[0], wb[0], f"T {T} check_every {ce} warm")


def test_mixed_batch_takes_the_generic_form(solver):
    """J = 0, 1, 2 and 4 windows of T = 200 in one batch: the generic instantiation takes them all, and every window
    comes out as in a batch of its own (where the J = 1 window takes the static instantiation)."""
    lps = [_window(200, J, 5)[0] for J in (0, 1, 2, 4)]
    res = _solve(solver, lps, GENERIC)
    for J, lp, r in zip((0, 1, 2, 4), lps, res):
        alone = _solve(solver, [lp], STATIC if J == 1 else GENERIC)[0]
        assert r.status == 0
        _same(r, alone, f"J {J} in the mixed batch / alone")


def test_all_j1_batch_takes_the_static_form(solver):
    """40 J = 1 windows of mixed T, the first window again in the middle and at the end: the static instantiation is
    reported, the three copies agree bit for bit, every window equals the forced generic instantiation's result, and
    the choice costs no host wait."""
    Ts = (2, 25, 48, 96, 193, 200, 384, 600)
    lps = [_window(Ts[k % len(Ts)], 1, 7000 + k)[0] for k in range(38)]
    lps.insert(20, lps[0])
    lps.append(lps[0])
    res = _solve(solver, lps, STATIC)
    syncs = solver.host_syncs()
    for k in (20, 39):
        _same(res[k], res[0], f"copy at position {k} / position 0")
    with _generic_forced():
        gen = _solve(solver, lps, GENERIC)
        assert solver.host_syncs() == syncs, (solver.host_syncs(), syncs)
    for k, (a, b) in enumerate(zip(res, gen)):
        assert a.status == 0, (k, a.status_name, a.iters)
        _same(a, b, f"window {k} static / generic")


def test_no_state_survives_a_window(solver):
    """1,100 J = 1 windows -- 11 distinct T = 48 windows, 100 copies each, interleaved -- so that every persistent
    workgroup takes at least two: every copy of a window is bit-identical (test_gpu_band_loop's check, on the static
    instantiation)."""
    base = [_window(48, 1, 4800 + k)[0] for k in range(11)]
    res = _solve(solver, [base[i % 11] for i in range(1100)], STATIC)
    for i, r in enumerate(res):
        f = res[i % 11]
        assert r.status == f.status == 0 and r.iters == f.iters, (i, r.status, r.iters, f.status, f.iters)
        assert np.array_equal(r.x, f.x) and np.array_equal(r.y, f.y), f"copy {i} of window {i % 11} differs"
