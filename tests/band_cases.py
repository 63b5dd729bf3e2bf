"""What the band kernel's GPU tests share (tests/test_gpu_band_loop.py, _j1, _wave0, _reads; tests/band_limits.py): the
variant codes, the window generator, the case tables with the reason for every step count, the solve that asserts which
kernel ran, the comparisons and their bars, and the host references, computed once per session.  A change to the band
kernel adds its cases to the tables here and its tests to a test file; it does not bring a harness of its own.

The generator's draws and their order are pinned: the bits in tests/golden/band_limits_parent.json belong to its
windows (tests/test_band_cases.py holds the generator to the digests recorded there).
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from dervet_hip.lp import builder
from oracle import pdlp_ref, window_lp
from planted_lp import from_window as oracle_lp  # noqa: F401  (the oracle dict of a WindowLP)

# kernel_stats()["variant"] and ["band_variant"] (csrc/dvh_internal.h launch_pdhg_band):
# 9000000 + 1000 (steps per lane - 1) + 100 ice + waves per window, + 50 (kBandJ1) for the compile-time J = 1 instantiation
GENERIC = 9002004   # three steps per lane, J read from the descriptor; also the three-step form's "variant"
STATIC = 9002054    # its single-demand-period instantiation ("band_variant" only)
ONE_STEP = 9000012  # one step per lane
ICE = 9000112       # one step per lane with the LP-relaxed ICE columns and rows
FORM_VARIANT = {"band3": GENERIC, "band1": ONE_STEP}  # kernel path: the form's "variant"

ITER_TOL = 128   # iterations, against the host restatement (tests/test_gpu_parity.py's bars)
OBJ_TOL = 1e-7   # objective, relative, against the host restatement
LIMITS = (1, 2, 63, 64, 65, 127, 129)  # max_iters below, at and past one and two check periods of 64


def window(T, J, seed, G=1, load_scale=1.0, masks=None):
    """G battery + DCM windows of T steps with J demand periods: J = 0 none, J = 1 the first half of the window (as
    test_gpu_configs.test_band_kernel_forms_agree), J > 1 interleaved; masks [J, T] replaces these periods (it is built
    by the caller and draws nothing).  Non-zero soc_target and llsoc, so the init row's dual is non-zero at the optimum."""
    rng = np.random.default_rng(seed)
    load = load_scale * (400 + 200 * rng.random((G, T)))
    bat = dict(E=rng.uniform(500, 2000, G), Pch=rng.uniform(100, 400, G), Pdis=rng.uniform(100, 400, G),
               rte=rng.uniform(0.8, 0.95, G), sdr=rng.uniform(0, 1, G), soc_target=rng.uniform(0.3, 0.9, G),
               ulsoc=0.95, llsoc=0.05, fixedOM=10.0, OMexpenses=rng.uniform(0, 5, G))
    price = rng.uniform(0.03, 0.2, (G, T))
    if J == 0:
        g = builder.battery_group(T, 1.0, load, bat, retail_price=price)
    else:
        if masks is None:
            masks = np.zeros((J, T), bool)
            if J == 1:
                masks[0, : (T + 1) // 2] = True
            else:
                for j in range(J):
                    masks[j, j::J] = True
        g = builder.battery_group(T, 1.0, load, bat, retail_price=price, demand_masks=masks,
                                  demand_prices=rng.uniform(5, 20, (G, J)))
    return builder.group_window_lps(g)


# ---- cases: (T, J, seed) or (T, J, seed, load_scale), one window each (G = 1).  The seeds are those whose windows the
# host restatement solves in a few thousand iterations at most: it runs on the host.
@functools.lru_cache(maxsize=None)
def case_window(case):
    T, J, seed, load_scale = (tuple(case) + (1.0,))[:4]
    return window(T, J, seed, load_scale=load_scale)[0]


def neighbour(case):
    """The same site and battery with 3 % more load: the window a carried or warm start is tried on."""
    return tuple(case[:3]) + (1.03,)


# test_gpu_band_wave0 (all J = 1), T: seed
WAVE0_SEEDS = {
    2: 2, 3: 4, 4: 3,           # the init row and the end row one or two steps apart inside one lane
    192: 4, 193: 6,             # wave 0's last lane against wave 1's first: the XE / YS hand-over next to the init lane
    576: 7, 577: 4,             # the last wave holds no step, then one
    766: 7, 767: 4, 768: 1,     # lane 63 of the last wave holds real steps
}
# test_gpu_band_j1 (all J = 1), T: seed
J1_SEEDS = {
    2: 2,    # degenerate
    25: 4,   # padding steps inside a lane
    193: 5,  # both sides of the wave 0 / wave 1 boundary
    600: 4,  # all four waves
}
# test_gpu_band_loop, both battery forms
LOOP_WINDOWS = {
    "T2": (2, 1, 2),        # degenerate
    "T25": (25, 1, 4),      # padding steps inside a lane
    "T200J0": (200, 0, 5),  # two waves of the three-step form hold steps; no tau column
    "T200J1": (200, 1, 5),  # the straight-line tau path
    "T200J4": (200, 4, 5),  # the per-column tau loop
    "T600": (600, 1, 4),    # all four waves
}
HARD = (200, 1, 201)  # needs thousands of iterations: no iteration limit of LIMITS ends it early
WARM_PAIR = (HARD, neighbour(HARD))
# test_gpu_band_reads, (T, J): seed.  J = 1: wave0's windows; J = 2 and 4 on its T = 193 seed take the generic
# instantiation's other loop body (the per-column tau path on wave 0)
READS_SEEDS = {**{(T, 1): seed for T, seed in WAVE0_SEEDS.items()}, (193, 2): WAVE0_SEEDS[193], (193, 4): WAVE0_SEEDS[193]}


# ---- host references, one computation per case and session; nobody writes to what these return
@functools.lru_cache(maxsize=None)
def reference(case, check_every=64):
    """(pdlp_ref's cold solve of the case at the check period, its trace)."""
    trace = []
    ref = pdlp_ref.solve(oracle_lp(case_window(case)), dict(check_every=check_every, kkt_every=1), trace=trace)
    return ref, tuple(trace)


@functools.lru_cache(maxsize=None)
def optimum(case):
    """The HiGHS optimum of the case."""
    h = window_lp.solve_highs(oracle_lp(case_window(case)))
    assert h["status"] == 0, case
    return h["obj"]


def restarts(trace):
    """Restarts in a pdlp_ref trace: checks at which the iterations since the last restart fell back."""
    ks = [t[1] for t in trace]
    return sum(1 for u, v in zip(ks, ks[1:]) if v <= u)


# ---- the solver and the solve
def open_solver():
    """A fresh BatchSolver(0) for a module-scoped fixture (options and the kernel path persist on a solver, so no two
    test modules share one); without a GPU the test fails, it does not skip."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no GPU is visible (run with -m 'not gpu' on CPU hosts)")
    from dervet_hip import BatchSolver
    with BatchSolver(0) as s:
        yield s


@contextlib.contextmanager
def env(name, value):
    """An A/B switch the library reads at every launch (DVH_BAND_J1, DVH_BAND_QUEUE), for the solves inside."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def solve(s, lps, path="band3", variant=None, band_variant=None, start=None, **options):
    """Solve lps on a forced battery form and assert that it took them all: the form's variant code (that of the path
    unless given) and, where given, the instantiation."""
    opts = dict(check_every=64, kkt_every=1, kkt_predict=0, max_iters=100000, warm_start=0)
    opts.update(options)
    s.set_options(**opts)
    s.set_kernel_path(path)
    res = s.solve(lps, start=start)
    st = s.kernel_stats()
    assert st["band_windows"] == len(lps) and st["variant"] == (FORM_VARIANT[path] if variant is None else variant), (path, st)
    assert band_variant is None or st["band_variant"] == band_variant, (path, st)
    return res


def both(s, lps, **kw):
    """The same three-step solve by the static instantiation and, forced (DVH_BAND_J1=0), by the generic one."""
    a = solve(s, lps, band_variant=STATIC, **kw)
    with env("DVH_BAND_J1", "0"):
        b = solve(s, lps, band_variant=GENERIC, **kw)
    return a, b


# ---- comparisons
def same(a, b, what):
    """Bit for bit: status, iterations, the four statistics, x and y."""
    print(f"{what}: status {a.status} / {b.status}, iterations {a.iters} / {b.iters}, obj {a.obj!r} / {b.obj!r}")
    assert (a.status, a.iters) == (b.status, b.iters), f"{what}: status, iterations {a.status, a.iters} vs {b.status, b.iters}"
    sa = np.array([a.obj, a.primal_res_rel, a.dual_res_rel, a.gap_rel])
    sb = np.array([b.obj, b.primal_res_rel, b.dual_res_rel, b.gap_rel])
    assert np.array_equal(sa, sb, equal_nan=True), f"{what}: stats {sa} vs {sb}"
    assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y), f"{what}: x or y differ"


def agrees(r, ref, ce, what):
    """The bars against the host restatement's solve ref at check period ce."""
    print(f"{what}: gpu {r.iters} iterations, obj {r.obj!r}; reference {ref['iters']}, obj {ref['obj']!r}")
    assert ref["status"] == 0, f"{what}: the reference ends with status {ref['status']}"
    assert r.status == 0, f"{what}: {r.status_name} after {r.iters} iterations"
    assert r.iters % ce == 0, f"{what}: {r.iters} iterations is no multiple of the check period"
    assert abs(r.iters - ref["iters"]) <= ITER_TOL, f"{what}: gpu {r.iters} vs reference {ref['iters']} iterations"
    assert abs(r.obj - ref["obj"]) <= OBJ_TOL * abs(ref["obj"]), f"{what}: obj {r.obj!r} vs reference {ref['obj']!r}"
