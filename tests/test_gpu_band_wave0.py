"""Wave 0 of the three-step band form's plain iteration: its dual half-step reads the next lane's ene, the tau x-bar and
the init row's ene_0 directly behind the first barrier, and the init row (row 0, ene_0 = target, held by lane 63 of
wave 0) is updated from that early read without a wait of its own.  The arithmetic and its order per value are the
parent's, so everything here is either a bar against the host restatement (oracle/pdlp_ref.py: iterations within 128,
objective within 1e-7 relative, as tests/test_gpu_band_loop.py), the result contract recomputed from the returned x, y
(tests/result_contract.py, tests/kkt_ref.py; reference optimum: HiGHS), or bit-for-bit equality of the static
single-demand-period instantiation with the forced generic one (DVH_BAND_J1=0, as tests/test_gpu_band_j1.py).

Every window has a non-zero soc_target and llsoc, so the init row's dual is non-zero at the optimum; that is asserted
on the reference, otherwise nothing here would be about that row.  Step counts, all J = 1 on the forced "band3" path:
T = 2, 3, 4 (the init row and the end row one or two steps apart inside one lane), 192 / 193 (wave 0's last lane against
wave 1's first: the XE / YS hand-over next to the init lane), 576 / 577 (the last wave holds no step, then one),
766, 767, 768 (lane 63 of the last wave holds real steps).
"""
import contextlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

import result_contract as rc
from dervet_hip import BatchSolver
from dervet_hip.lp import builder
from oracle import pdlp_ref, window_lp

pytestmark = pytest.mark.gpu

GENERIC, STATIC = 9002004, 9002054  # kernel_stats()["band_variant"]
ITER_TOL = 128
OBJ_TOL = 1e-7
# T: seed (windows the reference solves in a few thousand iterations at most)
SEEDS = {2: 2, 3: 4, 4: 3, 192: 4, 193: 6, 576: 7, 577: 4, 766: 7, 767: 4, 768: 1}
STEPS = tuple(SEEDS)
PERIODS = (1, 2, 64)
LIMITS = (1, 63, 65)


def _oracle_lp(lp):
    K = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))
    return dict(K=K, q=lp.q, c=lp.c, c0=lp.c0, l=lp.l, u=lp.u, m_eq=lp.m_eq)


def _window(T, J, seed, G=1, load_scale=1.0):
    """G battery windows of T steps with J demand periods (test_gpu_band_loop._window)."""
    rng = np.random.default_rng(seed)
    load = load_scale * (400 + 200 * rng.random((G, T)))
    bat = dict(E=rng.uniform(500, 2000, G), Pch=rng.uniform(100, 400, G), Pdis=rng.uniform(100, 400, G),
               rte=rng.uniform(0.8, 0.95, G), sdr=rng.uniform(0, 1, G), soc_target=rng.uniform(0.3, 0.9, G),
               ulsoc=0.95, llsoc=0.05, fixedOM=10.0, OMexpenses=rng.uniform(0, 5, G))
    price = rng.uniform(0.03, 0.2, (G, T))
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


@pytest.fixture(scope="module")
def windows():
    return {T: _window(T, 1, SEEDS[T])[0] for T in STEPS}


@pytest.fixture(scope="module")
def refs(windows):
    """pdlp_ref at check period 64 and the HiGHS optimum of every window, computed once."""
    out = {}
    for T, lp in windows.items():
        olp = _oracle_lp(lp)
        h = window_lp.solve_highs(olp)
        assert h["status"] == 0, T
        out[T] = (olp, pdlp_ref.solve(olp, dict(check_every=64, kkt_every=1)), h["obj"])
    return out


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


def _agrees(r, ref, ce, what):
    print(f"{what}: gpu {r.iters} iterations, obj {r.obj!r}; reference {ref['iters']}, obj {ref['obj']!r}")
    assert ref["status"] == 0, f"{what}: the reference ends with status {ref['status']}"
    assert r.status == 0, f"{what}: {r.status_name} after {r.iters} iterations"
    assert r.iters % ce == 0, f"{what}: {r.iters} iterations is no multiple of the check period"
    assert abs(r.iters - ref["iters"]) <= ITER_TOL, f"{what}: gpu {r.iters} vs reference {ref['iters']} iterations"
    assert abs(r.obj - ref["obj"]) <= OBJ_TOL * abs(ref["obj"]), f"{what}: obj {r.obj!r} vs reference {ref['obj']!r}"


@pytest.mark.parametrize("T", STEPS)
def test_against_the_host_restatement(solver, windows, refs, T):
    """The static instantiation against oracle/pdlp_ref.py, and the result contract on the returned x, y."""
    olp, ref, opt = refs[T]
    assert ref["y"][0] != 0.0, f"T {T}: the reference's init-row dual is zero"
    r = _solve(solver, [windows[T]], STATIC)[0]
    _agrees(r, ref, 64, f"T {T}")
    assert r.y[0] != 0.0, f"T {T}: init-row dual is zero"
    rc.check_both(olp, r, opt, f"T {T}", "band3_J1")


@pytest.mark.parametrize("ce", PERIODS)
@pytest.mark.parametrize("T", STEPS)
def test_static_equals_generic(solver, windows, T, ce):
    """Iteration limits below, off and at the period (a loop entered and left every iteration at period 1), static
    against forced generic, bit for bit."""
    for mi in LIMITS:
        a, b = _both(solver, [windows[T]], check_every=ce, max_iters=mi)
        _same(a[0], b[0], f"T {T} check_every {ce} max_iters {mi}")
        assert a[0].iters <= mi


def test_warm_start_with_a_nonzero_init_row_dual(solver, windows, refs):
    """A window started from its neighbour's solution (3 % less load), whose init-row dual is non-zero."""
    _, ra, _ = refs[193]
    assert ra["y"][0] != 0.0
    nb = _window(193, 1, SEEDS[193], load_scale=1.03)[0]
    ref = pdlp_ref.solve(_oracle_lp(nb), dict(check_every=64, kkt_every=1, x0=ra["x"], y0=ra["y"]))
    a, b = _both(solver, [nb], start=[(ra["x"], ra["y"])], warm_start=1)
    _same(a[0], b[0], "T 193 warm")
    _agrees(a[0], ref, 64, "T 193 warm")


def test_restarts(solver, windows):
    """Check period 4: the window restarts several times (the reference's trace: the iterations since the last restart
    fall back), the bars hold, and the two instantiations agree bit for bit."""
    lp = windows[193]
    trace = []
    ref = pdlp_ref.solve(_oracle_lp(lp), dict(check_every=4, kkt_every=1), trace=trace)
    ks = [t[1] for t in trace]
    restarts = sum(1 for u, v in zip(ks, ks[1:]) if v <= u)
    print(f"reference: {ref['iters']} iterations, {restarts} restarts")
    assert restarts >= 4, restarts
    a, b = _both(solver, [lp], check_every=4)
    _same(a[0], b[0], "T 193 check_every 4")
    _agrees(a[0], ref, 4, "T 193 check_every 4")


def test_no_state_survives_a_window(solver):
    """1,100 cheap windows, T = 2 and T = 200 alternating with different soc_target, so that every persistent workgroup
    takes several: every window equals its solo solve bit for bit."""
    base = [_window(2 if k % 2 == 0 else 200, 1, 9100 + k)[0] for k in range(10)]
    solo = [_solve(solver, [lp], STATIC)[0] for lp in base]
    res = _solve(solver, [base[i % 10] for i in range(1100)], STATIC)
    for i, r in enumerate(res):
        f = solo[i % 10]
        assert r.status == f.status == 0 and r.iters == f.iters, (i, r.status, r.iters, f.status, f.iters)
        assert np.array_equal(r.x, f.x) and np.array_equal(r.y, f.y), f"copy {i} of window {i % 10} differs from its solo solve"
