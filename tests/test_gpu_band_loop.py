"""The band kernel's solve loop: plain iterations run in an inner loop of their own between two checks, so the
iteration counter, the check counter and the iteration limit must come out exactly as before -- for every check
period, for limits below, at and off a multiple of the period, for both wave kinds (the wave with the tau column and
the others), and with no state carried from one window of a persistent workgroup to the next.

Both battery forms run ("band3": three steps per lane, persistent grid; "band1": one step per lane) on battery + DCM
windows built as in test_gpu_configs.test_band_kernel_forms_agree.  Step counts: T = 2 (degenerate), 25 (padding
steps inside a lane), 200 (two waves of the three-step form hold steps, so both loop variants do real work), 600 (all
four waves); J = 0, 1 and 4 demand periods on the T = 200 window (no tau column / the straight-line tau path / the
per-column loop).  The reference is the numpy restatement of the algorithm (oracle/pdlp_ref.py) with the same options;
the bars against it are those of test_gpu_parity.test_iterates_match_host_restatement: iterations within 128,
objective within 1e-7 relative.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from dervet_hip import BatchSolver
from dervet_hip.lp import builder
from oracle import pdlp_ref

pytestmark = pytest.mark.gpu

PATHS = (("band3", 9002004), ("band1", 9000012))
PERIODS = (1, 2, 3, 64, 100)
LIMITS = (1, 2, 63, 64, 65, 127, 129)
ITER_TOL = 128
OBJ_TOL = 1e-7
ITER_LIMIT = 3


def _oracle_lp(lp):
    K = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))
    return dict(K=K, q=lp.q, c=lp.c, c0=lp.c0, l=lp.l, u=lp.u, m_eq=lp.m_eq)


def _window(T, J, seed, G=1, load_scale=1.0):
    """G battery windows of T steps with J demand periods (J = 1: the first half of the window, as the forms test)."""
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


def _windows():
    # (seeds whose windows the reference solves in few thousand iterations at most: it runs on the host)
    return {"T2": _window(2, 1, 2)[0], "T25": _window(25, 1, 4)[0], "T200J0": _window(200, 0, 5)[0],
            "T200J1": _window(200, 1, 5)[0], "T200J4": _window(200, 4, 5)[0], "T600": _window(600, 1, 4)[0]}


def _hard_window():
    """A window that needs thousands of iterations (the reference: see test_iteration_limit)."""
    return _window(200, 1, 201)[0]


def _warm_pair():
    """A window and its neighbour: the same site and battery with 3 % more load."""
    return _window(200, 1, 201)[0], _window(200, 1, 201, load_scale=1.03)[0]


@pytest.fixture(scope="module")
def solver():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no GPU is visible (run with -m 'not gpu' on CPU hosts)")
    with BatchSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def windows():
    return _windows()


@pytest.fixture(scope="module")
def ref_by_period(windows):
    """pdlp_ref on every window at a check period, computed once per period and shared by the two forms."""
    cache = {}

    def get(ce):
        if ce not in cache:
            cache[ce] = {name: pdlp_ref.solve(_oracle_lp(lp), dict(check_every=ce, kkt_every=1))
                         for name, lp in windows.items()}
        return cache[ce]
    return get


def _solve(s, path, variant, lps, start=None, **options):
    opts = dict(check_every=64, kkt_every=1, kkt_predict=0, max_iters=100000, warm_start=0)
    opts.update(options)
    s.set_options(**opts)
    s.set_kernel_path(path)
    res = s.solve(lps, start=start)
    st = s.kernel_stats()
    assert st["band_windows"] == len(lps) and st["variant"] == variant, (path, st)
    return res


def _agrees(r, ref, ce, what):
    print(f"{what}: gpu {r.iters} iterations, obj {r.obj!r}; reference {ref['iters']}, obj {ref['obj']!r}")
    assert ref["status"] == 0, f"{what}: the reference ends with status {ref['status']}"
    assert r.status == 0, f"{what}: {r.status_name} after {r.iters} iterations"
    assert r.iters % ce == 0, f"{what}: {r.iters} iterations is no multiple of the check period"
    assert abs(r.iters - ref["iters"]) <= ITER_TOL, f"{what}: gpu {r.iters} vs reference {ref['iters']} iterations"
    assert abs(r.obj - ref["obj"]) <= OBJ_TOL * abs(ref["obj"]), f"{what}: obj {r.obj!r} vs reference {ref['obj']!r}"


@pytest.mark.parametrize("path,variant", PATHS)
def test_iteration_limit(solver, path, variant):
    """max_iters below, at and just past one and two check periods: the loop of plain iterations stops at the limit,
    not at the period, and the count comes back exact (as oracle/pdlp_ref.solve with the same options)."""
    lp = _hard_window()
    for mi in LIMITS:
        r = _solve(solver, path, variant, [lp], max_iters=mi)[0]
        print(f"{path} max_iters {mi}: status {r.status}, iters {r.iters}")
        assert r.status == ITER_LIMIT, f"{path} max_iters {mi}: {r.status_name}"
        assert r.iters == mi, f"{path} max_iters {mi}: {r.iters} iterations"


@pytest.mark.parametrize("path,variant", PATHS)
@pytest.mark.parametrize("ce", PERIODS)
def test_check_period(solver, windows, ref_by_period, path, variant, ce):
    names = list(windows)
    res = _solve(solver, path, variant, [windows[k] for k in names], check_every=ce)
    for name, r in zip(names, res):
        _agrees(r, ref_by_period(ce)[name], ce, f"{path} check_every {ce} {name}")


def test_reproducible_and_order_free(solver):
    """1,100 windows on the persistent form -- 11 distinct T = 48 windows, 100 copies each, interleaved -- so that every
    workgroup slot takes at least two windows: every copy of a window is bit-identical in x, y, status and iterations
    (no loop state survives from one window to the next)."""
    base = [_window(48, 1 + (k % 2), 4800 + k)[0] for k in range(11)]
    lps = [base[i % 11] for i in range(1100)]
    res = _solve(solver, "band3", 9002004, lps)
    for i, r in enumerate(res):
        f = res[i % 11]
        assert r.status == f.status == 0 and r.iters == f.iters, (i, r.status, r.iters, f.status, f.iters)
        assert np.array_equal(r.x, f.x) and np.array_equal(r.y, f.y), f"copy {i} of window {i % 11} differs"


@pytest.fixture(scope="module")
def warm_case():
    """(window, its neighbour's reference solution, the reference's warm solve from it), computed once."""
    a, b = _warm_pair()
    ra = pdlp_ref.solve(_oracle_lp(a), dict(check_every=64, kkt_every=1))
    assert ra["status"] == 0
    return b, ra, pdlp_ref.solve(_oracle_lp(b), dict(check_every=64, kkt_every=1, x0=ra["x"], y0=ra["y"]))


@pytest.mark.parametrize("path,variant", PATHS)
def test_warm_start(solver, warm_case, path, variant):
    """A window started from its neighbour's solution (warm_start = 1): the check-period assertions at period 64."""
    b, ra, ref = warm_case
    r = _solve(solver, path, variant, [b], start=[(ra["x"], ra["y"])], warm_start=1)[0]
    _agrees(r, ref, 64, f"{path} warm start")
