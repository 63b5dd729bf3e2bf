"""GPU: the certificate pass (csrc/dvh_certify.hip; BatchSolver(certify=1), BatchSolver.certify) against HiGHS and
the numpy certificate tests of tests/certify_ref.py.  A window the cascade leaves ITER_LIMIT / NUMERICAL and the pass
certifies comes back "infeasible" / "unbounded" with a ray that passes ``certify_ref.farkas`` / ``ray`` in numpy;
every other window is bit-identical to the same solve with the pass off.  max_iters = 4096 keeps the main solve of
an infeasible window short."""
import dataclasses
import functools

import numpy as np
import pytest

import certify_ref as cr
from dervet_hip import BatchSolver, _lib
from dervet_hip.lp import builder, scenarios

pytestmark = pytest.mark.gpu
MAX_ITERS = 4096
PATHS = ("default", "ell", "generic", "band1", "band3", "interconnect")


@pytest.fixture(scope="module")
def cert_solver(gpu_solver):  # (gpu_solver: the suite's no-GPU failure message)
    s = BatchSolver(0, max_iters=MAX_ITERS, certify=1)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _highs(key):
    """HiGHS status / objective of a window of this module, computed once (key: tiny kind or poi_window arguments)."""
    return cr.highs_status(_window(key))


@functools.lru_cache(maxsize=None)
def _window(key):
    return cr.tiny(key) if isinstance(key, str) else cr.poi_window(*key[:3], **dict(key[3:]))


def _check_farkas(lp, r):
    """The issue's bars for a Farkas ray: margin > 0, viol <= 1e-8 margin, ||y||_inf = 1 to 1e-12, >= rows >= 0, the
    reported margin within 1e-9 relative of numpy's."""
    margin, viol = cr.farkas(lp, r.y)
    print(f"farkas n={lp.n} m={lp.m}: margin {margin:.6e} (reported {r.primal_res_rel:.6e}) viol {viol:.3e} "
          f"(reported {r.dual_res_rel:.3e}) iters {r.iters}")
    assert r.status_name == "infeasible" and r.obj == np.inf and r.gap_rel == 0.0
    assert margin > 0.0 and viol <= 1e-8 * margin
    assert abs(np.max(np.abs(r.y)) - 1.0) <= 1e-12 and np.all(r.y[lp.m_eq:] >= 0.0)
    assert abs(r.primal_res_rel - margin) <= 1e-9 * margin


def test_tiny_lps(cert_solver):
    keys = ("infeasible", "unbounded", "infeasible_twin", "unbounded_twin")
    lps = [_window(k) for k in keys]
    assert [_highs(k)[0] for k in keys] == [2, 3, 0, 0]
    res = cert_solver.solve(lps)
    assert [r.status_name for r in res] == ["infeasible", "unbounded", "optimal", "optimal"]
    _check_farkas(lps[0], res[0])
    d = res[1].x
    descent, viol = cr.ray(lps[1], d)
    assert res[1].obj == -np.inf and descent > 0.0 and viol <= 1e-8 * descent
    assert abs(np.max(np.abs(d)) - 1.0) <= 1e-12 and np.all(d >= 0.0)
    assert abs(res[1].primal_res_rel - descent) <= 1e-9 * descent
    for k, r in zip(keys[2:], res[2:]):
        assert abs(r.obj - cr.TINY_OBJ[k]) <= 1e-5 * abs(cr.TINY_OBJ[k])
    st = cert_solver.certify_stats()
    assert st["primal_infeasible"] == 1 and st["dual_infeasible"] == 1 and st["examined"] == 2 and st["skipped"] == 0
    assert st["max_iters"] % cr.CHECK == 0 and 0 < st["max_iters"] <= cr.CAP


# smallest recurrence, a wave boundary, the full block; one generic window near the LDS limit (n = 3,001, m = 4,001)
SHAPES = [(T, pv, False) for T in (2, 3, 65, 768) for pv in (False, True)] + [(1000, False, True)]


@pytest.mark.parametrize("T,pv,dense", SHAPES)
def test_shapes_match_highs_and_rays_pass_in_numpy(cert_solver, T, pv, dense):
    keys = [(T, 1, kind, ("pv", pv), ("dense", dense)) for kind in ("feasible", "overload", "min_soe")]
    lps = [_window(k) for k in keys]
    hs = [_highs(k) for k in keys]
    assert [h[0] for h in hs] == [0, 2, 2]
    try:
        # (the month-long feasible windows need more than 4,096 iterations to reach the optimum HiGHS reports)
        cert_solver.set_options(max_iters=MAX_ITERS if T <= 65 else 100000)
        res = cert_solver.solve(lps)
        st = cert_solver.certify_stats()
    finally:
        cert_solver.set_options(max_iters=MAX_ITERS)
    print(T, pv, [(r.status_name, r.iters) for r in res], st)
    assert [r.status_name for r in res] == ["optimal", "infeasible", "infeasible"]
    assert abs(res[0].obj - hs[0][1]) <= 1e-5 * abs(hs[0][1])
    for lp, r in zip(lps[1:], res[1:]):
        _check_farkas(lp, r)
    assert st["primal_infeasible"] == 2 and st["dual_infeasible"] == 0 and st["skipped"] == 0


def _config4_batch():
    """Four config-4 battery windows, the third with an energy bound at step 1 that is unreachable from the starting
    SOE but not crossed.  (A config-4 window starts full, ene_0 = the upper limit, so no lower bound at step 1 is
    out of reach; it is the upper bound that is set below what one step of discharge at the rating leaves.)"""
    lps = [lp for g in scenarios.config4([3]) for lp in builder.group_window_lps(g)][:4]
    lp = lps[2]
    T = lp.m_eq - 1
    p = lp.indptr[1]  # row 1: -dt rte ch_0 + dt dis_0 - (1 - dt sdr) ene_0 + ene_1 = 0
    reach = -lp.data[p + 2] * lp.q[0] - lp.data[p + 1] * lp.u[T]  # the lowest ene_1
    lo = lp.l[2 * T + 1]
    assert lo < reach
    u = lp.u.copy()
    u[2 * T + 1] = 0.5 * (lo + reach)
    lps[2] = dataclasses.replace(lp, u=u)
    return lps


@pytest.mark.parametrize("path", PATHS)
def test_every_kernel_path_certifies_and_leaves_the_neighbours_alone(path, cert_solver):
    lps = _config4_batch()
    assert cr.highs_status(lps[2])[0] == 2
    try:
        cert_solver.set_kernel_path(path)
        cert_solver.set_options(certify=0)
        off = cert_solver.solve(lps)
        syncs_off, st_off = cert_solver.host_syncs(), cert_solver.certify_stats()
        cert_solver.set_options(certify=1)
        on = cert_solver.solve(lps)
        syncs_on, st_on = cert_solver.host_syncs(), cert_solver.certify_stats()
    finally:
        cert_solver.set_kernel_path("default")
        cert_solver.set_options(certify=1)
    print(path, [(r.status_name, r.iters) for r in off], [(r.status_name, r.iters) for r in on], st_on)
    assert off[2].status in (_lib.ITER_LIMIT, _lib.NUMERICAL) and st_off["examined"] == 0
    _check_farkas(lps[2], on[2])
    assert on[2].iters == off[2].iters  # the main solve's count stays
    assert np.array_equal(on[2].x, off[2].x)  # and its x: the ray went into y
    for k in (0, 1, 3):
        assert on[k].status == off[k].status and on[k].obj == off[k].obj and on[k].iters == off[k].iters
        assert np.array_equal(on[k].x, off[k].x) and np.array_equal(on[k].y, off[k].y)
    assert syncs_on == syncs_off
    assert st_on["primal_infeasible"] == 1 and st_on["examined"] >= 1


def test_the_pass_is_opt_in(gpu_solver):
    lp = _window("infeasible")
    with BatchSolver(0, max_iters=MAX_ITERS) as s:
        r = s.solve([lp])[0]
        st = s.certify_stats()
    assert r.status_name not in ("optimal", "infeasible")
    assert st["examined"] == 0 and st["primal_infeasible"] == 0 and st["ms"] == 0.0


def test_certificates_are_bit_reproducible(cert_solver):
    keys = ["infeasible", "unbounded"] + [(65, 1, kind, ("pv", True)) for kind in ("feasible", "overload", "short")]
    lps = [_window(k) for k in keys]
    runs = []
    for _ in range(2):
        res = cert_solver.solve(lps)
        st = cert_solver.certify_stats()
        runs.append((res, {k: v for k, v in st.items() if k != "ms"}))
    (a, sa), (b, sb) = runs
    assert sa == sb and sa["primal_infeasible"] == 3 and sa["dual_infeasible"] == 1
    for ra, rb in zip(a, b):
        assert ra.status == rb.status and ra.iters == rb.iters
        assert ra.x.tobytes() == rb.x.tobytes() and ra.y.tobytes() == rb.y.tobytes()
        assert (ra.obj, ra.primal_res_rel, ra.dual_res_rel) == (rb.obj, rb.primal_res_rel, rb.dual_res_rel)


def test_screen_decides_a_mixed_list_before_any_solve(cert_solver):
    keys = ["infeasible", "unbounded", "infeasible_twin", "unbounded_twin"] + \
           [(24, 2, kind) for kind in cr.KINDS] + [(65, 1, "short", ("pv", True))]
    lps = [_window(k) for k in keys]
    want = [cr.expected_status(_highs(k)[0]) for k in keys]
    assert set(want) == {1, 2, 5}
    res = cert_solver.certify(lps)
    st = cert_solver.certify_stats()
    print([(r.status_name, r.iters) for r in res], st)
    assert [r.status for r in res] == want
    assert all(r.status_name in ("infeasible", "unbounded", "undecided") for r in res)
    for lp, r in zip(lps, res):
        if r.status == 1:
            _check_farkas(lp, r)
            assert r.iters % cr.CHECK == 0 and r.iters > 0
        elif r.status == 5:
            assert not r.x.any() and not r.y.any()  # untouched
    assert st["examined"] == len(lps) and st["primal_infeasible"] == want.count(1)
    assert st["dual_infeasible"] == want.count(2) and st["skipped"] == 0
    assert st["max_iters"] == max(r.iters for r in res if r.status in (1, 2))


def test_every_device_of_a_handle_certifies_its_share(cert_solver):
    """A handle over two sub-handles (the same GPU twice) splits the batch; each part's infeasible windows are
    certified on its device, the counts are summed, and the results equal the one-device handle's bit for bit."""
    keys = [(24, 1, kind) for kind in ("overload", "feasible", "min_soe", "feasible", "short", "overload")]
    lps = [_window(k) for k in keys]
    one = cert_solver.solve(lps)
    st_one = cert_solver.certify_stats()
    with BatchSolver(devices=[0, 0], max_iters=MAX_ITERS, certify=1) as s:
        two = s.solve(lps)
        st_two = s.certify_stats()
    assert [r.status_name for r in two] == ["infeasible", "optimal", "infeasible", "optimal", "infeasible", "infeasible"]
    assert {k: v for k, v in st_two.items() if k != "ms"} == {k: v for k, v in st_one.items() if k != "ms"}
    assert st_two["primal_infeasible"] == 4
    for a, b in zip(one, two):
        assert a.status == b.status and a.iters == b.iters and a.obj == b.obj
        assert a.x.tobytes() == b.x.tobytes() and a.y.tobytes() == b.y.tobytes()


def _battery(T, kind):
    """A plain battery window (no POI rows) of T steps, infeasible through its minimum SOE at step 1."""
    return cr.poi_window(T, 1, kind, poi=False)


def test_windows_above_the_on_chip_size_are_skipped_and_counted(cert_solver):
    """A battery window of 1,000 steps (n = 3,001) is still an on-chip window and is certified; the medium tier starts
    above n = 4,096 (1,500 steps here): its infeasible window stays ITER_LIMIT and is counted under ``skipped``."""
    small, medium = _battery(1000, "min_soe"), _battery(1500, "min_soe")
    assert medium.n > 4096 and small.n <= 4096 and small.m <= 4096
    assert cr.highs_status(small)[0] == 2 and cr.highs_status(medium)[0] == 2
    res = cert_solver.solve([small, medium])
    st, ks = cert_solver.certify_stats(), cert_solver.kernel_stats()
    print([(r.status_name, r.iters) for r in res], st, ks)
    _check_farkas(small, res[0])
    assert res[1].status == _lib.ITER_LIMIT and ks["chain_windows"] == 1
    assert st["skipped"] == 1 and st["examined"] == 1 and st["primal_infeasible"] == 1
    scr = cert_solver.certify([medium])
    assert scr[0].status_name == "undecided" and cert_solver.certify_stats()["skipped"] == 1
