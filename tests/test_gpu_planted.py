"""GPU: planted-optimum LPs (tests/planted_lp.py) through the general kernels -- every compiled ELL instantiation
(csrc/dvh_kernels.hip launch_pdhg_ell), the generic CSR kernel's five sizes with the matrices in LDS and not, and the
grid-wide path -- none of which had seen an LP with free, upper-only, boxed and fixed columns, scale spread, empty rows
and columns, or long rows that are no demand-charge column.

tests/planted_cases.py lists the cases with the kernel each must reach (asserted here from the path counts and the
variant code) and says how the shapes follow from the dispatch: n below, at and one above each instantiation's
column slots, m below, at and one above its row slots (one above lands on the next kernel), ELL widths at and one above each instantiation's, a row of exactly 32 entries and one of 33, exactly 64 long
rows and 65.  tests/test_planted_lp.py holds the CPU side (HiGHS returns the planted value; the host restatement needs
at most 25,000 iterations).  Each window must come back OPTIMAL within the default max_iters and meet contracts A and
B (tests/result_contract.py) against the planted value; x and y must lie within 1e-4 (1 + |x*|), 1e-4 (1 + |y*|) of
the planted optimum, which is unique by construction -- except where planted_cases.py switches the distance check off
because the host restatement itself misses that bar (the scale-spread windows).
"""
import numpy as np
import pytest

import band_cases as bc
import planted_cases as pc
import planted_lp
import result_contract as rc
from dervet_hip import BatchSolver, _lib

pytestmark = pytest.mark.gpu

OPTIONS = dict(eps=1e-6, eps_obj=1e-6, max_iters=100000, check_every=32, kkt_every=4, kkt_predict=0, warm_start=0,
               certify=0)
COUNTS = ("band_windows", "ell_windows", "generic_windows", "large_windows", "chain_windows")


@pytest.fixture(scope="module")
def solver():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no GPU is visible (run with -m 'not gpu' on CPU hosts)")
    with BatchSolver(0) as s:
        s.set_options(**OPTIONS)
        yield s


def _solve(s, path, lps, **options):
    s.set_options(**dict(OPTIONS, **options))
    s.set_kernel_path(path)
    try:
        res = s.solve(lps)
        return res, s.kernel_stats()
    finally:
        s.set_kernel_path("default")
        s.set_options(**OPTIONS)


def _distance(lp, r):
    dx = float(np.max(np.abs(r.x - lp["x_star"]) / (1 + np.abs(lp["x_star"]))))
    dy = float(np.max(np.abs(r.y - lp["y_star"]) / (1 + np.abs(lp["y_star"]))))
    return dx, dy


@pytest.mark.parametrize("name", list(pc.GENERAL))
def test_planted_optimum_through_the_general_kernels(solver, name):
    n, m_eq, m_ineq, wy, wx, seed, opts, path, copies, tier, variant, distance = pc.GENERAL[name]
    lp = pc.general(name)
    res, ks = _solve(solver, path, [planted_lp.to_window(lp)] * copies)
    if tier is None:  # long rows: the ELL kernel that is launched may hand the window to the generic kernel
        assert ks["ell_windows"] + ks["generic_windows"] == copies and ks["large_windows"] == ks["band_windows"] == 0, ks
    else:
        for k in COUNTS:
            assert ks[k] == (copies if k == tier else 0), (name, ks)
    if variant is not None:
        assert ks["variant"] == variant, (name, ks)
    form = "large" if tier == "large_windows" else "generic" if ks["generic_windows"] else "ell"
    rc.check_both(lp, res[0], lp["opt"], name, form)
    dx, dy = _distance(lp, res[0])
    print(f"RESULT_CONTRACT form={form} case={name} variant={ks['variant']} distance_x={dx:.3e} distance_y={dy:.3e}")
    if distance:
        assert dx <= 1e-4 and dy <= 1e-4, (name, dx, dy)
    for r in res[1:]:  # copies of one window in one launch: the same bits
        assert r.status == 0 and r.iters == res[0].iters and np.array_equal(r.x, res[0].x) \
            and np.array_equal(r.y, res[0].y)


LIMITS = bc.LIMITS


@pytest.mark.parametrize("name", ["small12_at", "ell24_22_at", "ell24_53_at", "gen22_lds", "gen53", "large4097"])
def test_iteration_limits_on_the_general_kernels(solver, name):
    """A limit below, at and past the check period on an ELL kernel with K in registers and one with K in LDS, the
    generic kernel with the matrices in LDS and not, and the grid-wide path: a check runs at the limit
    (csrc/dvh_solve.cpp make_opts), so the numbers are finite and describe the returned x, y (contract B) -- before,
    the on-chip kernels returned NaN and an unchecked x, y for max_iters < check_every.  These windows need 256 to 384
    iterations at the default periods; at this period one may end OPTIMAL at iteration 128, which contract B covers too."""
    n, m_eq, m_ineq, wy, wx, seed, opts, path, copies, tier, variant, distance = pc.GENERAL[name]
    lp = pc.general(name)
    w = planted_lp.to_window(lp)
    worst = 0.0
    for mi in LIMITS:
        res, ks = _solve(solver, path, [w], max_iters=mi, check_every=64, kkt_every=1)
        r = res[0]
        assert ks[tier] == 1, (name, mi, ks)
        assert (r.status == _lib.ITER_LIMIT and r.iters == mi) or (r.status == 0 and r.iters == 128 < mi), \
            (name, mi, r.status_name, r.iters)
        assert np.isfinite([r.obj, r.primal_res_rel, r.dual_res_rel, r.gap_rel]).all(), (name, mi)
        assert np.all(r.x >= lp["l"]) and np.all(r.x <= lp["u"]) and np.all(r.y[m_eq:] >= 0), (name, mi)
        worst = max(worst, rc.check_reported(lp, r, f"{name} max_iters {mi}")[1])
    print(f"RESULT_CONTRACT form={'large' if tier == 'large_windows' else tier[:-8]} case=iteration_limits "
          f"reported_vs_recomputed={worst:.3e}")


def test_sixty_five_long_rows_come_back_numerical_and_leave_the_neighbours_alone(solver):
    """kLMax = 64 long rows per window are handled on chip (case gen_long64 above solves); one more and the set-up
    refuses the window: NUMERICAL, never OPTIMAL, with NaN numbers -- and the other windows of the batch come back bit
    for bit as without it."""
    neighbours = [planted_lp.to_window(pc.general(k)) for k in ("gen_long64", "gen_rows_32_33", "gen22_lds")]
    bad = planted_lp.to_window(pc.long65())
    alone, ks0 = _solve(solver, "generic", neighbours)
    mixed, ks1 = _solve(solver, "generic", neighbours[:1] + [bad] + neighbours[1:])
    assert ks0["generic_windows"] == 3 and ks1["generic_windows"] == 4, (ks0, ks1)
    r = mixed[1]
    assert r.status == _lib.NUMERICAL and r.iters == 0, (r.status_name, r.iters)
    assert np.isnan([r.obj, r.primal_res_rel, r.dual_res_rel, r.gap_rel]).all()
    for a, b in zip(alone, mixed[:1] + mixed[2:]):
        assert a.status == b.status == 0 and a.iters == b.iters and a.obj == b.obj
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
    # the default cascade ends the same way (set-up flag -> the ELL kernel hands on -> the generic kernel reports)
    res, _ = _solve(solver, "default", [bad])
    assert res[0].status == _lib.NUMERICAL


def test_mixed_batch_of_size_classes_equals_the_solo_results(solver):
    """One planted window of each size class (the small ELL kernels' n <= 512 and m <= 768, the other on-chip windows,
    and past the on-chip kernels) in one batch with battery windows: the route kernel splits them by class, every window
    keeps the kernel it has alone, and every result equals the solo result bit for bit."""
    planted = [planted_lp.to_window(pc.general(k)) for k in pc.MIXED]
    battery = [planted_lp.to_window(pc.band_windows()[k][0]) for k in ("T25J1", "T200J4")]
    solo = []
    for w in planted + battery:
        r, _ = _solve(solver, "default", [w])
        solo.append(r[0])
    order = [battery[0], planted[0], planted[2], battery[1], planted[1]]
    want = [solo[3], solo[0], solo[2], solo[4], solo[1]]
    res, ks = _solve(solver, "default", order)
    assert ks["band_windows"] == 2 and ks["ell_windows"] == 2 and ks["large_windows"] == 1 \
        and ks["generic_windows"] == ks["chain_windows"] == 0, ks
    for k, (a, b) in enumerate(zip(want, res)):
        assert a.status == b.status == 0 and a.iters == b.iters and a.obj == b.obj, (k, a.iters, b.iters)
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y), k
        assert (a.primal_res_rel, a.dual_res_rel, a.gap_rel) == (b.primal_res_rel, b.dual_res_rel, b.gap_rel), k
