"""CPU: the planted-optimum LPs (tests/planted_lp.py) are what they claim, and every LP the GPU tests use
(tests/planted_cases.py) has the planted value as its optimum (HiGHS, 1e-9 relative) and is solved by the host
restatement of the algorithm within 25,000 iterations -- a condition on the cases, fixed in planted_cases.py, so that a
GPU tier has four-fold room under the default max_iters."""
import numpy as np
import pytest
import scipy.sparse as sp

import chain_plan_ref
import kkt_ref
import planted_cases as pc
import planted_lp
from oracle import pdlp_ref, window_lp

ITER_CONDITION = 25000


def _planted_point_is_optimal(lp):
    x, y = lp["x_star"], lp["y_star"]
    assert np.all(x >= lp["l"]) and np.all(x <= lp["u"]) and np.all(y[lp["m_eq"]:] >= 0)
    k = kkt_ref.kkt(lp, x, y)
    for name in ("pres_rel", "dres_rel", "gap_rel"):  # zero up to the rounding of q and c
        assert k[name] <= 4 * k[name + "_bound"] + 1e-15, (name, k[name], k[name + "_bound"])
    # strict complementarity: slack > 0 or y > 0 on every >= row, lam != 0 on every column at a bound
    slack = (lp["K"] @ x - lp["q"])[lp["m_eq"]:]
    scale = 1.0 + np.abs(lp["q"][lp["m_eq"]:])
    assert np.all((slack > 1e-9 * scale) != (y[lp["m_eq"]:] > 0))
    at_bound = (x == lp["l"]) | (x == lp["u"])
    assert np.all((lp["lam_star"] != 0) == at_bound)


def test_every_bound_class_and_option():
    lp = planted_lp.planted(60, 30, 25, 4, 4, 3, empty_cols=2, empty_rows=2, long_rows=1, long_row_len=20, long_cols=1,
                            long_col_len=12)
    _planted_point_is_optimal(lp)
    assert set(lp["classes"]) == set(planted_lp.CLASSES)
    fl, fu = np.isfinite(lp["l"]), np.isfinite(lp["u"])
    assert (~fl & ~fu).any() and (fl & ~fu).any() and (~fl & fu).any() and (fl & fu & (lp["u"] > lp["l"])).any() \
        and (lp["l"] == lp["u"]).any()
    K = sp.csr_matrix(lp["K"])
    rl, cl = np.diff(K.indptr), np.diff(K.tocsc().indptr)
    assert sorted(rl)[:2] == [0, 0] and sorted(cl)[:2] == [0, 0] and rl.max() == 20 and cl.max() == 12
    assert np.all(lp["q"][rl == 0] < 0) and np.all(lp["c"][cl == 0] != 0)
    assert np.all(np.delete(rl, np.argmax(rl)) <= 4 + 1)  # (a row may hold the long column's entry on top)
    assert planted_lp.widths(lp)[:2] == (4, 4)


def test_scale_spread_spreads_the_entries():
    a = planted_lp.planted(60, 30, 25, 4, 4, 3)
    b = planted_lp.planted(60, 30, 25, 4, 4, 3, scale_spread=2.0)
    _planted_point_is_optimal(b)
    ra = np.abs(a["K"].data).max() / np.abs(a["K"].data).min()
    rb = np.abs(b["K"].data).max() / np.abs(b["K"].data).min()
    assert ra < 100 and rb > 1e4, (ra, rb)


def test_pivot_block_is_dominant():
    """K[active rows, interior columns]: one pivot per row and column, dominating its row's other interior entries."""
    lp = planted_lp.planted(300, 100, 150, 6, 6, 2)
    K = sp.csr_matrix(lp["K"]).toarray()
    act = np.nonzero(lp["pivot"] >= 0)[0]
    piv = lp["pivot"][act]
    assert len(set(piv.tolist())) == len(act) == int(lp["interior"].sum())
    B = np.abs(K[np.ix_(act, piv)])
    assert np.all(2 * np.diag(B) > B.sum(axis=1))


def _check_case(lp, name, want_unique_distance=None):
    _planted_point_is_optimal(lp)
    h = window_lp.solve_highs(lp)
    assert h["status"] == 0, name
    assert abs(h["obj"] - lp["opt"]) <= 1e-9 * (1 + abs(lp["opt"])), (name, h["obj"], lp["opt"])
    r = pdlp_ref.solve(lp)
    dx = float(np.max(np.abs(r["x"] - lp["x_star"]) / (1 + np.abs(lp["x_star"]))))
    dy = float(np.max(np.abs(r["y"] - lp["y_star"]) / (1 + np.abs(lp["y_star"]))))
    print(f"{name}: n {len(lp['c'])} m {len(lp['q'])} reference {r['iters']} iterations, objective error "
          f"{abs(r['obj'] - lp['opt']) / (1 + abs(lp['opt'])):.1e}, distance x {dx:.1e} y {dy:.1e}")
    assert r["status"] == 0, (name, r["status"])
    assert r["iters"] <= ITER_CONDITION, (name, r["iters"])
    if want_unique_distance:
        assert dx <= 1e-4 and dy <= 1e-4, (name, dx, dy)


@pytest.mark.parametrize("name", list(pc.GENERAL))
def test_general_case(name):
    n, m_eq, m_ineq, wy, wx, seed, opts, path, copies, tier, variant, distance = pc.GENERAL[name]
    lp = pc.general(name)
    K = sp.csr_matrix(lp["K"])
    assert K.shape == (m_eq + m_ineq, n)
    # the widths the table asks for are the widths the set-up kernel will count
    got = planted_lp.widths(lp)
    assert got[:2] == ((wx, wy) if wx <= 8 else (got[0], wy)), (name, got)  # (wx > 8 bounds columns that are no ELL width)
    if name == "setup_many_rows":
        assert (m_eq + m_ineq) + n > 16 * (n + 1)  # csrc/dvh_kernels.hip setup_kernel: fl_lds is false (4 segments)
    if tier == "generic_windows":  # matrices in LDS or not, as the variant code says
        fits = pc.generic_lds_bytes(n, m_eq + m_ineq, K.nnz) <= 160 * 1024
        assert variant == (1000 if fits else 0) + 10 * -(-n // 512) + -(-(m_eq + m_ineq) // 512), (name, K.nnz)
    if name == "gen_rows_32_33":
        assert {32, 33} <= set(np.diff(K.indptr).tolist()) and {32, 33} <= set(np.diff(K.tocsc().indptr).tolist())
    if name == "gen_long64":
        assert int((np.diff(K.indptr) > 32).sum()) == 64
    _check_case(lp, name, want_unique_distance=distance)


def test_long65_has_one_long_row_too_many():
    K = sp.csr_matrix(pc.long65()["K"])
    assert int((np.diff(K.indptr) > 32).sum()) == 65


@pytest.mark.parametrize("family", ["band", "ice", "interconnect", "chain"])
def test_window_cases(family):
    cases = dict(band=pc.band_windows, ice=pc.ice_windows, interconnect=pc.interconnect_windows,
                 chain=pc.chain_windows)[family]()
    for name, (base, lp) in cases.items():
        assert (lp["K"] != base["K"]).nnz == 0 and np.array_equal(lp["l"], base["l"]) \
            and np.array_equal(lp["u"], base["u"]) and lp["m_eq"] == base["m_eq"]
        _check_case(lp, f"{family} {name}")
        r = pdlp_ref.solve(base)  # the realistic window the GPU tests solve next to it: the same condition
        print(f"{family} {name} realistic: reference {r['iters']} iterations")
        assert r["status"] == 0 and r["iters"] <= ITER_CONDITION, (family, name, r["status"], r["iters"])


@pytest.mark.parametrize("name", list(pc.CHAIN_PLAN))
def test_chain_plan_case(name):
    """The chain plan's windows (no GPU test solves them yet: the condition is met ahead of those tests): the table's tau
    ids are the window's, and the same condition.  Of the 49k-step windows only the planted twin is held to it; the
    host restatement needs 20 s and more for a realistic one."""
    T, J, tau = pc.CHAIN_PLAN[name][:3]
    base, lp = pc.chain_plan_window(name)
    got, gj = chain_plan_ref.tau_ids(base)
    assert gj == J and np.array_equal(got, tau) and base["K"].shape[1] == 3 * T + J
    assert (lp["K"] != base["K"]).nnz == 0 and np.array_equal(lp["l"], base["l"]) \
        and np.array_equal(lp["u"], base["u"]) and lp["m_eq"] == base["m_eq"]
    _check_case(lp, f"chain_plan {name}")
    if name in pc.CHAIN_PLAN_LONG:
        return
    r = pdlp_ref.solve(base)
    print(f"chain_plan {name} realistic: reference {r['iters']} iterations")
    assert r["status"] == 0 and r["iters"] <= ITER_CONDITION, (name, r["status"], r["iters"])


def test_route_twin_stays_on_chip():
    base = pc.route_twin()
    assert base["K"].shape[1] == 4096 and base["K"].shape[0] <= 4096
    assert pc.chain_plan_window("route_J2")[0]["K"].shape[1] == 4097
    r = pdlp_ref.solve(base)
    assert r["status"] == 0 and r["iters"] <= ITER_CONDITION, (r["status"], r["iters"])
