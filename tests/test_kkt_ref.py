"""CPU: the host KKT reference (tests/kkt_ref.py) on hand-built LPs whose numbers follow from the algebra, and against
oracle/pdlp_ref.py's own kkt on the iterate it returns."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_ref
import planted_lp
from oracle import pdlp_ref

INF = np.inf


def _lp():
    """One column of each bound class (free, lower only, upper only, boxed, fixed); row 0 an equality, rows 1, 2 >=.

        min  2 x0 + 3 x1 - 1 x2 + 1 x3 + 5 x4 + 7
        s.t. x0 + x1 + x2 + x3 + x4  = 4        (y0)
             x0 - x2                >= 1        (y1: active at x below)
             x1 + x3                >= -5       (y2: inactive)
             x0 free, x1 >= 0, x2 <= 2, 0 <= x3 <= 3, x4 = 1
    """
    K = sp.csr_matrix(np.array([[1.0, 1, 1, 1, 1], [1, 0, -1, 0, 0], [0, 1, 0, 1, 0]]))
    return dict(K=K, q=np.array([4.0, 1.0, -5.0]), c=np.array([2.0, 3.0, -1.0, 1.0, 5.0]), c0=7.0,
                l=np.array([-INF, 0.0, -INF, 0.0, 1.0]), u=np.array([INF, INF, 2.0, 3.0, 1.0]), m_eq=1)


X = np.array([2.0, 0.0, 1.0, 0.0, 1.0])  # feasible: row 0: 4 = 4, row 1: 1 >= 1 (active), row 2: 0 >= -5 (inactive)


def test_a_kkt_point_has_zero_residuals_and_gap():
    lp = _lp()
    # rc = c - K'y = (2 - y0 - y1, 3 - y0 - y2, -1 - y0 + y1, 1 - y0 - y2, 5 - y0): x0 free -> y0 + y1 = 2; x2 interior
    # of its upper bound -> y1 - y0 = 1: y0 = 0.5, y1 = 1.5, y2 = 0; rc = (0, 2.5, 0, 0.5, 4.5) with x1, x3 at their
    # lower bounds (lam >= 0 fine), x4 fixed
    y = np.array([0.5, 1.5, 0.0])
    k = kkt_ref.kkt(lp, X, y)
    assert k["pres"] == 0.0 and k["dres_rel"] == 0.0 and k["rdx"] == 0.0
    assert k["pobj"] == 2 * 2 - 1 + 5 + 7 == 15.0
    # dobj = q'y + l1 lam1 + l3 lam3 + l4 lam4 + c0 = 2 + 1.5 + 0 + 0 + 4.5 + 7
    assert k["dobj"] == 15.0 and k["gap_rel"] == 0.0
    assert k["ynorm"] == pytest.approx(math.sqrt(0.25 + 2.25), rel=1e-15)
    for name in ("pres_rel", "dres_rel", "gap_rel", "pobj", "dobj", "rdx", "ynorm", "pres"):
        assert 0.0 <= k[name + "_bound"] < 1e-13, name


def test_inactive_and_violated_ge_rows():
    lp = _lp()
    y = np.array([0.5, 1.5, 0.0])
    x = X.copy()
    x[0] = 3.0  # row 0: q - Kx = -1; row 1: 1 - 2 = -1 -> clipped to 0; row 2 still inactive
    k = kkt_ref.kkt(lp, x, y)
    assert k["pres"] == 1.0
    assert k["pres_rel"] == pytest.approx(1.0 / (1.0 + math.sqrt(16 + 1 + 25)), rel=1e-15)
    x[0] = 1.0  # row 0: +1; row 1: 1 - 0 = +1 (violated, counts)
    k = kkt_ref.kkt(lp, x, y)
    assert k["pres"] == pytest.approx(math.sqrt(2.0), rel=1e-15)


def test_a_negative_dual_on_a_ge_row_moves_the_numbers_as_the_algebra_says():
    """y2 = -1 (a wrong sign: the header promises y >= 0 on >= rows; the reference evaluates what it is given):
    rc1 = 3 - 0.5 + 1 = 3.5, rc3 = 1 - 0.5 + 1 = 1.5, both still carried by the lower bounds (0): r_d stays 0;
    dobj moves by q2 y2 = +5."""
    lp = _lp()
    k = kkt_ref.kkt(lp, X, np.array([0.5, 1.5, -1.0]))
    assert k["dres_rel"] == 0.0
    assert k["dobj"] == 20.0 and k["pobj"] == 15.0
    assert k["gap_rel"] == pytest.approx(5.0 / 36.0, rel=1e-15)


def test_a_wrong_dual_on_an_upper_only_column():
    """y1 = 2.5 instead of 1.5: rc0 = 2 - 0.5 - 2.5 = -1 on the free column -> r_d0 = -1; rc2 = -1 - 0.5 + 2.5 = 1 > 0
    on the upper-only column, which only carries rc <= 0 -> r_d2 = 1 and no bound term.  ||r_d|| = sqrt 2,
    rdx = 1 * 2 + 1 * 1 = 3, dobj = 4 * 0.5 + 1 * 2.5 + 0 + 0 + 4.5 + 7 = 16."""
    lp = _lp()
    k = kkt_ref.kkt(lp, X, np.array([0.5, 2.5, 0.0]))
    assert k["dres_rel"] == pytest.approx(math.sqrt(2.0) / (1.0 + math.sqrt(4 + 9 + 1 + 1 + 25)), rel=1e-15)
    assert k["rdx"] == 3.0 and k["dobj"] == 16.0
    # the same column with rc < 0: y1 = 0.5 -> rc2 = -1, carried by the upper bound 2: bound term 2 * (-1);
    # rc0 = 1 on the free column
    k = kkt_ref.kkt(lp, X, np.array([0.5, 0.5, 0.0]))
    assert k["dres_rel"] == pytest.approx(1.0 / (1.0 + math.sqrt(40.0)), rel=1e-15)
    assert k["dobj"] == 4 * 0.5 + 0.5 + 2 * (-1.0) + 4.5 + 7 == 12.0
    assert k["rdx"] == 2.0


def test_boxed_column_takes_either_bound_by_the_sign():
    lp = _lp()
    # y0 = 2: rc3 = 1 - 2 = -1 < 0 on the boxed column -> u3 lam = 3 * (-1); rc1 = 1 (lower 0), rc4 = 3 (fixed at 1),
    # rc0 = 2 - 2 - 0 = 0, rc2 = -1 - 2 = -3 (upper 2 -> -6)
    k = kkt_ref.kkt(lp, X, np.array([2.0, 0.0, 0.0]))
    assert k["dres_rel"] == 0.0
    assert k["dobj"] == 8.0 - 3.0 + 0.0 + 3.0 - 6.0 + 7.0


def test_rounding_bounds_cover_a_double_precision_evaluation():
    """The bounds are forward bounds for any double-precision evaluation: the plain numpy one must lie inside."""
    for seed in (1, 2, 3):
        lp = planted_lp.planted(300, 100, 150, 6, 6, seed, scale_spread=2.0, long_rows=2, long_row_len=40)
        rng = np.random.default_rng(seed)
        x = np.clip(lp["x_star"] + 1e-3 * rng.standard_normal(300), lp["l"], lp["u"])
        y = lp["y_star"] + 1e-3 * rng.standard_normal(250)
        k = kkt_ref.kkt(lp, x, y)
        K, q, c, l, u = lp["K"], lp["q"], lp["c"], lp["l"], lp["u"]
        r = q - K @ x
        r[100:] = np.maximum(r[100:], 0)
        rc = c - K.T @ y
        fl, fu = np.isfinite(l), np.isfinite(u)
        lam = np.where(fl & fu, rc, np.where(fl, np.maximum(rc, 0), np.where(fu, np.minimum(rc, 0), 0.0)))
        pobj = c @ x + lp["c0"]
        dobj = q @ y + np.sum(np.where(fl, l, 0) * np.maximum(lam, 0)) + np.sum(np.where(fu, u, 0) * np.minimum(lam, 0)) \
            + lp["c0"]
        got = dict(pres_rel=np.linalg.norm(r) / (1 + np.linalg.norm(q)),
                   dres_rel=np.linalg.norm(rc - lam) / (1 + np.linalg.norm(c)),
                   gap_rel=abs(pobj - dobj) / (1 + abs(pobj) + abs(dobj)), pobj=pobj, dobj=dobj,
                   rdx=np.sum(np.abs(rc - lam) * np.abs(x)), ynorm=np.linalg.norm(y), pres=np.linalg.norm(r))
        for name, v in got.items():
            assert abs(v - k[name]) <= k[name + "_bound"], (seed, name, v, k[name], k[name + "_bound"])
            assert k[name + "_bound"] <= 1e-9 * (1 + abs(k[name])), (seed, name, k[name + "_bound"])


def test_agrees_with_the_algorithm_restatements_own_kkt():
    for seed in (1, 2):
        lp = planted_lp.planted(60, 30, 25, 4, 4, seed)
        r = pdlp_ref.solve(lp)
        assert r["status"] == 0
        k = kkt_ref.kkt(lp, r["x"], r["y"])
        for name in ("pres_rel", "dres_rel", "gap_rel", "pobj", "dobj", "rdx", "ynorm", "pres"):
            # (pdlp_ref unscales its iterate once more inside kkt: a rounding per entry on top of the bound)
            assert abs(k[name] - r["kkt"][name]) <= 10 * k[name + "_bound"] + 1e-14 * (1 + abs(k[name])), name
        lhs, _ = kkt_ref.objective_gate(k)
        assert lhs <= 1e-6 * (1 + abs(k["pobj"]))


def test_empty_rows_and_columns_and_a_matrix_without_entries():
    K = sp.csr_matrix((2, 2))
    lp = dict(K=K, q=np.array([0.0, -1.0]), c=np.array([1.0, -2.0]), c0=0.5, l=np.array([0.0, -1.0]),
              u=np.array([2.0, 3.0]), m_eq=1)
    k = kkt_ref.kkt(lp, np.array([0.0, 3.0]), np.zeros(2))
    assert k["pres"] == 0.0 and k["dres_rel"] == 0.0
    assert k["pobj"] == -5.5 and k["dobj"] == 0.0 * 1.0 + 3.0 * -2.0 + 0.5 and k["gap_rel"] == 0.0
