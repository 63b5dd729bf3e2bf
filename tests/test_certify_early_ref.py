"""The in-kernel Farkas test of ``certify = 2`` restated in numpy (tests/certify_early_ref.py) on the population the
GPU tests draw from: certify_ref.poi_window over T in {2, 3, 5, 25, 200, 768} x J in {0, 1, 2} x the six kinds x PV
on / off, and the kinds "feasible" and "min_soe" without POI rows.  Every HiGHS-infeasible window is certified within
4,096 iterations (the worst: 3,456, T = 768, J = 1, margin_out with PV) with a ray that passes certify_ref.farkas;
no HiGHS-feasible window -- margin_in, 8 % inside feasibility, among them -- is certified before its OPTIMAL
termination (or before 30,000 iterations for T <= 25 and 8,192 above, where the optimum takes longer than that)."""
import numpy as np
import pytest

import certify_early_ref as er
import certify_ref as cr


@pytest.mark.parametrize("T", er.TS)
@pytest.mark.parametrize("J", er.JS)
def test_population(T, J):
    n_bad = n_good = 0
    for pv in (False, True):
        for key in er.keys_of(T, J, pv) + er.keys_no_poi(T, J, pv):
            lp, status = er.window(key), er.highs(key)[0]
            assert status in (0, 2), key
            if status == 2:
                r = er.solve(lp, max_iters=2 * er.EARLY_CAP)
                assert r["status"] == er.PRIMAL_INFEASIBLE and r["iters"] <= er.EARLY_CAP, (key, r["status"], r["iters"])
                assert r["iters"] % er.KKT_PERIOD == 0
                margin, viol = er.farkas_bars(lp, r["y"])
                assert (margin, viol) == (r["margin"], r["viol"])
                # the unscaled candidate passes the certificate pass's own test as well
                assert cr._farkas_candidate(lp, r["y"], cr._K(lp)) is not None, key
                n_bad += 1
            else:
                r = er.solve(lp, max_iters=30000 if T <= 25 else 8192)
                assert r["status"] in (er.OPTIMAL, er.ITER_LIMIT), (key, r["status"], r["iters"])
                n_good += 1
    assert n_bad >= 4 and n_good >= 4


def test_early_exit_leaves_a_feasible_solve_alone():
    """With the test on, a feasible window's restated solve is the one without it, bit for bit."""
    key = er.keys_of(25, 1, True)[3]  # margin_in
    assert key[2] == "margin_in" and er.highs(key)[0] == 0
    a, b = er.solve(er.window(key)), er.solve(er.window(key), early=False)
    assert a["status"] == b["status"] == er.OPTIMAL and a["iters"] == b["iters"]
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"])
    assert abs(er.window(key).c @ a["x"] + er.window(key).c0 - er.highs(key)[1]) <= 1e-5 * abs(er.highs(key)[1])


def test_scaled_terms_are_the_unscaled_ones():
    """q'v, the bound terms and the violation formed from y~, K~'y~ and the scaled data equal certify_ref's on v."""
    import scipy.sparse as sp
    from oracle import pdlp_ref
    lp = er.window(er.keys_of(25, 2, True)[1])  # overload
    K = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))
    Dr, Dc = pdlp_ref.precondition(K, 10)
    Kt = sp.diags(Dr) @ K @ sp.diags(Dc)
    ys = np.random.default_rng(3).uniform(-1.0, 1.0, lp.m)
    ys[lp.m_eq:] = np.abs(ys[lp.m_eq:])
    _, margin, viol, scale = er.farkas_scaled(ys, Kt.T @ ys, Dr * lp.q, lp.l / Dc, lp.u / Dc, Dc, lp.m_eq)
    m2, v2, s2 = cr.farkas_terms(lp, Dr * ys)
    assert abs(margin - m2) <= 1e-12 * s2 and abs(scale - s2) <= 1e-12 * s2 and abs(viol - v2) <= 1e-12 * max(v2, 1.0)
