"""The certificate pass restated in numpy (tests/certify_ref.py, the reference of tests/test_gpu_certify.py) against
HiGHS: on POI windows that are feasible, overloaded, short of energy, marginal on either side of the energy limit or
bound to an unreachable minimum SOE, and on the tiny LPs, ``certify`` certifies every window
scipy.optimize.linprog(method="highs") reports infeasible, none it solves, and every ray it returns passes the
certificate test on its own."""
import numpy as np
import pytest

import certify_ref as cr

SHAPES = [(T, J) for T in (5, 24, 65, 168) for J in (0, 1, 2)]


def _check_farkas(lp, got):
    y = got["ray"]
    margin, viol = cr.farkas(lp, y)
    assert margin > 0.0 and viol <= cr.RAY_TOL * margin, (margin, viol)
    assert abs(np.max(np.abs(y)) - 1.0) <= 1e-12 and np.all(y[lp.m_eq:] >= 0.0)
    assert abs(margin - got["margin"]) <= 1e-12 * abs(margin)


@pytest.mark.parametrize("T,J", SHAPES)
def test_population_matches_highs(T, J):
    seen = set()
    for kind in cr.KINDS:
        lp = cr.poi_window(T, J, kind)
        hs, _ = cr.highs_status(lp)
        got = cr.certify(lp, cr.CAP // 4)  # (a quarter of the default cap: the headroom DESIGN.md section 4 asks for)
        seen.add(hs)
        assert got["status"] == cr.expected_status(hs), (kind, hs, got["status"], got["iters"])
        if hs == 2:
            assert got["iters"] % cr.CHECK == 0
            _check_farkas(lp, got)
        else:
            assert got["ray"] is None
    assert seen == {0, 2}  # the population holds windows of both kinds at every shape


def test_population_is_what_it_says():
    """The kinds are infeasible (or not) for the reason they name: HiGHS on a day window."""
    hs = {kind: cr.highs_status(cr.poi_window(24, 1, kind))[0] for kind in cr.KINDS}
    assert hs == {"feasible": 0, "overload": 2, "short": 2, "margin_in": 0, "margin_out": 2, "min_soe": 2}


def test_tiny_lps():
    lp = cr.tiny("infeasible")
    assert cr.highs_status(lp)[0] == 2
    got = cr.certify(lp, 1024)
    assert got["status"] == cr.PRIMAL_INFEASIBLE
    _check_farkas(lp, got)
    assert got["margin"] == pytest.approx(1.0)  # y = 1: 3 - (1 + 1)
    lp = cr.tiny("unbounded")
    assert cr.highs_status(lp)[0] == 3
    got = cr.certify(lp, 1024)
    assert got["status"] == cr.DUAL_INFEASIBLE
    descent, viol = cr.ray(lp, got["ray"])
    assert descent > 0.0 and viol <= cr.RAY_TOL * descent and np.all(got["ray"] >= 0.0)
    assert abs(np.max(np.abs(got["ray"])) - 1.0) <= 1e-12
    for kind, obj in cr.TINY_OBJ.items():
        lp = cr.tiny(kind)
        assert cr.highs_status(lp) == (0, pytest.approx(obj))
        assert cr.certify(lp, 2048)["status"] == cr.UNDECIDED


def test_a_feasible_point_refutes_every_candidate():
    """By construction no candidate passes on a feasible window: with x feasible, q'y <= r'x <= the bound sum, so the
    margin of any y with y_I >= 0 and no violation is <= 0 (checked on random duals and the HiGHS point's window)."""
    lp = cr.poi_window(24, 1, "feasible")
    rng = np.random.default_rng(5)
    for _ in range(20):
        y = rng.normal(size=lp.m)
        y[lp.m_eq:] = np.abs(y[lp.m_eq:])
        margin, viol, scale = cr.farkas_terms(lp, y / np.max(np.abs(y)))
        assert not cr._passes(margin, viol, scale)
