"""The two halves of the result contract (include/dervet_hip.h dvh_result), checked from a returned WindowResult and
the LP alone with the host reference tests/kkt_ref.py.  Shared by test_gpu_result_contract.py and test_gpu_planted.py.

Contract A -- an OPTIMAL result is optimal: l <= x <= u and y >= 0 on >= rows exactly; the recomputed pres_rel,
dres_rel, gap_rel <= eps (1 + 1e-6) + their rounding bounds (1e-6: five times the 2e-7 per-norm error dvh_band.hip
documents for its single-precision scale factors); the objective gate |pobj - dobj| + ||y|| ||r_p|| + rdx <=
eps_obj (1 + |pobj|) with the same slack (without rdx for the band ICE form, BandTune<true>::gate_rdx); pobj and dobj
within 1e-5 (1 + |optimum|) of the reference optimum (the planted value, or HiGHS).

Contract B -- the reported numbers describe the returned point: obj = c'x + c0 to 1e-9 relative; primal_res_rel,
dual_res_rel, gap_rel each within 1e-6 value + rounding bound of the recomputed one.
"""
import numpy as np

import kkt_ref

SLACK = 1e-6
OBJ_BAR = 1e-5


def check_reported(lp, r, what, k=None):
    """Contract B.  Returns (kkt dict, the largest |reported - recomputed|)."""
    k = k or kkt_ref.kkt(lp, r.x, r.y)
    assert abs(r.obj - k["pobj"]) <= 1e-9 * abs(k["pobj"]) + k["pobj_bound"], (what, r.obj, k["pobj"])
    worst = 0.0
    for got, name in ((r.primal_res_rel, "pres_rel"), (r.dual_res_rel, "dres_rel"), (r.gap_rel, "gap_rel")):
        d = abs(got - k[name])
        worst = max(worst, d)
        assert d <= SLACK * k[name] + k[name + "_bound"], (what, name, got, k[name], k[name + "_bound"])
    return k, worst


def check_optimal(lp, r, opt, what, eps=1e-6, eps_obj=1e-6, with_rdx=True, k=None):
    """Contract A.  Returns (kkt dict, max recomputed number / eps, max objective error / (1 + |opt|))."""
    assert r.status == 0, (what, r.status_name, r.iters)
    m_eq = int(lp["m_eq"])
    assert np.all(r.x >= lp["l"]) and np.all(r.x <= lp["u"]), what
    assert np.all(r.y[m_eq:] >= 0.0), what
    k = k or kkt_ref.kkt(lp, r.x, r.y)
    for name in ("pres_rel", "dres_rel", "gap_rel"):
        assert k[name] <= eps * (1 + SLACK) + k[name + "_bound"], (what, name, k[name], k[name + "_bound"])
    lhs, bound = kkt_ref.objective_gate(k, with_rdx)
    assert lhs <= eps_obj * (1 + abs(k["pobj"])) * (1 + SLACK) + bound, (what, "objective gate", lhs, k["pobj"], bound)
    err = max(abs(k["pobj"] - opt), abs(k["dobj"] - opt)) / (1 + abs(opt))
    assert err <= OBJ_BAR, (what, k["pobj"], k["dobj"], opt)
    return k, max(k["pres_rel"], k["dres_rel"], k["gap_rel"]) / eps, err


def check_both(lp, r, opt, what, form, **kw):
    """Contracts A and B on one OPTIMAL result; prints the figures profiles/result_contract.log collects."""
    k, ratio, err = check_optimal(lp, r, opt, what, **kw)
    _, diff = check_reported(lp, r, what, k=k)
    print(f"RESULT_CONTRACT form={form} case={what} iters={r.iters} ratio_to_eps={ratio:.3e} "
          f"reported_vs_recomputed={diff:.3e} objective_error={err:.3e}")
    return k
