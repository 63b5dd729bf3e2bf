"""Test infrastructure: the certificate pass of csrc/dvh_certify.hip restated in numpy, the two certificate tests on
their own, and the window population the certificate tests share.

The pass runs plain PDHG on the unscaled window LP
    min c'x  s.t.  K_E x = q_E,  K_I x >= q_I,  l <= x <= u
from a cold start (x = proj_[l,u](0), y = 0) with the diagonal Pock-Chambolle steps tau_j = 1 / sum_i |K_ij|,
sigma_i = 1 / sum_j |K_ij| (1 for an empty column / row):
    x+ = proj(x - tau (c - K'y)),   y+ = y + sigma (q - K (2 x+ - x)),  the >= rows' y clamped at 0.
On an infeasible LP both z_k - z_0 and z_{k+1} - z_k converge to the infimal displacement vector, whose dual part is
a Farkas certificate and whose primal part an unbounded ray; every CHECK iterations the pass tests, in this order,
y_k, y_k - y_{k-1} (Farkas), x_k - x_0, x_k - x_{k-1} (ray) and stops at the first that passes.

  farkas(lp, y) -> (margin, viol): for any feasible x, y'q <= y'Kx = r'x <= sum_j (r_j > 0 ? u_j r_j : l_j r_j) with
      r = K'y; margin = q'y minus that sum over the finite bounds, viol = the largest r_j on the wrong side of an
      infinite bound.  margin > 0 with viol = 0 proves the window infeasible.
  ray(lp, d) -> (descent, viol): descent = -c'd, viol = max(||K_E d||_inf, ||(K_I d)^-||_inf); d (sign-constrained by
      the finite bounds) with descent > 0 and viol = 0 is a direction of unbounded descent.
"""
import numpy as np
import scipy.optimize
import scipy.sparse as sp

from dervet_hip.lp import builder
from dervet_hip.solver import WindowLP

CHECK = 64           # iterations between certificate tests
CAP = 65536          # default iteration cap (dvh_options.certify_iters = 0)
RAY_TOL = 1e-8       # viol <= RAY_TOL * margin (PDLP's default ray tolerance)
FLOOR = 1e-9         # margin >= FLOOR * (sum of the absolute terms it is the difference of)
PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, UNDECIDED = 1, 2, 5


def _K(lp):
    return sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))


def farkas_terms(lp, y, K=None):
    """(margin, viol, sum of the absolute terms of margin) of the Farkas candidate y, taken as given."""
    K = _K(lp) if K is None else K
    y = np.asarray(y, np.float64)
    r = K.T @ y
    pos, neg = r > 0.0, r < 0.0
    ufin, lfin = np.isfinite(lp.u), np.isfinite(lp.l)
    viol = max(np.max(r[pos & ~ufin], initial=0.0), np.max(-r[neg & ~lfin], initial=0.0))
    bt = np.zeros(lp.n)
    bt[pos & ufin] = lp.u[pos & ufin] * r[pos & ufin]
    bt[neg & lfin] = lp.l[neg & lfin] * r[neg & lfin]
    qy = lp.q * y
    return float(qy.sum() - bt.sum()), float(viol), float(np.abs(qy).sum() + np.abs(bt).sum())


def farkas(lp, y):
    m, v, _ = farkas_terms(lp, y)
    return m, v


def ray_terms(lp, d, K=None):
    K = _K(lp) if K is None else K
    d = np.asarray(d, np.float64)
    a = K @ d
    viol = max(np.max(np.abs(a[:lp.m_eq]), initial=0.0), np.max(-a[lp.m_eq:], initial=0.0))
    cd = lp.c * d
    return float(-cd.sum()), float(viol), float(np.abs(cd).sum())


def ray(lp, d):
    m, v, _ = ray_terms(lp, d)
    return m, v


def _passes(margin, viol, scale):
    return margin > 0.0 and viol <= RAY_TOL * margin and margin >= FLOOR * scale


def _farkas_candidate(lp, v, K):
    v = v.copy()
    v[lp.m_eq:] = np.maximum(v[lp.m_eq:], 0.0)
    nrm = np.max(np.abs(v), initial=0.0)
    if not (nrm > 0.0 and np.isfinite(nrm)):
        return None
    v = v / nrm
    margin, viol, scale = farkas_terms(lp, v, K)
    return (v, margin, viol) if _passes(margin, viol, scale) else None


def _ray_candidate(lp, d, K):
    d = d.copy()
    lfin, ufin = np.isfinite(lp.l), np.isfinite(lp.u)
    d[lfin] = np.maximum(d[lfin], 0.0)
    d[ufin] = np.minimum(d[ufin], 0.0)
    nrm = np.max(np.abs(d), initial=0.0)
    if not (nrm > 0.0 and np.isfinite(nrm)):
        return None
    d = d / nrm
    margin, viol, scale = ray_terms(lp, d, K)
    return (d, margin, viol) if _passes(margin, viol, scale) else None


def certify(lp, cap=CAP):
    """The kernel's pass: dict(status 1 / 2 / 5, iters, ray (y for 1, x-direction for 2, else None), margin, viol)."""
    K = _K(lp)
    Kt = K.T.tocsr()
    A = abs(K)
    cs, rs = np.asarray(A.sum(axis=0)).ravel(), np.asarray(A.sum(axis=1)).ravel()
    tau = np.where(cs > 0.0, 1.0 / np.where(cs > 0.0, cs, 1.0), 1.0)
    sig = np.where(rs > 0.0, 1.0 / np.where(rs > 0.0, rs, 1.0), 1.0)
    x0 = np.minimum(np.maximum(0.0, lp.l), lp.u)
    x, y = x0.copy(), np.zeros(lp.m)
    for k in range(1, int(cap) + 1):
        xn = np.minimum(np.maximum(x - tau * (lp.c - Kt @ y), lp.l), lp.u)
        yn = y + sig * (lp.q - K @ (2.0 * xn - x))
        yn[lp.m_eq:] = np.maximum(yn[lp.m_eq:], 0.0)
        dx, dy = xn - x, yn - y
        x, y = xn, yn
        if k % CHECK:
            continue
        for cand in (y, dy):
            got = _farkas_candidate(lp, cand, K)
            if got:
                return dict(status=PRIMAL_INFEASIBLE, iters=k, ray=got[0], margin=got[1], viol=got[2])
        for cand in (x - x0, dx):
            got = _ray_candidate(lp, cand, K)
            if got:
                return dict(status=DUAL_INFEASIBLE, iters=k, ray=got[0], margin=got[1], viol=got[2])
    return dict(status=UNDECIDED, iters=int(cap) - int(cap) % CHECK, ray=None, margin=0.0, viol=0.0)


def highs_status(lp):
    """scipy.optimize.linprog(method="highs") status of the window: 0 optimal, 2 infeasible, 3 unbounded."""
    K = _K(lp)
    me = lp.m_eq
    bounds = [(None if np.isneginf(a) else a, None if np.isposinf(b) else b) for a, b in zip(lp.l, lp.u)]
    r = scipy.optimize.linprog(lp.c, A_ub=-K[me:] if lp.m > me else None, b_ub=-lp.q[me:] if lp.m > me else None,
                               A_eq=K[:me] if me else None, b_eq=lp.q[:me] if me else None, bounds=bounds,
                               method="highs")
    return int(r.status), (float(r.fun) + lp.c0 if r.status == 0 else None)


def expected_status(highs):
    """The certificate pass's status for a window of that HiGHS status."""
    return {0: UNDECIDED, 2: PRIMAL_INFEASIBLE, 3: DUAL_INFEASIBLE}[highs]


# ---- the tiny LPs
def _lp(rows, q, c, l, u, m_eq):
    return WindowLP.from_csr(sp.csr_matrix(np.asarray(rows, np.float64)), q, c, l, u, m_eq)


def tiny(kind):
    inf = np.inf
    if kind == "infeasible":       # x0 + x1 = 3 inside the unit box
        return _lp([[1.0, 1.0]], [3.0], [1.0, 2.0], [0.0, 0.0], [1.0, 1.0], 1)
    if kind == "infeasible_twin":  # x0 + x1 = 1.5: optimum 2 at (1, 0.5)
        return _lp([[1.0, 1.0]], [1.5], [1.0, 2.0], [0.0, 0.0], [1.0, 1.0], 1)
    if kind == "unbounded":        # min -x0, x0 = x1, no upper bound
        return _lp([[1.0, -1.0]], [0.0], [-1.0, 0.0], [0.0, 0.0], [inf, inf], 1)
    if kind == "unbounded_twin":   # the same below x <= 4: optimum -4
        return _lp([[1.0, -1.0]], [0.0], [-1.0, 0.0], [0.0, 0.0], [4.0, 4.0], 1)
    raise KeyError(kind)


TINY_OBJ = {"infeasible_twin": 2.0, "unbounded_twin": -4.0}

# ---- POI windows (builder.battery_group), feasible and infeasible for the reasons a sensitivity sweep meets
BAT = dict(E=2000.0, Pch=500.0, Pdis=500.0, rte=0.9, sdr=0.0, soc_target=0.5, ulsoc=1.0, llsoc=0.1, fixedOM=1.0,
           OMexpenses=0.0, hp=0.0)
POI = dict(max_import=-650.0, max_export=0.0)
KINDS = ("feasible", "overload", "short", "margin_in", "margin_out", "min_soe")


def poi_window(T, J, kind, pv=False, poi=True, seed=0, dense=False):
    """One window: the load stays below the import limit except
      overload   : one step asks for more than the import limit plus the discharge rating;
      short      : every step needs some discharge, and the window must end at its starting SOE;
      margin_in / margin_out : the first min(8, T - 1) steps draw 92 % / 108 % of the energy above the SOE floor;
      min_soe    : an energy lower bound at step 1 that the charger cannot reach from the start (not crossed).
    dense: every demand period covers every step (T demand-charge rows per period) instead of every (J + 1)-th."""
    rng = np.random.default_rng(7919 * T + 31 * J + KINDS.index(kind) + 1000003 * seed)
    t = np.arange(T)
    load = rng.uniform(400.0, 600.0, T)
    emin = None
    if kind == "overload":
        load[T // 2] = 650.0 + 500.0 + 150.0
    elif kind == "short":
        load[:] = rng.uniform(660.0, 700.0, T)
    elif kind in ("margin_in", "margin_out"):
        h = min(8, T - 1)
        load[:h] = 650.0 + (1.08 if kind == "margin_out" else 0.92) * 800.0 / h
    elif kind == "min_soe":
        emin = np.zeros((1, T))
        emin[0, 1] = 1000.0 + 0.9 * 500.0 + 150.0
    kw = {}
    if poi:
        kw["poi"] = POI
    if pv:  # a little curtailable PV: less than the discharge the infeasible kinds are short of
        kw["pv_curtail_max"] = (5.0 + 20.0 * np.sin(np.pi * (t + 0.5) / T))[None]
    masks = np.array([(t % (J + 1) == j) | dense for j in range(J)], bool).reshape(J, T)
    g = builder.battery_group(T, 1.0, load[None], BAT, retail_price=rng.uniform(0.05, 0.15, (1, T)),
                              demand_masks=masks if J else None,
                              demand_prices=rng.uniform(8.0, 20.0, (1, J)) if J else None, ene_min=emin, **kw)
    return builder.group_window_lps(g)[0]
