"""Test infrastructure: the in-kernel Farkas test of ``dvh_options.certify = 2`` (csrc/dvh_kernels.hip pdhg_kernel,
csrc/dvh_band_grid.hip) restated in numpy, the bars a Farkas ray must pass, and the window population the early-exit
tests share.

``solve`` follows ``oracle.pdlp_ref.solve``'s loop (restarted reflected Halpern PDHG on the preconditioned LP, default
options) and, at every KKT check -- before the termination test -- puts the scaled dual y~ of T(z_k) through the
kernels' test.  With v = Dr y~ and kty = K~'y~ every term of the margin is scale-free:
    q'v              = sum_i q~_i y~_i
    bound term of j  = kty_j > 0 ? u~_j kty_j : l~_j kty_j           (finite bounds only)
    viol             = max |kty_j| / Dc_j over the columns whose bound on r_j's side is infinite
and the window is certified when margin > 0, viol <= 1e-8 margin and margin >= 1e-9 (sum |q~_i y~_i| + sum |bound
terms|) -- the constants and meaning of ``certify_ref._passes``.  The conditions are homogeneous in v; only a passing v
is normalised to ||v||_inf = 1, and its margin and violation are then evaluated on the unscaled window.
"""
import functools

import numpy as np
import scipy.sparse as sp

import certify_ref as cr
from oracle import pdlp_ref

OPTIMAL, PRIMAL_INFEASIBLE, ITER_LIMIT = pdlp_ref.OPTIMAL, pdlp_ref.PRIMAL_INFEASIBLE, pdlp_ref.ITER_LIMIT
KKT_PERIOD = pdlp_ref.DEFAULTS["check_every"] * pdlp_ref.DEFAULTS["kkt_every"]  # 128: iterations between KKT checks
EARLY_CAP = 4096   # every HiGHS-infeasible window of the population is certified within this many iterations
TS = (2, 3, 5, 25, 200, 768)
JS = (0, 1, 2)


def farkas_scaled(ys, kty, qt, lt, ut, Dc, m_eq):
    """The kernels' test of the scaled dual ys: (passes, margin, viol, scale), all in the units of v = Dr ys."""
    assert np.all(ys[m_eq:] >= 0.0)  # (the projection keeps the >= rows' duals there)
    qy = qt * ys
    pos, neg = kty > 0.0, kty < 0.0
    ufin, lfin = np.isfinite(ut), np.isfinite(lt)
    bt = np.zeros(len(kty))
    bt[pos & ufin] = ut[pos & ufin] * kty[pos & ufin]
    bt[neg & lfin] = lt[neg & lfin] * kty[neg & lfin]
    r = np.abs(kty) / Dc
    viol = max(np.max(r[pos & ~ufin], initial=0.0), np.max(r[neg & ~lfin], initial=0.0))
    margin = float(qy.sum() - bt.sum())
    scale = float(np.abs(qy).sum() + np.abs(bt).sum())
    return cr._passes(margin, viol, scale), margin, float(viol), scale


def solve(lp, max_iters=100000, early=True):
    """lp: a WindowLP.  dict(status, iters, x, y, margin, viol): status 1 with the normalised Farkas ray in y when the
    in-loop test passes (iters = the iteration of that KKT check), else pdlp_ref's own OPTIMAL / ITER_LIMIT result."""
    o = dict(pdlp_ref.DEFAULTS)
    o["max_iters"] = int(max_iters)
    o["check_every"] = max(1, min(o["check_every"], o["max_iters"]))
    K = sp.csr_matrix((lp.data, lp.indices, lp.indptr), shape=(lp.m, lp.n))
    m_eq = int(lp.m_eq)
    q, c, l, u = lp.q, lp.c, lp.l, lp.u
    Dr, Dc = pdlp_ref.precondition(K, o["ruiz_iters"])
    Kt = (sp.diags(Dr) @ K @ sp.diags(Dc)).tocsr()
    KtT = Kt.T.tocsr()
    ct, qt, lt, ut = Dc * c, Dr * q, l / Dc, u / Dc
    eta = o["step_safety"] / (pdlp_ref.power_norm(Kt, o["power_iters"]) if o["power_iters"] > 0 else 1.0)
    nc, nq = np.linalg.norm(ct), np.linalg.norm(qt)
    w = nc / nq if (nc > 1e-10 and nq > 1e-10) else 1.0
    q_norm, c_norm = np.linalg.norm(q), np.linalg.norm(c)
    fl, fu = np.isfinite(l), np.isfinite(u)

    def kkt_ok(xs, ys):
        x, y = Dc * xs, Dr * ys
        r = q - K @ x
        r[m_eq:] = np.maximum(r[m_eq:], 0.0)
        rc = c - K.T @ y
        lam = np.where(fl & fu, rc, np.where(fl, np.maximum(rc, 0), np.where(fu, np.minimum(rc, 0), 0.0)))
        rd = rc - lam
        pobj = c @ x + lp.c0
        dobj = q @ y + np.sum(np.where(fl, l, 0) * np.maximum(lam, 0)) + np.sum(np.where(fu, u, 0) * np.minimum(lam, 0)) \
            + lp.c0
        pres, dres = np.linalg.norm(r), np.linalg.norm(rd)
        gap = abs(pobj - dobj) / (1 + abs(pobj) + abs(dobj))
        ok = pres / (1 + q_norm) <= o["eps"] and dres / (1 + c_norm) <= o["eps"] and gap <= o["eps"]
        return ok and abs(pobj - dobj) + np.linalg.norm(y) * pres + float(np.sum(np.abs(rd) * np.abs(x))) \
            <= o["eps_obj"] * (1.0 + abs(pobj))

    x = np.clip(np.zeros(lp.n), lt, ut)
    y = np.zeros(lp.m)
    xa, ya = x.copy(), y.copy()
    k, it, r0, r_prev, status = 0, 0, None, None, ITER_LIMIT
    last = (x, y)
    while it < o["max_iters"]:
        tau, sigma = eta / w, eta * w
        xp = np.clip(x - tau * (ct - KtT @ y), lt, ut)
        yp = y + sigma * (qt - Kt @ (2 * xp - x))
        yp[m_eq:] = np.maximum(yp[m_eq:], 0.0)
        it += 1
        if it % o["check_every"] == 0:
            dx, dy = x - xp, y - yp
            r = np.sqrt(w * (dx @ dx) + (dy @ dy) / w)
            if it % (o["check_every"] * o["kkt_every"]) == 0 or it + o["check_every"] > o["max_iters"]:
                last = (xp, yp)
                if early:
                    ok, _, _, _ = farkas_scaled(yp, KtT @ yp, qt, lt, ut, Dc, m_eq)
                    if ok:
                        v = Dr * yp
                        v = v / np.max(np.abs(v))
                        margin, viol = cr.farkas(lp, v)
                        return dict(status=PRIMAL_INFEASIBLE, iters=it, x=Dc * xp, y=v, margin=margin, viol=viol)
                if kkt_ok(xp, yp):
                    status = OPTIMAL
                    break
            if r0 is None:
                r0 = r
            restart = (r <= o["b_suff"] * r0) or (r <= o["b_nec"] * r0 and r_prev is not None and r > r_prev) \
                or (k + 1 >= o["b_art"] * it)
            if restart:
                ddx, ddy = np.linalg.norm(xp - xa), np.linalg.norm(yp - ya)
                if ddx > 1e-10 and ddy > 1e-10:
                    w = ddy / ddx  # (theta = 1)
                x, y = xp, yp
                xa, ya = xp.copy(), yp.copy()
                k, r0, r_prev = 0, r, None
                continue
            r_prev = r
        cb = 1.0 / (k + 2)
        x = (1.0 - cb) * (2.0 * xp - x) + cb * xa
        y = (1.0 - cb) * (2.0 * yp - y) + cb * ya
        k += 1
    xs, ys = last
    return dict(status=status, iters=it, x=Dc * xs, y=Dr * ys, margin=0.0, viol=0.0)


def farkas_bars(lp, y, reported_margin=None):
    """The bars of a returned Farkas ray, recomputed in numpy: margin > 0, viol <= 1e-8 margin, ||y||_inf = 1 to 1e-12,
    >= rows >= 0 and, where given, the reported margin within 1e-9 relative of numpy's.  Returns (margin, viol)."""
    margin, viol = cr.farkas(lp, y)
    assert margin > 0.0 and viol <= 1e-8 * margin, (margin, viol)
    assert abs(np.max(np.abs(y)) - 1.0) <= 1e-12 and np.all(y[lp.m_eq:] >= 0.0)
    if reported_margin is not None:
        assert abs(reported_margin - margin) <= 1e-9 * margin, (reported_margin, margin)
    return margin, viol


# ---- the population: certify_ref.poi_window over T x J x the six kinds x PV on / off; "feasible" and "min_soe" also
#      without POI rows.  A key is poi_window's arguments (T, J, kind, ("pv", bool), ("poi", bool)).
def keys_of(T, J, pv):
    return [(T, J, kind, ("pv", pv), ("poi", True)) for kind in cr.KINDS]


def keys_no_poi(T, J, pv):
    return [(T, J, kind, ("pv", pv), ("poi", False)) for kind in ("feasible", "min_soe")]


@functools.lru_cache(maxsize=None)
def window(key):
    return cr.poi_window(*key[:3], **dict(key[3:]))


@functools.lru_cache(maxsize=None)
def highs(key):
    return cr.highs_status(window(key))


@functools.lru_cache(maxsize=None)
def restated(key, max_iters=100000):
    """The restatement's result for an infeasible window of the population, computed once per session."""
    return solve(window(key), max_iters=max_iters)
