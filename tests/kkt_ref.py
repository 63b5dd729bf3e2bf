"""Host reference of the result contract (include/dervet_hip.h dvh_result): the relative KKT numbers of a point
(x, y) of a window LP, recomputed from the LP's own data.  Test infrastructure only.

    LP:   min c'x + c0   s.t.  K[:m_eq] x = q[:m_eq],  K[m_eq:] x >= q[m_eq:],  l <= x <= u

    r_p   = q - K x, the >= rows' entries clipped at 0 (a satisfied >= row has no residual)
    rc    = c - K'y
    lam   = the part of rc the bounds can carry: rc (boxed), max(rc, 0) (lower only), min(rc, 0) (upper only), 0 (free)
    r_d   = rc - lam
    pobj  = c'x + c0
    dobj  = q'y + sum_j l_j max(lam_j, 0) + sum_j u_j min(lam_j, 0) + c0        (finite bounds only)
    pres_rel = ||r_p||_2 / (1 + ||q||_2),  dres_rel = ||r_d||_2 / (1 + ||c||_2),
    gap_rel  = |pobj - dobj| / (1 + |pobj| + |dobj|),  rdx = sum_j |r_d,j| |x_j|,  ynorm = ||y||_2,  pres = ||r_p||_2

These are the header's definitions and those of oracle/pdlp_ref.py's kkt, written a second time on purpose: no scaling,
no shared code, np.longdouble arithmetic with compensated (Neumaier) accumulation of every sum.

Every number comes with a forward rounding bound ``<name>_bound``: what a double-precision evaluation of the same
expression, in any summation order, can differ from the exact value by.  A sum of `len` terms t_k evaluated in double
precision is off by at most gamma * sum |t_k| with gamma = (len + 2) 2^-53 (len - 1 additions, one rounding per
product, one spare); the bounds below are those sums over the data, pushed through the 1-Lipschitz clip / projection
and the 2-norm (| ||a|| - ||b|| | <= ||a - b||).  The GPU tests use them as their absolute slack.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53


def gamma(length):
    return (np.asarray(length, LD) + 2) * LD(U)


def _sum(v):
    """Neumaier-compensated sum of a longdouble vector."""
    s = LD(0)
    comp = LD(0)
    for t in np.asarray(v, LD).ravel():
        a = s + t
        comp += (s - a) + t if abs(s) >= abs(t) else (t - a) + s
        s = a
    return s + comp


def _rows(K, v):
    """Per row of the CSR K: (sum_k K_ik v_k, sum_k |K_ik v_k|, entries), in longdouble; an empty row gives 0."""
    K = sp.csr_matrix(K)
    m = K.shape[0]
    prod = K.data.astype(LD) * np.asarray(v, LD)[K.indices]
    s = np.zeros(m, LD)
    a = np.zeros(m, LD)
    lens = np.diff(K.indptr)
    for i in np.nonzero(lens)[0]:
        p = prod[K.indptr[i]:K.indptr[i + 1]]
        s[i] = _sum(p) if len(p) > 8 else p.sum()
        a[i] = np.abs(p).sum()
    return s, a, lens


def _norm(v):
    return np.sqrt(_sum(np.asarray(v, LD) ** 2))


def kkt(lp, x, y):
    """lp: the oracle dict (K, q, c, c0, l, u, m_eq).  Returns the dict described in the module docstring (floats)."""
    K = sp.csr_matrix(lp["K"])
    m, n = K.shape
    m_eq = int(lp["m_eq"])
    q, c, l, u = (np.asarray(lp[k], float) for k in ("q", "c", "l", "u"))
    c0 = LD(float(lp.get("c0", 0.0)))
    x = np.asarray(x, float)
    y = np.asarray(y, float)
    assert x.shape == (n,) and y.shape == (m,) and q.shape == (m,) and c.shape == (n,)
    xl, yl, ql, cl = x.astype(LD), y.astype(LD), q.astype(LD), c.astype(LD)

    # primal side
    kx, kx_abs, rlen = _rows(K, x)
    r = ql - kx
    r_err = gamma(rlen + 1) * (np.abs(ql) + kx_abs)
    r[m_eq:] = np.maximum(r[m_eq:], 0)
    pres = _norm(r)
    pres_b = _norm(r_err) + gamma(m) * pres
    qn, cn = _norm(ql), _norm(cl)
    pres_rel = pres / (1 + qn)
    pres_rel_b = pres_b / (1 + qn) + (gamma(m) + 4 * LD(U)) * pres_rel

    # dual side
    kty, kty_abs, clen = _rows(K.T.tocsr(), y)
    rc = cl - kty
    rc_err = gamma(clen + 1) * (np.abs(cl) + kty_abs)
    fl, fu = np.isfinite(l), np.isfinite(u)
    lam = np.where(fl & fu, rc, np.where(fl, np.maximum(rc, 0), np.where(fu, np.minimum(rc, 0), LD(0))))
    rd = rc - lam
    dres = _norm(rd)
    dres_b = _norm(rc_err) + gamma(n) * dres
    dres_rel = dres / (1 + cn)
    dres_rel_b = dres_b / (1 + cn) + (gamma(n) + 4 * LD(U)) * dres_rel

    # objectives
    cx = cl * xl
    pobj = _sum(cx) + c0
    pobj_b = gamma(n + 1) * (_sum(np.abs(cx)) + abs(c0))
    qy = ql * yl
    lo = np.where(fl, l, 0.0).astype(LD)
    hi = np.where(fu, u, 0.0).astype(LD)
    bl = lo * np.maximum(lam, 0)
    bu = hi * np.minimum(lam, 0)
    dobj = _sum(qy) + _sum(bl) + _sum(bu) + c0
    # lam is 1-Lipschitz in rc, so a column's bound term moves by at most max(|l|, |u|) rc_err
    dobj_b = gamma(m + 2 * n + 1) * (_sum(np.abs(qy)) + _sum(np.abs(bl)) + _sum(np.abs(bu)) + abs(c0)) + \
        _sum(np.maximum(np.abs(lo), np.abs(hi)) * rc_err)
    den = 1 + abs(pobj) + abs(dobj)
    gap_rel = abs(pobj - dobj) / den
    gap_rel_b = 2 * (pobj_b + dobj_b) / den + 4 * LD(U) * gap_rel  # numerator and denominator both move by <= the sum

    rdx = _sum(np.abs(rd) * np.abs(xl))
    rdx_b = _sum(rc_err * np.abs(xl)) + gamma(n) * rdx
    ynorm = _norm(yl)
    ynorm_b = (gamma(m) + 2 * LD(U)) * ynorm

    out = dict(pres_rel=pres_rel, dres_rel=dres_rel, gap_rel=gap_rel, pobj=pobj, dobj=dobj, rdx=rdx, ynorm=ynorm,
               pres=pres, pres_rel_bound=pres_rel_b, dres_rel_bound=dres_rel_b, gap_rel_bound=gap_rel_b,
               pobj_bound=pobj_b, dobj_bound=dobj_b, rdx_bound=rdx_b, ynorm_bound=ynorm_b, pres_bound=pres_b)
    return {k: float(v) for k, v in out.items()}


def objective_gate(k, with_rdx=True):
    """(left side, its rounding bound) of the objective gate |pobj - dobj| + ||y|| ||r_p|| + rdx <= eps_obj (1 + |pobj|)
    (csrc/dvh_device.h kkt_done) from a kkt() dict; with_rdx = False: the band ICE form's gate, which omits rdx."""
    lhs = abs(k["pobj"] - k["dobj"]) + k["ynorm"] * k["pres"] + (k["rdx"] if with_rdx else 0.0)
    b = k["pobj_bound"] + k["dobj_bound"] + k["ynorm"] * k["pres_bound"] + k["ynorm_bound"] * (k["pres"] + k["pres_bound"]) \
        + (k["rdx_bound"] if with_rdx else 0.0)
    return lhs, b
