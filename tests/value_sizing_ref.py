"""CPU references of the economic sizing (dervet_hip/value_sizing.py): the battery window of a device-builder spec as
a host LP (the layout of csrc/dvh_build.hip), HiGHS on it with duals, the monolithic relaxed sizing LP
    min c_E E + c_P P + c_fix + alpha sum_w (c_w'x_w + c0_w)
    s.t. every window's rows with soc_target E moved to the left, P - ch_t >= 0, P - dis_t >= 0,
         ene_t - llsoc E >= 0, ulsoc E - ene_t >= 0 (ene_t <= emax_t stays a bound), E and P in their boxes,
and the cutting-plane loop restated with HiGHS duals and a HiGHS master (value_sizing.loop_host)."""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import linprog

from dervet_hip import value_sizing as VS


def window_lp(s, k, E, P):
    """Row k of the BatteryGroupSpec ``s`` at the rating (E, pch = pdis = P) as a host LP, entry for entry what the
    device builder writes (no ICE, no emin)."""
    T, J, dt = s.T, s.J, s.dt
    dcm_t, dcm_j = np.asarray(s.dcm_t, np.int64), np.asarray(s.dcm_j, np.int64)
    mI = len(dcm_t)
    n, m, nnz = 3 * T + J, T + 1 + mI, 4 * T + 3 * mI
    eta, sdr = float(s.scal["rte"][k]), float(s.scal["sdr"][k])
    target = float(s.scal["soc_target"][k]) * E
    fin, dcm0 = 1 + 4 * (T - 1), 1 + 4 * (T - 1) + 3
    ip = np.zeros(m + 1, np.int64)
    ip[1:T + 1] = 1 + 4 * np.arange(T)
    ip[T + 1:] = dcm0 + 3 * np.arange(mI + 1)
    ix, dv = np.zeros(nnz, np.int64), np.zeros(nnz)
    ix[0], dv[0] = 2 * T, 1.0
    t = np.arange(T - 1)
    p = 1 + 4 * t
    ix[p], ix[p + 1], ix[p + 2], ix[p + 3] = t, T + t, 2 * T + t, 2 * T + t + 1
    dv[p], dv[p + 1], dv[p + 2], dv[p + 3] = -dt * eta, dt, -(1.0 - dt * sdr), 1.0
    ix[fin:fin + 3] = [T - 1, 2 * T - 1, 3 * T - 1]
    dv[fin:fin + 3] = [dt * eta, -dt, 1.0 - dt * sdr]
    pi = dcm0 + 3 * np.arange(mI)
    ix[pi], ix[pi + 1], ix[pi + 2] = dcm_t, T + dcm_t, 3 * T + dcm_j
    dv[pi], dv[pi + 1], dv[pi + 2] = -1.0, 1.0, 1.0
    q = np.zeros(m)
    q[0] = q[T] = target
    q[T + 1:] = s.base[k][dcm_t]
    l, u = np.zeros(n), np.zeros(n)
    u[:T], u[T:2 * T] = P, P
    l[2 * T:3 * T] = float(s.scal["llsoc"][k]) * E
    hi = np.full(T, float(s.scal["ulsoc"][k]) * E)
    u[2 * T:3 * T] = hi if s.emax is None else np.minimum(hi, s.emax[k])
    l[3 * T:], u[3 * T:] = -np.inf, np.inf
    c = np.zeros(n)
    for price in (s.da, s.retail):
        if price is not None:
            c[:T] += price[k] * dt
            c[T:2 * T] += -price[k] * dt
    c[T:2 * T] += float(s.scal["om"][k]) / 1000.0 * dt
    if J:
        c[3 * T:] = s.demand[k]
    K = sp.csr_matrix((dv, ix, ip), shape=(m, n))
    return dict(T=T, J=J, mI=mI, dcm_t=dcm_t, dcm_j=dcm_j, K=K, dv=dv, q=q, c=c, l=l, u=u, c0=float(s.c0[k]), m_eq=T + 1,
                E=E, P=P, soc_target=float(s.scal["soc_target"][k]), llsoc=float(s.scal["llsoc"][k]),
                ulsoc=float(s.scal["ulsoc"][k]), emax=None if s.emax is None else np.asarray(s.emax[k]))


def solve_highs(lp):
    """HiGHS on a window: obj (with c0), x, y (equality duals, then the >= rows' duals, non-negative), ok."""
    K, me = lp["K"], lp["m_eq"]
    bounds = [(None if np.isneginf(a) else a, None if np.isposinf(b) else b) for a, b in zip(lp["l"], lp["u"])]
    r = linprog(lp["c"], A_ub=-K[me:] if K.shape[0] > me else None, b_ub=-lp["q"][me:] if K.shape[0] > me else None,
                A_eq=K[:me], b_eq=lp["q"][:me], bounds=bounds, method="highs")
    if r.status != 0:
        return dict(ok=False, obj=np.nan, x=None, y=None, status=r.status)
    y = np.concatenate([r.eqlin.marginals, -r.ineqlin.marginals if K.shape[0] > me else np.zeros(0)])
    return dict(ok=True, obj=float(r.fun) + lp["c0"], x=r.x, y=y, status=0)


def cut_of(lp, x, y):
    """The cut record of a window LP and a primal / dual pair (value_sizing.host_cut)."""
    return VS.host_cut(lp["T"], lp["J"], lp["dcm_t"], lp["dcm_j"], lp["dv"], lp["c"], lp["l"], lp["u"], lp["q"], x, y,
                       lp["c0"], lp["E"], lp["P"], lp["soc_target"], lp["llsoc"], lp["ulsoc"], lp["emax"])


def value_at(positions, k, E, P):
    """sum_w V_w(E, P) of case k by HiGHS (NaN when a window is infeasible)."""
    tot = 0.0
    for s in positions:
        h = solve_highs(window_lp(s, k, E, P))
        if not h["ok"]:
            return np.nan
        tot += h["obj"]
    return tot


def evaluate_highs(positions, k):
    """``evaluate`` of value_sizing.loop_host with HiGHS primal / dual pairs."""
    def ev(E, P):
        V = a = ge = gp = 0.0
        for s in positions:
            lp = window_lp(s, k, E, P)
            h = solve_highs(lp)
            if not h["ok"]:
                return 0.0, 0.0, 0.0, 0.0, False
            cut = cut_of(lp, h["x"], h["y"])
            V, a, ge, gp = V + h["obj"], a + cut[VS.A], ge + cut[VS.GE], gp + cut[VS.GP]
        return V, a, ge, gp, True
    return ev


def monolithic(positions, k, spec):
    """The relaxed sizing LP of case k in one piece: dict(E, P, obj, ok)."""
    elo, ehi, plo, phi = spec.box()
    blocks, rows_E, rows_P, rhs, eq, cost, lo, up = [], [], [], [], [], [0.0, 0.0], [elo, plo], [ehi, phi]
    const = spec.ccost
    for s in positions:
        lp = window_lp(s, k, 1.0, 1.0)  # (q at E = 1: the rating's coefficient)
        T, n, m = lp["T"], lp["K"].shape[1], lp["K"].shape[0]
        eye = sp.identity(T, format="csr")
        zero = sp.csr_matrix((T, T))
        ztau = sp.csr_matrix((T, lp["J"]))
        extra = sp.vstack([sp.hstack([-eye, zero, zero, ztau]), sp.hstack([zero, -eye, zero, ztau]),
                           sp.hstack([zero, zero, eye, ztau]), sp.hstack([zero, zero, -eye, ztau])]).tocsr()
        blocks.append(sp.vstack([lp["K"], extra]).tocsr())
        cE = np.zeros(m + 4 * T)
        cE[0] = cE[T] = -lp["soc_target"]
        cE[m + 2 * T:m + 3 * T] = -lp["llsoc"]
        cE[m + 3 * T:m + 4 * T] = lp["ulsoc"]
        cP = np.zeros(m + 4 * T)
        cP[m:m + 2 * T] = 1.0
        q = lp["q"].copy()
        q[0] = q[T] = 0.0
        rows_E.append(cE)
        rows_P.append(cP)
        rhs.append(np.concatenate([q, np.zeros(4 * T)]))
        eq.append(np.concatenate([np.ones(lp["m_eq"], bool), np.zeros(m - lp["m_eq"] + 4 * T, bool)]))
        cost.extend(spec.alpha * lp["c"])
        wl, wu = lp["l"].copy(), lp["u"].copy()
        wl[:3 * T] = 0.0
        wu[:2 * T] = np.inf
        wu[2 * T:3 * T] = np.inf if lp["emax"] is None else lp["emax"]
        lo.extend(wl)
        up.extend(wu)
        const += spec.alpha * lp["c0"]
    A = sp.hstack([sp.csr_matrix(np.concatenate(rows_E)[:, None]), sp.csr_matrix(np.concatenate(rows_P)[:, None]),
                   sp.block_diag(blocks)]).tocsr()
    b, eq = np.concatenate(rhs), np.concatenate(eq)
    cost = np.array(cost)
    cost[0], cost[1] = spec.c_energy, spec.c_power
    bounds = [(None if np.isneginf(a) else a, None if np.isposinf(c) else c) for a, c in zip(lo, up)]
    r = linprog(cost, A_ub=-A[~eq], b_ub=-b[~eq], A_eq=A[eq], b_eq=b[eq], bounds=bounds, method="highs")
    if r.status != 0:
        return dict(ok=False, E=np.nan, P=np.nan, obj=np.nan)
    return dict(ok=True, E=float(r.x[0]), P=float(r.x[1]), obj=float(r.fun) + const)


def objective_at(positions, k, spec, E, P):
    """F(E, P) of case k with HiGHS window optima."""
    return ((spec.c_energy * E + spec.c_power * P) + spec.alpha * value_at(positions, k, E, P)) + spec.ccost


U = 2.0 ** -53


def longdouble_cut(lp, x, y):
    """a, gE, gP, D, pobj in long double, straight sums; and the magnitude the rounding bound scales with."""
    L = np.longdouble
    T, J = lp["T"], lp["J"]
    yy = np.array(y, L)
    yy[T + 1:] = np.maximum(yy[T + 1:], 0)
    Kc = lp["K"].tocoo()
    kty = np.zeros(len(x), L)
    mag = np.zeros(len(x), L)   # |c_j| + sum_i |K_ij y_i|: what r_j's rounding error scales with
    np.add.at(kty, Kc.col, Kc.data.astype(L) * yy[Kc.row])
    np.add.at(mag, Kc.col, np.abs(Kc.data.astype(L) * yy[Kc.row]))
    c, l, u = lp["c"].astype(L), lp["l"].astype(L), lp["u"].astype(L)
    r = c - kty
    mag += np.abs(c)
    lo = np.where(np.isfinite(lp["l"]), l, 0)
    hi = np.where(np.isfinite(lp["u"]), u, 0)
    bound = np.where(r > 0, lo * r, hi * r)
    D = (lp["q"].astype(L) * yy).sum() + bound.sum() + L(lp["c0"])
    rene, rch, rdis = r[2 * T:3 * T], r[:T], r[T:2 * T]
    act = np.ones(T, bool) if lp["emax"] is None else lp["ulsoc"] * lp["E"] <= lp["emax"]
    gE = L(lp["soc_target"]) * (yy[0] + yy[T]) + (L(lp["llsoc"]) * np.maximum(rene, 0)).sum() + \
        (L(lp["ulsoc"]) * np.minimum(rene, 0) * act).sum()
    gP = np.minimum(rch, 0).sum() + np.minimum(rdis, 0).sum()
    a = D - gE * L(lp["E"]) - gP * L(lp["P"])
    pobj = (c * np.array(x, L)).sum() + L(lp["c0"])
    bmax = np.maximum(np.abs(lo), np.abs(hi))
    scale = float(np.abs(lp["q"] * y).sum() + (bmax * mag).sum() + abs(lp["c0"]))
    gscale = float(mag.sum() + abs(yy[0]) + abs(yy[T]))
    return np.array([a, gE, gP, D, pobj], L), scale, gscale, float(np.abs(c * x).sum() + abs(lp["c0"]))


def assert_within_rounding(got, lp, x, y):
    """A cut record against the long-double sums.  Forward bound: every term goes through <= 6 roundings before the
    sums, a lane's chain is ceil(m / 256) + 3 long, the trees 6 + 3 deep, the tau tail J: k u times the sum of the
    terms' magnitudes."""
    ref, scale, gscale, cscale = longdouble_cut(lp, x, y)
    m = len(y)
    k = (6 + -(-m // 256) + 3 + 9 + lp["J"] + 4) * U
    sizes = abs(lp["E"]) + abs(lp["P"]) + 1.0
    print(f"|dD| {abs(float(got[VS.DOBJ] - ref[3])):.3e} bound {k * scale:.3e}; |dgE| {abs(float(got[VS.GE] - ref[1])):.3e} "
          f"|dgP| {abs(float(got[VS.GP] - ref[2])):.3e} bound {k * gscale:.3e}")
    assert abs(float(got[VS.DOBJ] - ref[3])) <= k * scale
    assert abs(float(got[VS.GE] - ref[1])) <= k * gscale and abs(float(got[VS.GP] - ref[2])) <= k * gscale
    assert abs(float(got[VS.A] - ref[0])) <= k * (scale + gscale * sizes) + 4 * U * (abs(float(ref[3])) + gscale * sizes)
    assert abs(float(got[VS.POBJ] - ref[4])) <= k * cscale
