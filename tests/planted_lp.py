"""LPs built backwards from a chosen primal-dual optimum, so that their optimal value is known without a solver.
Test infrastructure only.

    LP:   min c'x + c0   s.t.  K[:m_eq] x = q[:m_eq],  K[m_eq:] x >= q[m_eq:],  l <= x <= u

Choose x* inside [l, u], duals y* (any sign on equality rows; on a >= row either y* > 0 and no slack, or y* = 0 and a
positive slack) and reduced costs lam* (> 0 on a column at its lower bound, < 0 at its upper bound, 0 on an interior
column), then set  q = K x* - slack,  c = K'y* + lam*.  (x*, y*) satisfies the KKT conditions with strict
complementarity, so it is optimal and the optimal value is c'x* + c0.

``planted`` draws the matrix as well: a shifted band whose row lengths are bounded by wy and whose column lengths are
bounded by wx (the ELL instantiations are chosen by both), plus optional long rows / columns, empty columns and empty
>= rows.  Every active row (equality rows and >= rows with y* > 0) owns one pivot column, which is interior; every
other column sits at a bound.  The pivot entry dominates its row's other interior entries, so the square matrix
K[active rows, interior columns] is strictly diagonally dominant after a column permutation, hence non-singular: the
optimal x* (the active rows determine the interior columns) and y* (the interior columns' rc = 0 determines the active
rows' duals) are both unique.

``planted_window`` keeps a given window's K, l, u and m_eq -- the pattern a band kernel verifies -- and replaces c and
q only; its optimum is planted the same way but need not be unique.
"""
import numpy as np
import scipy.sparse as sp

CLASSES = ("free", "lower", "upper", "boxed", "fixed")


def _pattern(n, m, wy, wx, rng, active, long_rows, long_row_len, long_cols, long_col_len, empty_cols, empty_rows):
    """(row lists of column indices, pivot column per row or -1).  Every row of `active` gets a pivot column of its
    own first, in the order of the rows' places along the band; empty_rows / empty_cols get no entry."""
    rows = [[] for _ in range(m)]
    ccount = np.zeros(n, int)
    col_ok = np.ones(n, bool)
    col_ok[empty_cols] = False
    row_ok = np.ones(m, bool)
    row_ok[empty_rows] = False
    rcap = np.full(m, wy)
    ccap = np.full(n, wx)
    rlen = np.broadcast_to(np.asarray(long_row_len, int), (len(long_rows),))
    clen = np.broadcast_to(np.asarray(long_col_len, int), (len(long_cols),))
    rcap[long_rows] = rlen
    ccap[long_cols] = clen
    live_cols = np.nonzero(col_ok)[0]
    live_rows = np.nonzero(row_ok)[0]
    place = rng.permutation(m)  # a row's place along the band: equality and >= rows interleave
    pivot = np.full(m, -1)
    act = np.asarray(active, int)
    act = act[np.argsort(place[act])]
    assert len(act) <= len(live_cols)
    for r, i in enumerate(act):
        pivot[i] = live_cols[r * len(live_cols) // len(act)]
        rows[i].append(int(pivot[i]))
        ccount[pivot[i]] += 1
    for a, i in enumerate(long_rows):  # evenly spaced columns, shifted per long row
        pick = live_cols[(np.arange(rlen[a]) * len(live_cols) // rlen[a] + a) % len(live_cols)]
        for j in pick:
            if len(rows[i]) < rlen[a] and int(j) not in rows[i]:
                rows[i].append(int(j))
                ccount[j] += 1
        assert len(rows[i]) == rlen[a]
    short_rows = np.array([i for i in live_rows if i not in set(long_rows)], int)
    for a, j in enumerate(long_cols):
        pick = short_rows[(np.arange(clen[a]) * len(short_rows) // clen[a] + a) % len(short_rows)]
        for i in pick:
            if ccount[j] < clen[a] and int(j) not in rows[int(i)]:
                rows[int(i)].append(int(j))
                ccount[j] += 1
        assert ccount[j] == clen[a], (j, ccount[j])
    # where the columns cannot hold wy entries for every row, most rows take their share and a few, evenly spread,
    # the full wy (so that both bounds are reached)
    room = int(np.maximum(ccap[live_cols] - ccount[live_cols], 0).sum())
    held = sum(len(rows[i]) for i in short_rows)
    share = max(1, min(wy, (room + held) // max(len(short_rows), 1)))
    if share < wy:
        full = (room + held - share * len(short_rows)) // (wy - share) // 2
        if full == 0 and share > 1:
            share -= 1
            full = (room + held - share * len(short_rows)) // (wy - share) // 2
        rcap[short_rows] = share
        if full > 0:
            rcap[short_rows[(np.arange(full) * len(short_rows)) // full]] = wy
    for i in short_rows[np.argsort(place[short_rows])]:
        a = int(pivot[i]) if pivot[i] >= 0 else int(place[i]) * n // m
        # the band stays narrow: a row looks 4 wy columns ahead, takes those without an entry first, and wanders
        # further only for its first entry
        ahead = [(a + t) % n for t in range(min(4 * wy, n))]
        cand = [j for j in ahead if col_ok[j] and ccount[j] < ccap[j] and j not in rows[i]]
        cand.sort(key=lambda j: ccount[j] > 0)
        for j in cand[:max(0, rcap[i] - len(rows[i]))]:
            rows[i].append(j)
            ccount[j] += 1
        t = len(ahead)
        while not rows[i] and t < n:
            j = (a + t) % n
            t += 1
            if col_ok[j] and ccount[j] < ccap[j]:
                rows[i].append(j)
                ccount[j] += 1
        if not rows[i]:
            raise ValueError(f"row {i}: no column with room (n wx = {n * wx} < entries asked for)")
    for j in live_cols[ccount[live_cols] == 0]:  # a column the band left out: the nearest row with room takes it
        near = np.argsort(np.abs(place[short_rows] * n // m - j))
        for i in short_rows[near]:
            if len(rows[i]) < max(rcap[i], 2):
                rows[i].append(int(j))
                ccount[j] += 1
                break
        else:
            raise ValueError(f"column {j} cannot be covered (m wy = {m * wy} too small for n = {n})")
    return [sorted(r) for r in rows], pivot


def planted(n, m_eq, m_ineq, wy, wx, seed, scale_spread=0.0, long_rows=0, long_row_len=0, long_cols=0,
            long_col_len=0, empty_cols=0, empty_rows=0, active_frac=0.5, classes=CLASSES):
    """An LP (oracle dict form: K csr, q, c, c0, l, u, m_eq) with extra keys x_star, y_star, lam_star, opt.

    wy / wx bound the entries per row / per column of the band; long_rows rows of long_row_len entries and long_cols
    columns of long_col_len entries (one length, or one per row / column) come on top (rows and columns of the band stay within wy / wx counting them);
    empty_cols columns without an entry (boxed, non-zero cost); empty_rows >= rows without an entry (q < 0);
    scale_spread s: rows and columns scaled by 10^U(-s, s); active_frac: the share of >= rows with y* > 0 (cut down
    where the active rows would outnumber the columns that can be their pivots)."""
    rng = np.random.default_rng(seed)
    m = m_eq + m_ineq
    assert empty_rows <= m_ineq and empty_cols < n
    er = m_eq + np.asarray((np.arange(empty_rows) * 2 + 1) * m_ineq // (2 * max(empty_rows, 1)), int)
    assert len(set(er.tolist())) == empty_rows
    ec = np.asarray((np.arange(empty_cols) * 2 + 1) * n // (2 * max(empty_cols, 1)), int) if empty_cols else np.zeros(0, int)
    cand_r = np.array([i for i in range(m) if i not in set(er.tolist())], int)
    lr = cand_r[(np.arange(long_rows) * 2 + 1) * len(cand_r) // (2 * max(long_rows, 1))] if long_rows else np.zeros(0, int)
    cand_c = np.array([j for j in range(n) if j not in set(ec.tolist())], int)
    lc = cand_c[(np.arange(long_cols) * 2 + 1) * len(cand_c) // (2 * max(long_cols, 1))] if long_cols else np.zeros(0, int)
    assert len(set(lr.tolist())) == long_rows and len(set(lc.tolist())) == long_cols
    # the active rows: every equality row, and a share of the >= rows that leaves a quarter of the columns at bounds
    live_ineq = np.setdiff1d(np.arange(m_eq, m), er)
    want = min(int(round(active_frac * len(live_ineq))), max(0, (n - empty_cols) * 3 // 4 - m_eq))
    active = np.zeros(m, bool)
    active[:m_eq] = True
    active[rng.choice(live_ineq, want, replace=False) if want else []] = True
    rows, pivot = _pattern(n, m, wy, wx, rng, np.nonzero(active)[0], [int(i) for i in lr], long_row_len,
                           [int(j) for j in lc], long_col_len, ec, er)
    interior = np.zeros(n, bool)
    interior[pivot[active]] = True

    # values: magnitudes in [0.5, 1.5], random signs; a pivot dominates its row's other interior entries
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([j for r in rows for j in r], np.int64)
    data = rng.uniform(0.5, 1.5, len(indices)) * rng.choice([-1.0, 1.0], len(indices))
    for i in np.nonzero(active)[0]:
        s, e = indptr[i], indptr[i + 1]
        cols = indices[s:e]
        p = s + int(np.nonzero(cols == pivot[i])[0][0])
        others = sum(abs(data[t]) for t in range(s, e) if t != p and interior[indices[t]])
        data[p] = np.sign(data[p]) * (1.0 + others) * rng.uniform(1.0, 1.25)
    K = sp.csr_matrix((data, indices, indptr), shape=(m, n))
    if scale_spread > 0:
        dr = 10.0 ** rng.uniform(-scale_spread, scale_spread, m)
        dc = 10.0 ** rng.uniform(-scale_spread, scale_spread, n)
        K = (sp.diags(dr) @ K @ sp.diags(dc)).tocsr()
    K.sort_indices()

    # bound classes, positions, x*, lam*
    inner_cls = [k for k in classes if k != "fixed"]
    outer_cls = [k for k in classes if k != "free"]
    cls = np.where(interior, rng.choice(inner_cls, n), rng.choice(outer_cls, n))
    cls[ec] = "boxed"
    if n >= len(classes):  # every class at least once where the columns allow
        for k in classes:
            pool = np.nonzero(interior if k == "free" else ~interior if k == "fixed" else np.ones(n, bool))[0]
            pool = np.setdiff1d(pool, ec)
            if not (cls == k).any() and len(pool):
                cls[pool[int(rng.integers(len(pool)))]] = k
    l = np.full(n, -np.inf)
    u = np.full(n, np.inf)
    x = np.zeros(n)
    lam = np.zeros(n)
    base = rng.uniform(-2.0, 2.0, n)
    width = rng.uniform(1.0, 3.0, n)
    mag = rng.uniform(0.5, 1.5, n)
    coin = rng.random(n) < 0.5
    for j in range(n):
        k = cls[j]
        if k in ("lower", "boxed", "fixed"):
            l[j] = base[j]
        if k == "boxed":
            u[j] = base[j] + width[j]
        if k == "upper":
            u[j] = base[j]
        if k == "fixed":
            u[j] = l[j]
        if interior[j]:
            x[j] = {"free": base[j], "lower": base[j] + width[j], "upper": base[j] - width[j],
                    "boxed": base[j] + width[j] * (0.25 + 0.5 * rng.random())}[k]
        else:
            at_upper = k == "upper" or (k == "boxed" and coin[j])
            x[j] = u[j] if at_upper else l[j]
            lam[j] = -mag[j] if at_upper else mag[j]
            if k == "fixed" and coin[j]:
                lam[j] = -mag[j]
    y = np.zeros(m)
    y[:m_eq] = rng.uniform(0.5, 1.5, m_eq) * rng.choice([-1.0, 1.0], m_eq)
    act_i = np.nonzero(active[m_eq:])[0] + m_eq
    y[act_i] = rng.uniform(0.5, 1.5, len(act_i))
    slack = np.zeros(m)
    idle = np.nonzero(~active)[0]
    slack[idle] = rng.uniform(0.5, 1.5, len(idle))
    if scale_spread > 0:  # keep |K x*| ~ |q| and |K'y*| ~ |c| row by row: the slack and lam follow the scaling
        slack *= dr
        lam *= dc
    q = K @ x - slack
    c = K.T @ y + lam
    c0 = float(rng.uniform(-10.0, 10.0))
    return dict(K=K, q=q, c=c, c0=c0, l=l, u=u, m_eq=m_eq, x_star=x, y_star=y, lam_star=lam,
                opt=float(c @ x + c0), pivot=pivot, interior=interior, classes=cls)


def planted_window(lp, seed, interior_frac=0.4, active_frac=0.5):
    """The oracle-dict window `lp` with its K, l, u, m_eq kept and c, q (and c0) replaced so that a drawn (x*, y*) is
    optimal.  Columns: interior with probability interior_frac where the box has an inside (always when the column has
    no finite bound), else at one of the finite bounds."""
    rng = np.random.default_rng(seed)
    K = sp.csr_matrix(lp["K"])
    m, n = K.shape
    m_eq = int(lp["m_eq"])
    l, u = np.asarray(lp["l"], float), np.asarray(lp["u"], float)
    fl, fu = np.isfinite(l), np.isfinite(u)
    wide = ~(fl & fu) | (u > l)
    interior = (wide & (rng.random(n) < interior_frac)) | (~fl & ~fu)
    at_upper = ~interior & fu & (~fl | (rng.random(n) < 0.5))
    span = np.where(fl & fu, u - l, 1.0 + np.abs(np.where(fl, l, np.where(fu, u, 0.0))))
    frac = 0.25 + 0.5 * rng.random(n)
    x = np.where(fl, l, np.where(fu, u - span, 0.0)) + frac * span  # interior value
    x = np.where(interior, x, np.where(at_upper, u, l))
    mag = rng.uniform(0.5, 1.5, n)
    lam = np.where(interior, 0.0, np.where(at_upper, -mag, mag))
    y = np.zeros(m)
    y[:m_eq] = rng.uniform(0.5, 1.5, m_eq) * rng.choice([-1.0, 1.0], m_eq)
    active = rng.random(m - m_eq) < active_frac
    y[m_eq:] = np.where(active, rng.uniform(0.5, 1.5, m - m_eq), 0.0)
    kx = K @ x
    slack = np.zeros(m)
    slack[m_eq:] = np.where(active, 0.0, rng.uniform(0.05, 0.15, m - m_eq) * (1.0 + np.abs(kx[m_eq:])))
    q = kx - slack
    c = K.T @ y + lam
    c0 = float(rng.uniform(-10.0, 10.0))
    return dict(K=K, q=q, c=c, c0=c0, l=l, u=u, m_eq=m_eq, x_star=x, y_star=y, lam_star=lam,
                opt=float(c @ x + c0))


def widths(lp):
    """(wx, wy, long columns, long rows) as the set-up kernel counts them for the ELL kernels: the widest column / row
    among those of at most 8 entries, and the number of longer ones."""
    K = sp.csr_matrix(lp["K"])
    rl = np.diff(K.indptr)
    cl = np.diff(K.tocsc().indptr)
    return (int(cl[cl <= 8].max(initial=0)), int(rl[rl <= 8].max(initial=0)), int((cl > 8).sum()), int((rl > 8).sum()))


def to_window(lp):
    from dervet_hip.solver import WindowLP
    return WindowLP.from_csr(sp.csr_matrix(lp["K"]), lp["q"], lp["c"], lp["l"], lp["u"], lp["m_eq"], lp["c0"])


def from_window(w):
    """The oracle dict of a dervet_hip WindowLP."""
    return dict(K=sp.csr_matrix((w.data, w.indices, w.indptr), shape=(w.m, w.n)), q=w.q, c=w.c, c0=w.c0, l=w.l, u=w.u,
                m_eq=w.m_eq)
