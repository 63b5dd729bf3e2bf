"""The medium tier's plan (csrc/dvh_chain.hip chain_plan_kernel) in plain Python: how a battery window of T steps is
cut into segments of at most 768 steps and which demand (tau) columns each segment holds and shares.
tests/test_chain_plan_ref.py holds this restatement to hand-derived plans (planted_cases.CHAIN_PLAN) and to
`invariants` on random run patterns.

The input is the tau id of every step (-1: the step has no demand row) and the number of tau columns J.  The greedy
walks the runs of equal ids:
  * a segment is closed in front of a run when it is full (768 steps), when the run brings a column and the segment's
    four slots are taken, or when the run would not end inside the segment but fits a segment of its own (run_cut);
  * a run longer than what is left of the segment is cut into full segments;
  * more than 192 segments: refused;
  * a column's sharers are the segments from the first to the last that has rows of it; a segment in between without
    rows of it takes it into a free slot, or the window is refused; a column without rows: refused.
A refused window is {"P": 0}: the grid-wide path solves it.

The poll lists.  The team kernel gives each segment two lists of 256 entries in LDS (poff: A in [0, 256), K in
[256, 512)) and fills them without looking at their ends: every (slot, other sharer) pair takes 2 entries of A and 2
of K, and K starts with the 2 of the next segment's first-ene image (the last segment has none).  So the lists hold
127 pairs (`PAIRS_MAX`), and THE PLAN KERNEL DOES NOT REFUSE A WINDOW WITH MORE: `lists_fit` is false for the plan it
accepts of two interleaved columns over 65 segments (planted_cases s65_J2: 128 pairs, K spills 2 entries into the C
list, which is rewritten before every check) and of one year-round column over 129 segments or more.  That is a
defect of the kernel, found by reading; no GPU test here runs such a window.
"""
import numpy as np

CB = 768        # steps per segment (kChainB)
P_MAX = 192     # segments per window (kPMax)
J_SEG = 4       # tau slots per segment (kChainJSeg)
J_MAX = 256     # tau columns per window (kChainJMax)
LIST = 256      # entries of a segment's A list and of its K list (kPollK, kPollC - kPollK)
PAIRS_MAX = (LIST - 2) // 2

REFUSED = {"P": 0}


def tau_ids(lp):
    """(tau id per step, J) of an oracle-dict battery window: columns ch[T] dis[T] ene[T] tau[J], rows init + T SOE
    equalities, then one >= row per step of a demand period."""
    import scipy.sparse as sp
    K = sp.csr_matrix(lp["K"])
    T = int(lp["m_eq"]) - 1
    J = K.shape[1] - 3 * T
    tau = np.full(T, -1, np.int64)
    for i in range(T + 1, K.shape[0]):
        cols = K.indices[K.indptr[i]:K.indptr[i + 1]]
        tau[cols[cols < T][0]] = cols[cols >= 3 * T][0] - 3 * T
    return tau, J


def plan(tau, J):
    tau = np.asarray(tau, np.int64)
    T = len(tau)
    if T < 1 or T > P_MAX * CB or J < 0 or J > J_MAX:
        return dict(REFUSED)
    rs = np.concatenate(([0], 1 + np.nonzero(tau[1:] != tau[:-1])[0], [T])).tolist()
    starts, slots = [0], []
    state = dict(s0=0, cur=[])

    def close(t):
        if len(slots) >= P_MAX:
            return False
        slots.append(state["cur"] + [-1] * (J_SEG - len(state["cur"])))
        starts.append(t)
        state["s0"], state["cur"] = t, []
        return True

    for a, e in zip(rs[:-1], rs[1:]):
        j = int(tau[a])
        newj = j >= 0 and j not in state["cur"]
        s0 = state["s0"]
        run_cut = a > s0 and e - s0 > CB and e - a <= CB
        if a - s0 == CB or (newj and len(state["cur"]) == J_SEG) or run_cut:
            if not close(a):
                return dict(REFUSED)
            newj = j >= 0
        if newj:
            state["cur"].append(j)
        while e - state["s0"] > CB:  # full segments inside the run
            if not close(state["s0"] + CB):
                return dict(REFUSED)
            if j >= 0:
                state["cur"].append(j)
    if not close(T):
        return dict(REFUSED)
    P = len(slots)
    slot = np.array(slots, np.int32).reshape(P, J_SEG)
    col_lo, col_hi = {}, {}
    for s in range(P):
        for j in slot[s]:
            if j >= 0:
                col_lo.setdefault(int(j), s)
                col_hi[int(j)] = s
    for j in range(J):
        if j not in col_hi:
            return dict(REFUSED)  # a tau column without rows
        for s in range(col_lo[j] + 1, col_hi[j]):
            if j in slot[s]:
                continue
            free = np.nonzero(slot[s] < 0)[0]
            if len(free) == 0:
                return dict(REFUSED)
            slot[s, free[0]] = j
    lo = np.zeros((P, J_SEG), np.int32)
    hi = np.full((P, J_SEG), -1, np.int32)
    for s in range(P):
        for u in range(J_SEG):
            if slot[s, u] >= 0:
                lo[s, u], hi[s, u] = col_lo[int(slot[s, u])], col_hi[int(slot[s, u])]
    out = dict(P=P, T=T, J=J, starts=np.array(starts, np.int32), slot=slot, lo=lo, hi=hi)
    out.update(poll_lists(out))
    return out


def poll_lists(p):
    """Entries of each segment's A and K poll lists."""
    pairs = np.where(p["slot"] >= 0, p["hi"] - p["lo"], 0).sum(axis=1)
    nK = 2 * pairs + 2
    nK[-1] -= 2
    return dict(pairs=pairs, nA=2 * pairs, nK=nK)


def lists_fit(p):
    """Whether every segment's poll lists hold its entries."""
    lists = poll_lists(p)
    return bool(lists["nA"].max() <= LIST and lists["nK"].max() <= LIST)


def invariants(p, tau):
    """What the team kernel relies on in an accepted plan of the window with these tau ids."""
    tau = np.asarray(tau, np.int64)
    P, T = p["P"], p["T"]
    st, slot, lo, hi = p["starts"], p["slot"], p["lo"], p["hi"]
    assert 1 <= P <= P_MAX and T == len(tau) and len(st) == P + 1 and slot.shape == lo.shape == hi.shape == (P, J_SEG)
    L = np.diff(st)
    assert st[0] == 0 and st[-1] == T and L.min() >= 1 and L.max() <= CB, st  # the segments tile [0, T)
    holders = {}
    for s in range(P):
        ids = slot[s]
        nsl = int((ids >= 0).sum())
        assert np.all(ids[:nsl] >= 0) and np.all(ids[nsl:] == -1), (s, ids)  # packed from slot 0 (lane < nsl)
        assert len(set(ids[:nsl].tolist())) == nsl, (s, ids)
        for u in range(nsl):
            holders.setdefault(int(ids[u]), []).append(s)
        here = set(tau[st[s]:st[s + 1]].tolist()) - {-1}
        assert here <= set(ids[:nsl].tolist()), (s, here, ids)  # every step's column is held by its segment
    assert set(holders) == set(range(p["J"])), holders
    for j, hs in holders.items():
        assert hs == list(range(hs[0], hs[-1] + 1)), (j, hs)  # a contiguous range, every segment of it a holder
        for s in hs:
            u = int(np.nonzero(slot[s] == j)[0][0])
            assert (lo[s, u], hi[s, u]) == (hs[0], hs[-1]), (j, s)  # lo / hi equal across the sharers
        rows = np.nonzero(tau == j)[0]
        assert st[hs[0]] <= rows[0] < st[hs[0] + 1] and st[hs[-1]] <= rows[-1] < st[hs[-1] + 1], (j, hs)
    assert np.all(lo[slot < 0] == 0) and np.all(hi[slot < 0] == -1)
