"""CPU: tests/chain_plan_ref.py, the Python restatement of the medium tier's plan kernel, gives the hand-derived plans
of planted_cases.CHAIN_PLAN and plans that pass `invariants` on random run patterns, and its count of poll-list entries
shows which planned windows the team kernel's lists do not hold."""
import numpy as np
import pytest

import chain_plan_ref as cpr
import planted_cases as pc


@pytest.mark.parametrize("name", list(pc.CHAIN_PLAN))
def test_table_plan(name):
    T, J, tau, starts, pairs, _ = pc.CHAIN_PLAN[name]
    assert len(tau) == T and set(tau.tolist()) - {-1} == set(range(J))
    p = cpr.plan(tau, J)
    if starts is None:
        assert p == {"P": 0}, p
        return
    assert p["P"] == len(starts) - 1 and tuple(p["starts"].tolist()) == starts, (name, p["starts"])
    want = np.broadcast_to(np.array(pairs), (p["P"],))
    assert np.array_equal(p["pairs"], want), (name, p["pairs"])
    assert np.array_equal(p["nA"], 2 * want) and np.array_equal(p["nK"][:-1], 2 * want[:-1] + 2) \
        and p["nK"][-1] == 2 * want[-1]
    cpr.invariants(p, tau)
    assert cpr.lists_fit(p) == (name not in pc.CHAIN_PLAN_OVERFLOW), (name, p["nK"].max())


def test_table_plan_details():
    """The slots of the cases that are about them."""
    mid = cpr.plan(*_tj("mid1_J3"))
    assert mid["slot"].tolist() == [[-1] * 4, [0, -1, -1, -1], [1, -1, -1, -1], [2, 1, -1, -1], [1, -1, -1, -1]]
    assert (mid["lo"][3, 1], mid["hi"][3, 1]) == (2, 4)
    free = cpr.plan(*_tj("free_J2"))
    assert free["slot"][:, :2].tolist() == [[1, -1], [0, 1], [1, -1]]
    a4 = cpr.plan(*_tj("all_J4"))
    assert a4["slot"].tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]] and np.all(a4["lo"] == 0) and np.all(a4["hi"] == 1)
    # chainT1400J1: its demand period [350, 1050) gets a segment of its own; no column is shared
    tau = np.full(1400, -1)
    tau[350:1050] = 0
    own = cpr.plan(tau, 1)
    assert own["starts"].tolist() == [0, 350, 1050, 1400] and own["pairs"].tolist() == [0, 0, 0]


def _tj(name):
    return pc.CHAIN_PLAN[name][2], pc.CHAIN_PLAN[name][1]


def test_poll_list_limit():
    """127 pairs fill a segment's K list (2 x 127 + 2 = 256 entries).  One column over P segments is P - 1 pairs per
    segment, two interleaved columns 2 (P - 1).  The plan accepts more: those plans do not fit the lists."""
    assert cpr.PAIRS_MAX == 127
    fits = cpr.plan(np.zeros(128 * 768, int), 1)
    assert fits["pairs"].max() == 127 and fits["nK"].max() == 256 and cpr.lists_fit(fits)
    over = cpr.plan(np.zeros(128 * 768 + 1, int), 1)
    assert over["P"] == 129 and over["pairs"].max() == 128 and not cpr.lists_fit(over)
    two = cpr.plan(np.arange(64 * 768) % 2, 2)
    assert two["nA"].max() == 252 and two["nK"].max() == 254 and cpr.lists_fit(two)
    tail = cpr.plan(np.arange(64 * 768 + 1) % 2, 2)  # (the one-step tail holds one column)
    assert tail["pairs"].max() == 127 and cpr.lists_fit(tail)
    assert not cpr.lists_fit(cpr.plan(np.arange(64 * 768 + 2) % 2, 2))
    # the 5-minute year (T = 105,120): monthly columns (12 runs) share little; year-round columns run far past the
    # lists -- 136 pairs, 272 (the A list runs over the K list), 544 (over the boundary entries at 1016 .. 1023 too)
    month = np.repeat(np.arange(12), 105120 // 12)
    p = cpr.plan(month, 12)
    assert p["P"] >= 137 and p["pairs"].max() <= 24 and cpr.lists_fit(p)
    cpr.invariants(p, month)
    for J, pairs in ((1, 136), (2, 272), (4, 544)):
        year = cpr.plan(np.arange(105120) % J, J)
        assert year["P"] == 137 and year["pairs"].max() == pairs and not cpr.lists_fit(year)
    assert 2 * 544 > 1016


def test_segment_limit():
    assert cpr.plan(np.full(192 * 768, -1), 0)["P"] == 192
    assert cpr.plan(np.full(192 * 768 + 1, -1), 0) == {"P": 0}
    assert cpr.plan(np.array([0, 0, 2, 2]), 3) == {"P": 0}  # column 1 has no rows


def _random_tau(rng):
    """Runs of lengths mixing 1, 767, 768, 769 and arbitrary ones, over 0-6 columns and steps without a demand row;
    returned with the ids renumbered so that every column 0 .. J - 1 has rows."""
    J = int(rng.integers(0, 7))
    ids = list(range(J)) + ([-1] if J == 0 or rng.random() < 0.7 else [])
    pieces, prev = [], None
    for _ in range(int(rng.integers(1, 13))):
        j = ids[int(rng.integers(len(ids)))]
        if j == prev and len(ids) > 1:
            continue
        n = int(rng.choice([1, 767, 768, 769, int(rng.integers(2, 40)), int(rng.integers(40, 2000))]))
        if rng.random() < 0.15 and J >= 2:  # an interleaved stretch, as hourly tariff periods
            k = int(rng.integers(2, J + 1))
            pieces.append(np.arange(n) % k)
            prev = None
        else:
            pieces.append(np.full(n, j))
            prev = j
    tau = np.concatenate(pieces)
    used = sorted(set(tau.tolist()) - {-1})
    remap = {j: i for i, j in enumerate(used)}
    remap[-1] = -1
    return np.array([remap[j] for j in tau.tolist()]), len(used)


def test_random_run_patterns_hold_the_invariants():
    rng = np.random.default_rng(20240917)
    planned = refused = shared = free = 0
    for _ in range(400):
        tau, J = _random_tau(rng)
        p = cpr.plan(tau, J)
        if p["P"] == 0:
            refused += 1
            continue
        planned += 1
        cpr.invariants(p, tau)
        assert cpr.lists_fit(p)  # (at most 12 runs of at most 2,000 steps: far from 127 pairs)
        shared += int(p["pairs"].max() > 0)
        st = p["starts"]
        for s in range(p["P"]):  # a column held in a free slot: no rows of it in the segment
            here = set(tau[st[s]:st[s + 1]].tolist())
            free += any(j >= 0 and j not in here for j in p["slot"][s])
    print(f"planned {planned}, refused {refused}, with a shared column {shared}, free-slot holders {free}")
    assert planned >= 250 and refused >= 5 and shared >= 100 and free >= 10
