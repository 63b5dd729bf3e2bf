"""CPU: the band tests' window generator (tests/band_cases.py) builds the windows that the bits recorded in
tests/golden/band_limits_parent.json belong to, and planted_cases.battery_window is that generator."""
import json
import os

import numpy as np
import pytest

import band_cases as bc
import band_limits
import planted_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band_limits_parent.json")
ARRAYS = ("indptr", "indices", "data", "q", "c", "l", "u")


@pytest.mark.parametrize("T", band_limits.STEPS)
def test_generator_builds_the_recorded_windows(T):
    """The four golden windows (wave0's seeds) and their neighbours (load_scale 1.03), by the digest of their arrays."""
    with open(GOLDEN) as f:
        want = json.load(f)[str(T)]
    lp, nb = bc.window(T, 1, bc.WAVE0_SEEDS[T])[0], bc.window(T, 1, bc.WAVE0_SEEDS[T], load_scale=1.03)[0]
    assert band_limits.lp_digest(lp) == want["lp"], f"T {T}: not the recorded window"
    assert band_limits.lp_digest(nb) == want["neighbour"], f"T {T}: not the recorded neighbour"
    got_lp, got_nb = band_limits.windows()[T]
    assert band_limits.lp_digest(got_lp) == want["lp"] and band_limits.lp_digest(got_nb) == want["neighbour"]


@pytest.mark.parametrize("J", (0, 1, 4))
def test_planted_battery_window_is_the_generator(J):
    T = 25
    a, b = pc.battery_window(T, J), bc.window(T, J, 5)[0]
    assert (a.n, a.m, a.m_eq, a.c0) == (b.n, b.m, b.m_eq, b.c0)
    for k in ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), (J, k)


def test_span_covers_the_middle_half():
    """span: the one demand period is [T // 4, 3 T // 4) -- the DCM rows follow the T + 1 equality rows, one per step of
    the period, each starting with that step's charge column -- and nothing else of the window moves."""
    T = 25
    a, b = pc.battery_window(T, 1, span=True), bc.window(T, 1, 5)[0]
    assert a.m_eq == T + 1
    assert np.array_equal(a.indices[a.indptr[T + 1:a.m]], np.arange(T // 4, 3 * T // 4))
    assert np.array_equal(b.indices[b.indptr[T + 1:b.m]], np.arange((T + 1) // 2))
    assert np.array_equal(a.c, b.c) and np.array_equal(a.l, b.l) and np.array_equal(a.u, b.u)
    assert np.array_equal(a.q[:T + 1], b.q[:T + 1])
