"""A handle owns what its calls make, and dvh_destroy releases it (der-vet_amd/csrc/dvh_handle.h): the valuation's
timing events and the cut pass's long-window workspace are the handle's, so a fresh handle reports no valuation time
whatever address it was given, its results do not depend on the handles before it, the workspace regrows under a launch
in flight, and every kind of handle is destroyed cleanly.  The bill world is tests/test_valuation_abi.py's (3 windows,
T = 6, J = 1), the cut windows are the T = 769, J = 1 ones of tests/test_gpu_value_cut.py (the smallest T above the
LDS form) and a third of the same seeds' family."""
import ctypes

import numpy as np
import pytest

import test_gpu_value_cut as VC
import test_valuation_abi as VA
import value_sizing_cases as C
import value_sizing_ref as R
from dervet_hip import BatchSolver, _lib
from dervet_hip import value_sizing as VS

pytestmark = pytest.mark.gpu

T_LONG = 769
I_LONG = VC.SHAPES.index((T_LONG, 1, {}))


def valuation_ms(s):
    ms = (ctypes.c_double * 2)(-1.0, -1.0)
    assert s._lib.dvh_last_valuation_ms(s._h, ms) == _lib.DVH_OK
    return ms[0], ms[1]


def destroy(s):
    """dvh_destroy's own return code (BatchSolver.close drops it)."""
    rc = s._lib.dvh_destroy(s._h)
    s._h = None
    return rc


@pytest.fixture(scope="module")
def bill_world(gpu_solver):
    import torch
    _, pb, t = VA.make_world(gpu_solver)
    pb.x.copy_(torch.linspace(-3.0, 5.0, pb.x.numel(), dtype=torch.float64))  # (so that the bills are no zeros)
    torch.cuda.synchronize()
    return pb, t


def run_bill(s, bill_world):
    """One valid bill call on handle `s`: the bytes of its bills and flags."""
    import torch
    pb, t = bill_world
    t["bills"].fill_(-7.0)
    t["bad"].fill_(-7)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, the call runs on the handle's)
    rc, msg = VA.bill_call((s, pb, t))
    assert rc == _lib.DVH_OK, msg
    s._check(s._lib.dvh_synchronize(s._h), "dvh_synchronize")
    assert list(t["bad"].cpu().numpy()) == [0] * VA.G
    return t["bills"].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def long_windows(gpu_solver):
    """Three solved T = 769 windows (rows 0 and 1 are test_gpu_value_cut's) and each one's cut in the host form."""
    positions = [C.positions([300 + I_LONG, 400 + I_LONG, 500 + I_LONG], 1, T_LONG, J=1)[0]]
    res, pb, groups, firsts = VC._solved(gpu_solver, positions)
    host = pb.to_numpy()
    want = []
    for row in range(3):
        lp, x, y = VC._host_lp(host, row, positions[0], row)
        want.append((R.cut_of(lp, x, y), lp, x, y))
    return dict(s=positions[0], res=res, pb=pb, group=groups[0], want=want)  # (res: the group points into its tensors)


def run_cuts(s, w, calls):
    """dvh_value_cuts on handle `s`, one call after the other with no wait between them: calls = [(first row, G)]."""
    import torch
    p = w["pb"].as_ctypes()
    outs = [torch.full((G, VS.CUT_COLS), -7.0, dtype=torch.float64, device="cuda:0") for _, G in calls]
    torch.cuda.synchronize()
    for (row, G), out in zip(calls, outs):
        g = VC._solo_group(w["group"], w["s"], row)
        g.G = G
        s._check(s._lib.dvh_value_cuts(s._h, ctypes.byref(g), ctypes.byref(p), row, out.data_ptr(), None), "dvh_value_cuts")
    s._check(s._lib.dvh_synchronize(s._h), "dvh_synchronize")
    return [o.cpu().numpy() for o in outs]


def test_a_fresh_handle_reports_no_valuation_time():
    with BatchSolver(0) as s:
        assert valuation_ms(s) == (0.0, 0.0)


def test_handles_after_a_destroyed_one_start_clean_and_bill_alike(bill_world):
    a = BatchSolver(0)
    bills_a = run_bill(a, bill_world)
    ms = valuation_ms(a)
    print(f"handle A: bill {ms[0]!r} ms, valuation {ms[1]!r} ms")
    assert ms[0] > 0.0 and ms[1] == 0.0
    assert destroy(a) == _lib.DVH_OK
    later = [BatchSolver(0) for _ in range(4)]  # (alive together: one of them is likely to sit where A sat)
    try:
        for b in later:
            assert valuation_ms(b) == (0.0, 0.0)
        for b in later:
            assert run_bill(b, bill_world) == bills_a
            assert valuation_ms(b)[0] > 0.0
    finally:
        for b in later:
            b.close()


def test_cut_workspace_regrows_under_a_launch_in_flight(long_windows):
    w = long_windows
    with BatchSolver(0) as s:
        one, grown = run_cuts(s, w, [(0, 1), (0, 3)])
    with BatchSolver(0) as s:
        fresh, = run_cuts(s, w, [(0, 3)])
    assert grown.tobytes() == fresh.tobytes() and one.tobytes() == fresh[:1].tobytes()
    for row, (want, lp, x, y) in enumerate(w["want"]):
        print(f"row {row}: status {int(fresh[row, VS.STATUS])} a {fresh[row, VS.A]!r} gE {fresh[row, VS.GE]!r} "
              f"gP {fresh[row, VS.GP]!r} D {fresh[row, VS.DOBJ]!r}; equal {np.array_equal(fresh[row, :6], want[:6])}")
        assert fresh[row, VS.FLAG] == 0.0
        R.assert_within_rounding(fresh[row], lp, x, y)
        assert np.array_equal(fresh[row, :6], want[:6])


@pytest.mark.parametrize("kind", ["never_solved", "with_peers", "after_valuation_and_long_cuts"])
def test_destroy_returns_ok_and_the_next_create_works(kind, bill_world, long_windows):
    s = BatchSolver(devices=[0, 0]) if kind == "with_peers" else BatchSolver(0)
    if kind == "with_peers":
        assert s.device_count == 2
    if kind == "after_valuation_and_long_cuts":
        run_bill(s, bill_world)
        run_cuts(s, long_windows, [(0, 3)])
    assert destroy(s) == _lib.DVH_OK
    with BatchSolver(0) as nxt:
        assert valuation_ms(nxt) == (0.0, 0.0)
        assert nxt._lib.dvh_synchronize(nxt._h) == _lib.DVH_OK
