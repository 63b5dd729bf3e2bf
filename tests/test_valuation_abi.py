"""The valuation entry points' contract (include/dervet_hip.h dvh_bill_windows, dvh_value_scenarios,
dvh_last_valuation_ms).  Wherever the library loads: the ctypes structs match the C layout (checked against g++) and a
null handle is a code, not a crash.  With a handle (GPU): every DVH_ERR_ARG / DVH_ERR_UNSUPPORTED case returns its code
with a message and launches nothing -- the output arrays keep the pattern they were filled with."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from dervet_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dervet_hip.h"\nint main() { std::printf("%zu %zu %zu %zu '
                   '%d %d %d %d %d %d\\n", sizeof(dvh_bill_group), sizeof(dvh_valuation), offsetof(dvh_bill_group, om), '
                   'offsetof(dvh_valuation, growth), DVH_BILL_ROWS, DVH_BILL_MAX_J, DVH_CBA_MAX_YEARS, DVH_CBA_MAX_EXTRA, '
                   'DVH_CBA_FIXED_COLS, DVH_VALUE_COLS); }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.BillGroup), ctypes.sizeof(_lib.ValuationArgs), _lib.BillGroup.om.offset,
                   _lib.ValuationArgs.growth.offset, _lib.BILL_ROWS, _lib.BILL_MAX_J, _lib.CBA_MAX_YEARS,
                   _lib.CBA_MAX_EXTRA, _lib.CBA_FIXED_COLS, _lib.VALUE_COLS]


def test_null_handle_is_a_code():
    lib = _lib.load()
    ms = (ctypes.c_double * 2)()
    assert lib.dvh_bill_windows(None, None, None, 0, None, None, None, None) == _lib.DVH_ERR_ARG
    assert lib.dvh_value_scenarios(None, None, None, None, None, None) == _lib.DVH_ERR_ARG
    assert lib.dvh_last_valuation_ms(None, ms) == _lib.DVH_ERR_ARG


# ---- with a handle

T, J, G = 6, 1, 3
N = 3 * T + J


@pytest.fixture(scope="module")
def world(gpu_solver):
    """A valid bill call and a valid valuation call; every case below breaks one argument of a copy."""
    return make_world(gpu_solver)


def make_world(solver):
    """(solver, batch, tensors) of the two calls (tests/test_gpu_handle_lifetime.py runs them on handles of its own)."""
    import torch
    from dervet_hip.packed import PackedBatch
    z = np.zeros
    desc = z((G, 8), np.int64)
    desc[:, 0], desc[:, 6] = N, N * np.arange(G)
    pb = PackedBatch(desc=desc, indptr=z(2 * G, np.int32), indices=z(G, np.int32), data=z(G), c=z(G * N), c0=z(G),
                     q=z(G), l=z(G * N), u=z(G * N)).to_torch("cuda:0").alloc_outputs()
    f64 = dict(dtype=torch.float64, device="cuda:0")
    t = dict(base=torch.ones(G * T, **f64), demand=torch.ones(G * J, **f64),
             rows=torch.zeros(T, dtype=torch.int32, device="cuda:0"), bills=torch.full((G, 8), -7.0, **f64),
             bad=torch.full((G,), -7, dtype=torch.int32, device="cuda:0"), values=torch.full((2, 7), -7.0, **f64),
             valid=torch.full((2,), -7, dtype=torch.int32, device="cuda:0"),
             ptr=torch.tensor([0, 2, 3], dtype=torch.int64, device="cuda:0"),
             idx=torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda:0"),
             year=torch.zeros(3, dtype=torch.int32, device="cuda:0"), capex=torch.ones(2, **f64))
    torch.cuda.synchronize()
    return solver, pb, t


def bill_call(world, edit=None, first=0, bills=True, bad=True):
    s, pb, t = world
    g = _lib.BillGroup()
    g.T, g.J, g.G, g.mI, g.dt = T, J, G, T, 1.0
    g.dcm_t = g.dcm_j = t["rows"].data_ptr()
    g.base, g.demand = t["base"].data_ptr(), t["demand"].data_ptr()
    p = pb.as_ctypes()
    if edit:
        edit(g, p)
    rc = s._lib.dvh_bill_windows(s._h, ctypes.byref(g), ctypes.byref(p), first, t["bills"].data_ptr() if bills else None,
                                 None, t["bad"].data_ptr() if bad else None, None)
    return rc, s._lib.dvh_last_error(s._h).decode()


def value_call(world, edit=None, values=True, valid=True):
    s, _, t = world
    keep = dict(opt=np.array([0], np.int32), ptr=np.array([0, 2, 3], np.int64))
    v = _lib.ValuationArgs()
    v.S, v.Y, v.n_opt, v.n_extra, v.n_win, v.n_bills = 2, 3, 1, 0, 3, G
    v.opt_years = keep["opt"].ctypes.data_as(_lib.c_int32_p)
    v.win_ptr_host = keep["ptr"].ctypes.data_as(_lib.c_int64_p)
    v.win_ptr, v.win_idx, v.win_year = t["ptr"].data_ptr(), t["idx"].data_ptr(), t["year"].data_ptr()
    v.bills, v.capex, v.fixed_om = t["bills"].data_ptr(), t["capex"].data_ptr(), t["capex"].data_ptr()
    v.rate = 0.05
    if edit:
        edit(v, keep)
    rc = s._lib.dvh_value_scenarios(s._h, ctypes.byref(v), t["values"].data_ptr() if values else None,
                                    t["valid"].data_ptr() if valid else None, None, None)
    return rc, s._lib.dvh_last_error(s._h).decode()


def untouched(world):
    import torch
    _, _, t = world
    torch.cuda.synchronize()
    return all(bool((t[k] == -7).all()) for k in ("bills", "bad", "values", "valid"))


def _set(name, value):
    return lambda a, _: setattr(a, name, value)


BILL_ARG = {
    "G_negative": dict(edit=_set("G", -1)), "T_zero": dict(edit=_set("T", 0)), "J_negative": dict(edit=_set("J", -1)),
    "mI_negative": dict(edit=_set("mI", -1)), "dt_zero": dict(edit=_set("dt", 0.0)),
    "first_negative": dict(first=-1), "past_batch": dict(first=1), "null_bills": dict(bills=False),
    "null_bad": dict(bad=False), "null_base": dict(edit=_set("base", None)), "null_rows": dict(edit=_set("dcm_t", None)),
    "null_demand": dict(edit=_set("demand", None)), "ice_without_cost": dict(edit=_set("has_ice", 1)),
    "null_x": dict(edit=lambda g, p: setattr(p, "x", None)), "null_desc": dict(edit=lambda g, p: setattr(p, "desc", None)),
}


def _ptr(i, value):
    def edit(v, keep):
        keep["ptr"][i] = value
    return edit


def _opt(value):
    def edit(v, keep):
        keep["opt"][0] = value
    return edit


VALUE_ARG = {
    "S_negative": dict(edit=_set("S", -1)), "Y_zero": dict(edit=_set("Y", 0)), "Y_65": dict(edit=_set("Y", 65)),
    "extra_17": dict(edit=_set("n_extra", 17)), "no_opt_year": dict(edit=_set("n_opt", 0)),
    "null_opt_years": dict(edit=_set("opt_years", None)), "opt_year_is_Y": dict(edit=_opt(3)),
    "opt_year_negative": dict(edit=_opt(-1)), "rate_minus_one": dict(edit=_set("rate", -1.0)),
    "rate_below": dict(edit=_set("rate", -1.5)), "rate_nan": dict(edit=_set("rate", float("nan"))),
    "win_ptr_not_monotone": dict(edit=_ptr(1, 4)), "win_ptr_short": dict(edit=_ptr(2, 2)),
    "win_ptr_long": dict(edit=_ptr(2, 4)), "win_ptr_start": dict(edit=_ptr(0, 1)),
    "null_win_ptr_host": dict(edit=_set("win_ptr_host", None)), "null_win_ptr": dict(edit=_set("win_ptr", None)),
    "null_win_idx": dict(edit=_set("win_idx", None)), "null_bills": dict(edit=_set("bills", None)),
    "null_capex": dict(edit=_set("capex", None)), "null_values": dict(values=False), "null_valid": dict(valid=False),
    "extra_without_array": dict(edit=_set("n_extra", 1)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(BILL_ARG))
def test_bill_argument_error_launches_nothing(world, case):
    rc, msg = bill_call(world, **BILL_ARG[case])
    assert rc == _lib.DVH_ERR_ARG and msg.startswith("bill:") and len(msg) > 12, (rc, msg)
    assert untouched(world)


@pytest.mark.gpu
def test_bill_with_too_many_demand_columns_is_unsupported(world):
    rc, msg = bill_call(world, edit=_set("J", _lib.BILL_MAX_J + 1))
    assert rc == _lib.DVH_ERR_UNSUPPORTED and "17" in msg and untouched(world)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(VALUE_ARG))
def test_valuation_argument_error_launches_nothing(world, case):
    rc, msg = value_call(world, **VALUE_ARG[case])
    assert rc == _lib.DVH_ERR_ARG and msg.startswith("valuation:") and len(msg) > 18, (rc, msg)
    assert untouched(world)


@pytest.mark.gpu
def test_empty_calls_succeed_and_launch_nothing(world):
    assert bill_call(world, edit=_set("G", 0))[0] == _lib.DVH_OK

    def no_scenarios(v, keep):
        v.S, v.n_win = 0, 0
        keep["ptr"][:] = 0
    assert value_call(world, edit=no_scenarios)[0] == _lib.DVH_OK
    assert untouched(world)


@pytest.mark.gpu
def test_the_valid_calls_run(world):
    """Last in this module: the calls every case above is a broken copy of do launch."""
    import torch
    s, _, t = world
    assert bill_call(world)[0] == _lib.DVH_OK
    assert value_call(world)[0] == _lib.DVH_OK
    torch.cuda.synchronize()
    assert not untouched(world) and list(t["bad"].cpu().numpy()) == [0, 0, 0] and list(t["valid"].cpu().numpy()) == [1, 1]
    ms = (ctypes.c_double * 2)()
    assert s._lib.dvh_last_valuation_ms(s._h, ms) == _lib.DVH_OK and ms[0] > 0.0 and ms[1] > 0.0
