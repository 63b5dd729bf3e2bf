"""dvh_value_cuts on the GPU: the cut of every window of a really solved batch against the numpy restatement
(value_sizing.host_cut) computed from the returned x, y and the batch's own LP vectors -- equal up to the rounding
bound of tests/value_sizing_ref.py (the operations and their order are the same, so in fact equal) -- for the shapes
at which the kernel takes another path, an ITER_LIMIT window, solo calls against the mixed batch, run to run, and every
validation error by its message."""
import ctypes

import numpy as np
import pytest

import value_sizing_cases as C
import value_sizing_ref as R
from dervet_hip import _lib
from dervet_hip import value_sizing as VS

pytestmark = pytest.mark.gpu

E0, P0 = 2500.0, 350.0
# (T, J, battery / window options): every T x J of the band tier's sizes, then llsoc > 0 and soc_target < 1 (the
# cases' defaults) with sdr > 0, an aggregate SOE ceiling active on some steps, and the first chain-tier size, where
# the per-step duals live in the pass's workspace
SHAPES = [(T, J, {}) for T in (2, 25, 192, 768) for J in (0, 1, 4)] + \
         [(48, 1, dict(sdr=0.5)), (96, 1, dict(emax_frac=1500.0)), (769, 1, {}), (769, 4, {})]


def _positions():
    return [C.positions([300 + i, 400 + i], 1, T, J=J, **kw)[0] for i, (T, J, kw) in enumerate(SHAPES)]


def _solved(gpu_solver, positions):
    import torch
    res = VS._Resident(positions, gpu_solver, "cuda:0")
    N = res.N
    ids = torch.arange(N, device=res.dev)
    E = torch.full((N,), E0, dtype=torch.float64, device=res.dev)
    P = torch.full((N,), P0, dtype=torch.float64, device=res.dev)
    pb, groups, firsts = res.build(ids, 1, E, P)
    gpu_solver.solve_packed(pb)
    return res, pb, groups, firsts


def _host_lp(pb_host, k, s, row):
    """Window k of the (host copy of the) batch as the dict value_sizing_ref.cut_of reads."""
    w = pb_host.window(k)
    import scipy.sparse as sp
    ip = np.asarray(w["indptr"], np.int64)
    K = sp.csr_matrix((w["data"], w["indices"], ip - ip[0]), shape=(w["m"], w["n"]))
    lp = dict(T=s.T, J=s.J, mI=len(s.dcm_t), dcm_t=np.asarray(s.dcm_t), dcm_j=np.asarray(s.dcm_j), K=K, dv=np.asarray(w["data"]),
              q=np.asarray(w["q"]), c=np.asarray(w["c"]), l=np.asarray(w["l"]), u=np.asarray(w["u"]), c0=w["c0"], E=E0, P=P0,
              soc_target=float(s.scal["soc_target"][row]), llsoc=float(s.scal["llsoc"][row]),
              ulsoc=float(s.scal["ulsoc"][row]), emax=None if s.emax is None else np.asarray(s.emax[row]))
    return lp, np.asarray(w["x"]), np.asarray(w["y"])


@pytest.fixture(scope="module")
def solved(gpu_solver):
    positions = _positions()
    res, pb, groups, firsts = _solved(gpu_solver, positions)
    wc = res.cuts(pb, groups, firsts, res.N, 1)
    gpu_solver._check(gpu_solver._lib.dvh_synchronize(gpu_solver._h), "dvh_synchronize")
    return dict(positions=positions, res=res, pb=pb, groups=groups, firsts=firsts, wc=wc, cuts=wc.cpu().numpy()[:, :, 0, :],
                host=pb.to_numpy())


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"T{T}_J{J}" + "".join("_" + k for k in kw) for T, J, kw in SHAPES])
def test_cut_of_a_solved_window_is_the_numpy_restatement(solved, i):
    s = solved["positions"][i]
    for row in range(2):
        k = solved["firsts"][i] + row
        got = solved["cuts"][i, row]
        lp, x, y = _host_lp(solved["host"], k, s, row)
        want = R.cut_of(lp, x, y)
        st, it = solved["host"].istats[k]
        print(f"window {k}: status {st} iters {it} a {got[VS.A]!r} gE {got[VS.GE]!r} gP {got[VS.GP]!r} "
              f"D {got[VS.DOBJ]!r} pobj {got[VS.POBJ]!r} rinf {got[VS.RINF]:.3e}; equal {np.array_equal(got[:6], want[:6])}")
        assert got[VS.FLAG] == 0.0 and int(got[VS.STATUS]) == st == _lib.OPTIMAL and int(got[VS.ITERS]) == it
        R.assert_within_rounding(got, lp, x, y)
        assert np.array_equal(got[:6], want[:6])   # the same operations in the same order, no contraction: equal
        # a converged window: the cut supports the window's value at its own size (the free tau columns' reduced
        # costs, which the dual bound drops, aside)
        scale = 1.0 + abs(want[VS.POBJ])
        free = got[VS.RINF] * np.abs(x[3 * s.T:]).sum()
        assert abs(got[VS.DOBJ] - got[VS.POBJ]) <= 1e-5 * scale + free
        assert abs((got[VS.A] + got[VS.GE] * E0 + got[VS.GP] * P0) - got[VS.DOBJ]) <= 1e-9 * scale


def test_an_iter_limit_window_still_yields_the_restated_cut(gpu_solver):
    positions = [C.positions([77, 78], 1, 192, J=1)[0]]
    saved = gpu_solver.options()
    gpu_solver.set_options(max_iters=64)
    try:
        res, pb, groups, firsts = _solved(gpu_solver, positions)
    finally:
        gpu_solver.set_options(max_iters=saved.max_iters)
    wc = res.cuts(pb, groups, firsts, res.N, 1)
    gpu_solver._check(gpu_solver._lib.dvh_synchronize(gpu_solver._h), "dvh_synchronize")
    cuts, host = wc.cpu().numpy()[0, :, 0, :], pb.to_numpy()
    for row in range(2):
        assert host.istats[row][0] == _lib.ITER_LIMIT and int(cuts[row, VS.STATUS]) == _lib.ITER_LIMIT
        lp, x, y = _host_lp(host, row, positions[0], row)
        R.assert_within_rounding(cuts[row], lp, x, y)
        # weak duality: the cut lies below HiGHS's optimum at its own size (rinf times the free columns' |x| aside)
        h = R.solve_highs(R.window_lp(positions[0], row, E0, P0))
        slack = cuts[row, VS.RINF] * np.abs(h["x"][3 * 192:]).sum() + 1e-9 * (1.0 + abs(h["obj"]))
        assert cuts[row, VS.DOBJ] <= h["obj"] + slack


def _solo_group(g, s, row):
    """The group struct of window `row` alone: G = 1, the per-window arrays advanced to it."""
    one = _lib.BatteryGroup()
    ctypes.pointer(one)[0] = g
    one.G = 1
    for name, per in (("base", s.T), ("retail", s.T), ("da", s.T), ("emax", s.T), ("demand", s.J), ("E", 1), ("pch", 1),
                      ("pdis", 1), ("rte", 1), ("sdr", 1), ("soc_target", 1), ("ulsoc", 1), ("llsoc", 1), ("om", 1), ("c0", 1)):
        v = getattr(g, name)
        if v:
            setattr(one, name, v + 8 * per * row)
    return one


def test_solo_calls_and_a_second_run_are_bit_identical_to_the_mixed_batch(gpu_solver, solved):
    import torch
    lib, h, p = gpu_solver._lib, gpu_solver._h, solved["pb"].as_ctypes()
    again = solved["res"].cuts(solved["pb"], solved["groups"], solved["firsts"], 2, 1)
    solo = torch.full((len(SHAPES), 2, VS.CUT_COLS), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()   # (the fill ran on torch's stream, the cuts run on the handle's)
    for i, (g, f) in enumerate(zip(solved["groups"], solved["firsts"])):
        for row in range(2):
            one = _solo_group(g, solved["positions"][i], row)
            gpu_solver._check(lib.dvh_value_cuts(h, ctypes.byref(one), ctypes.byref(p), f + row, solo[i, row].data_ptr(), None),
                              "dvh_value_cuts")
    gpu_solver._check(lib.dvh_synchronize(h), "dvh_synchronize")
    assert np.array_equal(again.cpu().numpy()[:, :, 0, :], solved["cuts"])
    assert np.array_equal(solo.cpu().numpy(), solved["cuts"])


def test_a_window_of_another_shape_is_flagged_not_read(gpu_solver, solved):
    """The group of one position against the windows of another: the descriptor check refuses them."""
    import torch
    lib, h, p = gpu_solver._lib, gpu_solver._h, solved["pb"].as_ctypes()
    out = torch.zeros((2, VS.CUT_COLS), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    gpu_solver._check(lib.dvh_value_cuts(h, ctypes.byref(solved["groups"][4]), ctypes.byref(p), solved["firsts"][7],
                                         out.data_ptr(), None), "dvh_value_cuts")
    gpu_solver._check(lib.dvh_synchronize(h), "dvh_synchronize")
    o = out.cpu().numpy()
    assert (o[:, VS.FLAG] == 1.0).all() and np.isnan(o[:, :6]).all()


def _refused(gpu_solver, rc, code, text):
    msg = gpu_solver._lib.dvh_last_error(gpu_solver._h).decode()
    assert rc == code and text in msg, (rc, msg)


def test_every_validation_error_has_its_message(gpu_solver, solved):
    import torch
    lib, h, p = gpu_solver._lib, gpu_solver._h, solved["pb"].as_ctypes()
    g0 = solved["groups"][0]
    out = torch.zeros((2, VS.CUT_COLS), dtype=torch.float64, device="cuda:0")

    def cuts(edit=None, group=True, batch=True, first=0, dst=out.data_ptr()):
        g = _lib.BatteryGroup()
        ctypes.pointer(g)[0] = g0
        if edit:
            edit(g)
        return lib.dvh_value_cuts(h, ctypes.byref(g) if group else None, ctypes.byref(p) if batch else None, first, dst, None)

    _refused(gpu_solver, cuts(group=False), -1, "null group or batch")
    _refused(gpu_solver, cuts(batch=False), -1, "null group or batch")
    _refused(gpu_solver, cuts(dst=None), -1, "null output array")
    _refused(gpu_solver, cuts(first=-1), -1, "count out of range")
    _refused(gpu_solver, cuts(first=solved["pb"].count - 1), -1, "outside the batch")
    _refused(gpu_solver, cuts(lambda g: setattr(g, "T", 0)), -1, "count out of range")
    _refused(gpu_solver, cuts(lambda g: setattr(g, "E", None)), -1, "null rating array")
    _refused(gpu_solver, cuts(lambda g: setattr(g, "has_emax", 1)), -1, "null emax series")
    _refused(gpu_solver, cuts(lambda g: setattr(g, "has_ice", 1)), -3, "ICE windows are not sized")
    _refused(gpu_solver, cuts(lambda g: setattr(g, "has_emin", 1)), -3, "minimum-SOE series is not supported")
    _refused(gpu_solver, cuts(lambda g: setattr(g, "J", 65)), -3, "demand-charge columns (at most 64)")

    good = C.spec(0.1, 4).as_struct()
    dev = torch.zeros(64, dtype=torch.float64, device="cuda:0")

    def master(edit=None, spec_edit=None):
        a = _lib.ValueMasterArgs()
        a.count, a.n_cases, a.W, a.n_cand, a.n_next, a.cut_cap = 1, 1, 1, 1, 1, 64
        sh = (_lib.ValueSpec * 1)(good)
        if spec_edit:
            spec_edit(sh[0])
        a.spec_host = ctypes.cast(sh, ctypes.POINTER(_lib.ValueSpec))
        for f in ("spec", "case_ids", "window_cuts", "E_in", "P_in", "cuts", "state", "flags", "E_out", "pch_out", "pdis_out"):
            setattr(a, f, dev.data_ptr())
        if edit:
            edit(a)
        return lib.dvh_value_master(h, ctypes.byref(a), None)

    _refused(gpu_solver, lib.dvh_value_master(h, None, None), -1, "null arguments")
    _refused(gpu_solver, master(lambda a: setattr(a, "cuts", None)), -1, "null array")
    _refused(gpu_solver, master(lambda a: setattr(a, "count", 2)), -1, "case count out of range")
    _refused(gpu_solver, master(lambda a: setattr(a, "W", 0)), -1, "W must be at least 1")
    _refused(gpu_solver, master(lambda a: setattr(a, "n_cand", 9)), -1, "candidates per round out of range")
    _refused(gpu_solver, master(lambda a: setattr(a, "n_next", 0)), -1, "candidates per round out of range")
    _refused(gpu_solver, master(lambda a: setattr(a, "cut_cap", 257)), -1, "cut capacity out of range")
    _refused(gpu_solver, master(spec_edit=lambda s: setattr(s, "energy_max", float("inf"))), -1, "finite energy_max")
    _refused(gpu_solver, master(spec_edit=lambda s: setattr(s, "power_max", float("inf"))), -1, "finite power_max")
    _refused(gpu_solver, master(spec_edit=lambda s: setattr(s, "c_energy", 0.0)), -1, "c_energy > 0")
    _refused(gpu_solver, master(spec_edit=lambda s: setattr(s, "c_power", -1.0)), -1, "c_power > 0")
    _refused(gpu_solver, master(spec_edit=lambda s: (setattr(s, "size_energy", 0), setattr(s, "size_power", 0))), -1,
             "nothing is sized")
    _refused(gpu_solver, master(spec_edit=lambda s: setattr(s, "max_rounds", 0)), -1, "max_rounds out of range")
    _refused(gpu_solver, master(spec_edit=lambda s: setattr(s, "gap_tol", 0.0)), -1, "gap_tol must be positive")
