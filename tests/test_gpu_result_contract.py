"""GPU: the result contract of include/dervet_hip.h dvh_result on the band, ICE, interconnection and chain forms.

Every other GPU test takes primal_res_rel, dual_res_rel, gap_rel and the decision OPTIMAL from the kernel under test,
and checks the dual side, if at all, by comparing two kernels with each other.  Here both are recomputed on the host
from the returned x, y alone (tests/kkt_ref.py, tests/result_contract.py: contracts A and B), for one realistic window
(reference optimum: HiGHS) and one planted window (planted_lp.planted_window: the same K, l, u, m_eq, with c and q
replaced so that the optimal value is known exactly) per shape: T in {2, 25, 200, 745, 768} x J in {0, 1, 4} for the
battery forms, config-5 windows for the ICE form, POI / curtailable-PV / charge-from-PV windows for the interconnection
form, and two-segment windows (3 T + J > 4096) for the chain team.  tests/test_planted_lp.py holds the CPU side: every
planted window here has the planted optimum (HiGHS) and the host restatement solves it within 25,000 iterations.

The form that ran is asserted from the path counts and variant codes, as tests/test_gpu_band_loop.py does.
The ICE form's objective gate omits the dual-residual term by design (BandTune<true>::gate_rdx, dvh_band.hip), so its
windows are held to the gate without that term.
"""
import functools

import numpy as np
import pytest

import band_cases as bc
import planted_cases as pc
import planted_lp
import result_contract as rc
from dervet_hip import BatchSolver, _lib
from dervet_hip.solver import SolverError, WindowLP
from oracle import window_lp

pytestmark = pytest.mark.gpu

OPTIONS = dict(eps=1e-6, eps_obj=1e-6, max_iters=100000, check_every=32, kkt_every=4, kkt_predict=0, warm_start=0,
               certify=0)
BAND3, BAND3_J1, BAND1, ICE = bc.GENERIC, bc.STATIC, bc.ONE_STEP, bc.ICE
LIMITS = bc.LIMITS  # below, at and past one and two check periods


@pytest.fixture(scope="module")
def solver():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no GPU is visible (run with -m 'not gpu' on CPU hosts)")
    with BatchSolver(0) as s:
        yield s


@functools.lru_cache(maxsize=None)
def _highs_opt(family, name):
    base = _family(family)[name][0]
    h = window_lp.solve_highs(base)
    assert h["status"] == 0, (family, name)
    return h["obj"]


def _family(family):
    return dict(band=pc.band_windows, ice=pc.ice_windows, interconnect=pc.interconnect_windows,
                chain=pc.chain_windows)[family]()


def _batch(family, keep=lambda name: True):
    """[(what, oracle dict, reference optimum)]: the realistic and the planted window of every kept shape."""
    out = []
    for name, (base, planted) in _family(family).items():
        if keep(name):
            out.append((f"{name} realistic", base, _highs_opt(family, name)))
            out.append((f"{name} planted", planted, planted["opt"]))
    return out


def _solve(s, path, items, **options):
    opts = dict(OPTIONS)
    opts.update(options)
    s.set_options(**opts)
    s.set_kernel_path(path)
    try:
        res = s.solve([planted_lp.to_window(lp) for _, lp, _ in items])
        return res, s.kernel_stats()
    finally:
        s.set_kernel_path("default")
        s.set_options(**OPTIONS)


def _only(ks, key, count):
    for k in ("band_windows", "ell_windows", "generic_windows", "large_windows", "chain_windows"):
        assert ks[k] == (count if k == key else 0), ks


FORMS = {
    # form: (family, window filter, kernel path, path count, variant, band variant, gate has the rdx term)
    "band3_mixed_J": ("band", lambda n: True, "band3", "band_windows", BAND3, BAND3, True),
    "band3_J1": ("band", lambda n: n.endswith("J1"), "band3", "band_windows", BAND3, BAND3_J1, True),
    "band1": ("band", lambda n: True, "band1", "band_windows", BAND1, BAND1, True),
    # (band_variant reports the battery pass's instantiation only: -1 when that pass took nothing)
    "ice": ("ice", lambda n: True, "default", "band_windows", ICE, -1, False),
    "interconnect": ("interconnect", lambda n: True, "interconnect", "band_windows", None, None, True),
    "chain": ("chain", lambda n: True, "default", "chain_windows", None, None, True),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_optimal_results_are_optimal_and_reported_numbers_describe_them(solver, form):
    family, keep, path, count_key, variant, band_variant, with_rdx = FORMS[form]
    items = _batch(family, keep)
    res, ks = _solve(solver, path, items)
    _only(ks, count_key, len(items))
    if variant is not None:
        assert ks["variant"] == variant and ks["band_variant"] == band_variant, ks
    if form == "interconnect":  # dvh_band_grid.hip: 9000000 + 200 + waves per workgroup
        assert 9000200 <= ks["variant"] < 9000300, ks
    if form == "chain":
        assert ks["chain_aborts"] == 0, ks
    for (what, lp, opt), r in zip(items, res):
        rc.check_both(lp, r, opt, f"{form} {what}", form, with_rdx=with_rdx)


@pytest.mark.parametrize("form", ["band3_mixed_J", "band3_J1", "band1", "ice", "interconnect", "chain"])
def test_iteration_limit_results_describe_the_returned_point(solver, form):
    """ITER_LIMIT: contract B at limits below, at and past the check period.  A limit below check_every shortens the
    period (csrc/dvh_solve.cpp make_opts), so a check runs at the limit on every tier: the numbers are those of the
    returned x, y and never the NaN of "no check ran"."""
    family, keep, path, count_key, variant, band_variant, _ = FORMS[form]
    # (windows the host restatement needs more than a thousand iterations for: none ends OPTIMAL inside the limits)
    hard = dict(band3_mixed_J=("T200J4", "T745J4"), band1=("T200J4", "T745J4"), band3_J1=("T200J1", "T745J1"),
                ice=("ice0",), chain=("chainT1400J1",), interconnect=tuple(n for n in _family("interconnect") if "T745J4" in n))[form]
    items = _batch(family, lambda n: n in hard)
    assert len(items) == 2 * len(hard)
    worst = 0.0
    for mi in LIMITS:
        res, ks = _solve(solver, path, items, max_iters=mi, check_every=64, kkt_every=1)
        _only(ks, count_key, len(items))
        for (what, lp, _), r in zip(items, res):
            assert r.status == _lib.ITER_LIMIT and r.iters == mi, (form, what, mi, r.status_name, r.iters)
            assert np.isfinite([r.obj, r.primal_res_rel, r.dual_res_rel, r.gap_rel]).all(), (form, what, mi)
            assert np.all(r.x >= lp["l"]) and np.all(r.x <= lp["u"]) and np.all(r.y[lp["m_eq"]:] >= 0), (form, what, mi)
            worst = max(worst, rc.check_reported(lp, r, f"{form} {what} max_iters {mi}")[1])
    print(f"RESULT_CONTRACT form={form} case=iteration_limits reported_vs_recomputed={worst:.3e}")


def test_iteration_limit_on_a_multiple_of_the_kkt_period(solver):
    """max_iters = 2 check_every kkt_every on the default options' periods: the last check is the one at the limit."""
    items = _batch("band", lambda n: n in ("T200J1", "T745J4"))
    res, ks = _solve(solver, "band3", items, max_iters=256)
    _only(ks, "band_windows", len(items))
    for (what, lp, _), r in zip(items, res):
        assert r.status == _lib.ITER_LIMIT and r.iters == 256, (what, r.status_name, r.iters)
        rc.check_reported(lp, r, what)


def test_a_window_without_rows_is_rejected_with_a_message(solver):
    lp = WindowLP(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.array([1.0]), np.zeros(0), np.zeros(1),
                  np.ones(1), 0, 0.0)
    with pytest.raises(SolverError, match="no constraint rows"):
        solver.solve([lp])
