"""Economic sizing on the GPU (dervet_hip.size_for_value: dvh_solve_packed_device, dvh_value_cuts, dvh_value_master)
against the monolithic relaxed sizing LP solved by HiGHS (tests/value_sizing_ref.py): 4 seeded cases x 3 windows of 48
steps -- interior optima, a box edge and the corner E = P = 0 -- and one case of a single 800-step window (the chain
tier), each with 1 and 4 candidates per round.

Bounds: the loop stops at upper - lower <= gap_tol (1 + |upper|) and its window solves run at eps_obj = gap_tol / 10,
so lower <= opt + gap_tol (1 + |opt|) and upper - opt <= 2 gap_tol (1 + |opt|); the objective at the rounded size is
held to the project's 1e-5 bar against HiGHS at that size."""
import numpy as np
import pytest

import value_sizing_cases as C
import value_sizing_ref as R
from dervet_hip import size_for_value
from dervet_hip import value_sizing as VS

pytestmark = pytest.mark.gpu

GAP = 1e-6
_MONO = {}


def _mono(name, positions, specs):
    """The monolithic optima, computed once per case set (they do not depend on the candidates per round)."""
    if name not in _MONO:
        _MONO[name] = [R.monolithic(positions, k, s) for k, s in enumerate(specs)]
    return _MONO[name]


def _check(results, positions, specs, mono):
    for k, (r, s, m) in enumerate(zip(results, specs, mono)):
        opt = m["obj"]
        tol = GAP * (1.0 + abs(opt))
        F = R.objective_at(positions, k, s, r.energy, r.power)
        print(f"case {k}: {r.status_name} rounds {r.rounds} cuts {r.n_cuts} iters {r.lp_iters} E {r.energy_lp:.3f} -> {r.energy} "
              f"(HiGHS {m['E']:.3f}) P {r.power_lp:.3f} -> {r.power} (HiGHS {m['P']:.3f}) lower - opt {r.lower - opt:.3e} "
              f"upper - opt {r.upper - opt:.3e} (tol {tol:.3e}) objective {r.objective!r} HiGHS at the size {F!r}")
        assert r.status == VS.SIZED
        assert r.lower <= opt + tol
        assert r.upper - opt <= 2.0 * tol
        assert r.upper >= opt - tol      # (an upper bound of the optimum: primal objectives of feasible points)
        assert abs(r.objective - F) <= 1e-5 * abs(F)
        assert r.energy == np.ceil(r.energy) and r.power == np.ceil(r.power)
        assert r.energy >= r.energy_lp - 1e-6 * max(1.0, r.energy_lp) and r.power >= r.power_lp - 1e-6 * max(1.0, r.power_lp)
        assert r.capex == s.capex(r.energy, r.power)
        assert abs(sum(r.terms[t] for t in ("energy", "power", "fixed", "windows")) - r.objective) <= 1e-9 * abs(r.objective)


def _same(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in ("energy", "power", "energy_lp", "power_lp", "lower", "upper", "objective",
                                                        "rounds", "n_cuts", "lp_iters", "status"))


@pytest.fixture(scope="module", params=[1, 4], ids=["C1", "C4"])
def small(request, gpu_solver):
    positions, specs = C.small_cases(request.param)
    log = []
    results = size_for_value(positions, specs, gpu_solver, log=log)
    return dict(C=request.param, positions=positions, specs=specs, results=results, log=log)


def test_small_cases_reach_the_monolithic_optimum(small):
    mono = _mono("small", small["positions"], small["specs"])
    _check(small["results"], small["positions"], small["specs"], mono)
    kinds = [(m["E"], m["P"]) for m in mono]
    assert kinds[2] == (0.0, 0.0)                                            # the corner
    assert 0.0 < kinds[0][0] < 12000.0 and 0.0 < kinds[0][1] < 2000.0        # interior
    assert kinds[3][0] == 4000.0 and 0.0 < kinds[3][1] < 2000.0              # a box edge
    assert small["results"][2].energy == 0.0 and small["results"][2].power == 0.0
    for k in (0, 1, 3):   # the reference's 3 % bar on sizes (the objective is flat near the optimum)
        assert abs(small["results"][k].energy - mono[k]["E"]) <= 0.03 * mono[k]["E"] + 1.0
        assert abs(small["results"][k].power - mono[k]["P"]) <= 0.03 * mono[k]["P"] + 1.0
    print("rounds", [(e["cases"], e["n_cand"], e["windows"], e["solve_host_syncs"], e["finished"]) for e in small["log"]])


def test_options_are_restored(small, gpu_solver):
    o = gpu_solver.options()
    assert o.eps == 1e-6 and o.eps_obj == 1e-6


def test_solo_results_equal_batched_results_bit_for_bit(small, gpu_solver):
    from dataclasses import replace
    for k in (0, 2):
        pos1 = [replace(s, base=s.base[k:k + 1], retail=s.retail[k:k + 1], demand=s.demand[k:k + 1], c0=s.c0[k:k + 1],
                        scal={n: v[k:k + 1] for n, v in s.scal.items()}, tags=[None]) for s in small["positions"]]
        solo = size_for_value(pos1, [small["specs"][k]], gpu_solver)[0]
        assert _same(solo, small["results"][k]), (solo, small["results"][k])


def test_a_failed_case_leaves_the_others_unchanged(small, gpu_solver):
    """Case 1 remade so that no size is feasible: sdr > 0 drains the battery, P_max = 0 cannot recharge it and
    E_min > 0 forbids the empty one -- its windows do not come back OPTIMAL, the case ends LP_FAILED with that status,
    and the other cases' results are the batch's, bit for bit."""
    from dataclasses import replace
    positions = [replace(s, scal=dict(s.scal, sdr=np.where(np.arange(s.G) == 1, 0.01, s.scal["sdr"]))) for s in small["positions"]]
    specs = list(small["specs"])
    specs[1] = replace(specs[1], power_max=0.0, energy_min=500.0)
    saved = gpu_solver.options()
    gpu_solver.set_options(max_iters=20000)   # (the infeasible windows run to the limit)
    try:
        results = size_for_value(positions, specs, gpu_solver)
    finally:
        gpu_solver.set_options(max_iters=saved.max_iters)
    assert results[1].status == VS.LP_FAILED and results[1].lp_status != 0 and np.isnan(results[1].objective)
    for k in (0, 2, 3):
        assert _same(results[k], small["results"][k]), k


@pytest.mark.parametrize("cand", [1, 4], ids=["C1", "C4"])
def test_a_chain_tier_window_is_sized(gpu_solver, cand):
    positions, specs = C.long_case(cand)
    results = size_for_value(positions, specs, gpu_solver, dispatch=True)
    mono = _mono("long", positions, specs)
    _check(results, positions, specs, mono)
    x = results[0].dispatch[0]
    assert x.shape == (3 * 800 + 1,) and x[:800].max() <= results[0].power * (1 + 1e-9)
