"""Drop-in window loop with GPU certificates (dervet_hip.dropin, ``certify=True``), on tests/test_dropin.py's fakes:
a window the solver returns as PRIMAL_INFEASIBLE / DUAL_INFEASIBLE is saved as "infeasible" / "unbounded" without the
reference re-solve and counted under ``LoopReport.certified``; with the default the reference re-solves it, as
before.  The solver is a CPU stand-in (HiGHS) that marks chosen windows; the GPU run of the pass is
tests/test_gpu_certify.py."""
import types

import numpy as np

from dervet_hip import dropin
from test_dropin import CpuStandInSolver, FakeExporter, FakeScenario


class MarkingSolver(CpuStandInSolver):
    """Answers window `k` of every batch with `status` and a certificate's statistics; records set_options."""

    def __init__(self, marks):
        super().__init__()
        self.marks = marks
        self.options = []

    def set_options(self, **kw):
        self.options.append(kw)

    def solve(self, lps):
        out = super().solve(lps)
        for k, status in self.marks.items():
            out[k].status = status
            out[k].obj = np.inf if status == 1 else -np.inf
            out[k].primal_res_rel, out[k].dual_res_rel, out[k].gap_rel = 12.5, 0.0, 0.0
        return out


def test_certified_window_is_saved_without_the_reference_solve():
    sc = FakeScenario(n_windows=4)
    solver = MarkingSolver({1: 1})
    dropin.batched_optimize_problem_loop(sc, solver=solver, exporter=FakeExporter([]), certify=True)
    assert solver.options == [{"certify": 1}] and solver.calls == [4]
    assert sc.reference_solves == []
    st = {w: (prob.status, err) for w, prob, err, _ in sc.saved}
    assert st == {0: ("optimal", None), 1: ("infeasible", None), 2: ("optimal", None), 3: ("optimal", None)}
    rep = sc.dervet_hip_report
    assert rep.certified == 1 and rep.gpu == 4 and rep.retried == 0
    assert rep.as_dict()["certified"] == 1 and rep.as_dict()["retried_status"] == {}


def test_unbounded_verdict_and_uncertified_failures_with_certify():
    """An unbounded ray is saved as "unbounded"; a window that only ran out of iterations still goes to the
    reference solve."""
    sc = FakeScenario(n_windows=4)
    solver = MarkingSolver({0: 2, 3: 3})
    dropin.batched_optimize_problem_loop(sc, solver=solver, exporter=FakeExporter([]), certify=True)
    st = {w: prob.status for w, prob, _, _ in sc.saved}
    assert st[0] == "unbounded" and st[3] == "optimal"
    assert [id(lp) for lp in sc.reference_solves] == [id(sc.lps[3])]
    rep = sc.dervet_hip_report.as_dict()
    assert rep["certified"] == 1 and rep["retried"] == 1 and rep["retried_status"] == {"optimal_inaccurate": 1}


def test_default_keeps_the_retry():
    sc = FakeScenario(n_windows=4)
    solver = MarkingSolver({1: 1})
    dropin.batched_optimize_problem_loop(sc, solver=solver, exporter=FakeExporter([]))
    assert solver.options == []  # the handle's options are not touched
    assert [id(lp) for lp in sc.reference_solves] == [id(sc.lps[1])]
    assert all(prob.status == "optimal" for _, prob, _, _ in sc.saved)
    rep = sc.dervet_hip_report.as_dict()
    assert rep["certified"] == 0 and rep["retried"] == 1 and rep["retried_status"] == {"infeasible": 1}


def test_cases_loop_and_install_pass_certify_through():
    cases_ = [FakeScenario(n_windows=2, scen=0), FakeScenario(n_windows=2, scen=1)]
    solver = MarkingSolver({3: 1})
    dropin.batched_cases_loop(cases_, solver=solver, exporter=FakeExporter([]), certify=True)
    assert [c.dervet_hip_report.certified for c in cases_] == [0, 1]
    assert not cases_[0].reference_solves and not cases_[1].reference_solves
    mod = types.SimpleNamespace(MicrogridScenario=FakeScenario)
    cls = dropin.install(mod, certify=True)
    assert cls.dervet_hip_certify is True and cls.dervet_hip_options[1:] == (False, True)
    assert dropin.install(mod, certify=True) is cls
    cls2 = dropin.install(mod)  # the default again: re-installed over the reference class, certificates off
    assert cls2 is not cls and cls2.__bases__[0] is FakeScenario and cls2.dervet_hip_certify is False
