"""Drop-in: the ``certify`` argument's level reaches the solver handle (dervet_hip.dropin): ``certify=True`` stays
level 1, ``certify=2`` (the early exit for infeasible windows inside the PDHG kernels) is forwarded, and ``install``
compares the level, not its truth value.  CPU only: the solver is a recording fake."""
import types

from dervet_hip import dropin


class RecordingSolver:
    def __init__(self):
        self.options, self.calls = [], []

    def set_options(self, **kw):
        self.options.append(kw)

    def solve(self, lps):
        self.calls.append(len(lps))
        return [types.SimpleNamespace(status=0) for _ in lps]


def _plans(n):
    return [types.SimpleNamespace(win=types.SimpleNamespace(lp=object())) for _ in range(n)] + \
        [types.SimpleNamespace(win=None)]  # (a MILP window: not sent)


def test_level_is_forwarded_to_the_handle():
    for arg, want in ((True, 1), (1, 1), (2, 2)):
        s = RecordingSolver()
        res = dropin._solve_plans(_plans(3), s, arg)
        assert s.options == [{"certify": want}] and s.calls == [3] and sorted(res) == [0, 1, 2]
    s = RecordingSolver()
    dropin._solve_plans(_plans(2), s)
    assert s.options == [] and s.calls == [2]  # the default leaves the handle's options alone


class Scenario:
    pass


def test_install_compares_the_level():
    mod = types.SimpleNamespace(MicrogridScenario=Scenario)
    one = dropin.install(mod, certify=True)
    assert one.dervet_hip_certify is True and one.dervet_hip_certify_level == 1
    assert dropin.install(mod, certify=1) is one
    two = dropin.install(mod, certify=2)
    assert two is not one and two.__bases__[0] is Scenario
    assert two.dervet_hip_certify is True and two.dervet_hip_certify_level == 2
    assert dropin.install(mod, certify=2) is two
    off = dropin.install(mod)
    assert off is not two and off.dervet_hip_certify is False and off.dervet_hip_certify_level == 0
