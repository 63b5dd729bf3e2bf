"""The kernel-path name of the band kernel's heat form (dvh_set_kernel_path mode 7; no GPU needed).  The name lives in a
table of its own, BatchSolver._CHP_PATHS: _PATHS and _MORE_PATHS keep what tests/test_interconnect_path.py and
tests/test_load_shift_path.py pin."""
import pytest

from dervet_hip.solver import BatchSolver


class _Lib:
    def __init__(self):
        self.modes = []

    def dvh_set_kernel_path(self, h, mode):
        self.modes.append(mode)
        return 0


def test_chp_is_kernel_path_7_and_the_earlier_tables_are_unchanged():
    assert BatchSolver._CHP_PATHS == {"chp": 7}
    assert BatchSolver._MORE_PATHS == {"load_shift": 6}
    assert BatchSolver._PATHS == dict(default=0, generic=1, ell=2, band1=3, band3=4, interconnect=5)
    s = BatchSolver.__new__(BatchSolver)  # (no handle: set_kernel_path only maps the name and calls the library)
    s._lib, s._h = _Lib(), None
    for name in ("chp", "load_shift", "interconnect", "default", True):
        s.set_kernel_path(name)
    assert s._lib.modes == [7, 6, 5, 0, 1]
    with pytest.raises(KeyError):
        s.set_kernel_path("heat")
