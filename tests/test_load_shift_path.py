"""The kernel-path name of the band kernel's load-shift form (dvh_set_kernel_path mode 6; no GPU needed).  The name
lives in BatchSolver._MORE_PATHS: _PATHS keeps the six modes tests/test_interconnect_path.py pins."""
from dervet_hip.solver import BatchSolver


class _Lib:
    def __init__(self):
        self.modes = []

    def dvh_set_kernel_path(self, h, mode):
        self.modes.append(mode)
        return 0


def test_load_shift_is_kernel_path_6_and_the_earlier_modes_keep_their_numbers():
    assert BatchSolver._MORE_PATHS == {"load_shift": 6}
    assert BatchSolver._PATHS == dict(default=0, generic=1, ell=2, band1=3, band3=4, interconnect=5)
    s = BatchSolver.__new__(BatchSolver)  # (no handle: set_kernel_path only maps the name and calls the library)
    s._lib, s._h = _Lib(), None
    for name in ("load_shift", "interconnect", "default", True):
        s.set_kernel_path(name)
    assert s._lib.modes == [6, 5, 0, 1]
