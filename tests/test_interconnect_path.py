"""The kernel-path name of the band kernel's interconnection form (dvh_set_kernel_path mode 5; no GPU needed)."""
from dervet_hip.solver import BatchSolver


def test_interconnect_is_kernel_path_5():
    assert BatchSolver._PATHS["interconnect"] == 5
    assert sorted(BatchSolver._PATHS.values()) == list(range(6))
