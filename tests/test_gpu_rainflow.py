"""GPU: dvh_cycle_damage (csrc/dvh_degradation.hip) -- rainflow cycle damage of SOE profiles, one wave per profile,
bit-equal to degradation.cycle_damage on every branch of the counter (tests/rainflow_cases.py, the list the CPU
build of the same header passes in tests/test_rainflow_native.py), at every workgroup shape the launcher picks (four,
two and one profile per workgroup, a ragged last workgroup), through a row stride, and run to run."""
import numpy as np
import pytest

import rainflow_cases
from dervet_hip import _lib, degradation

pytestmark = pytest.mark.gpu
UPPER, LIFE = degradation.cycle_life_table()


def device_damage(solver, x, e, T=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x, np.float64)).to("cuda:0")
    return degradation.cycle_damage_device(t, e, UPPER, LIFE, solver, T=T).cpu().numpy()


def soe_like(S, T, seed):
    """Random walks clipped to [0, E]: flat stretches at both limits, like a solved SOE profile."""
    rng = np.random.default_rng(seed)
    E = rng.uniform(500.0, 10000.0, S)
    x = np.clip(0.5 * E[:, None] + np.cumsum(rng.normal(size=(S, T)), axis=1) * 0.08 * E[:, None], 0.0, E[:, None])
    return x, E


def test_shape_list_in_one_call(gpu_solver):
    x, e = rainflow_cases.stacked_one_length(UPPER)
    got = device_damage(gpu_solver, x, e)
    assert np.array_equal(got, degradation.cycle_damage(x, e, UPPER, LIFE))
    assert (got > 0).any()


def test_shape_list_at_each_length_through_the_stride(gpu_solver):
    """Every shape at its own length (T = 0, 1, 2, 3 among them): the rows of one length in one call on the padded
    array, whose padding (NaN) must not be read."""
    x, lens, e, names = rainflow_cases.stacked(UPPER)
    for T in sorted(set(lens)):
        rows = np.nonzero(lens == T)[0]
        got = device_damage(gpu_solver, x[rows], e[rows], T=int(T))
        want = degradation.cycle_damage(x[rows, :T], e[rows], UPPER, LIFE)
        assert np.array_equal(got, want), [names[i] for i in rows]
        for i, r in enumerate(rows):
            assert got[i] == rainflow_cases.oracle_damage(x[r, :T], e[r], UPPER, LIFE), names[r]


@pytest.mark.parametrize("S,T,stride", [(1, 744, 744), (257, 100, 100), (64, 744, 744), (9, 769, 800),
                                        (1, 8784, 8784),                 # an hourly leap year
                                        (3, 8784, 8784),                 # two profiles per workgroup, the last ragged
                                        (2, _lib.RAINFLOW_MAX_T, _lib.RAINFLOW_MAX_T)])  # one, all of the LDS
def test_equals_host_cycle_damage(gpu_solver, S, T, stride):
    x, e = soe_like(S, stride, seed=S + T)
    got = device_damage(gpu_solver, x, e, T=T)
    assert np.array_equal(got, degradation.cycle_damage(x[:, :T], e, UPPER, LIFE))
    assert (got > 0).all()


def test_random_walks_with_per_row_energy(gpu_solver):
    x, e = rainflow_cases.walks()
    assert np.array_equal(device_damage(gpu_solver, x, e), degradation.cycle_damage(x, e, UPPER, LIFE))


def test_two_runs_give_identical_bits(gpu_solver):
    x, e = soe_like(300, 744, seed=2)
    a, b = device_damage(gpu_solver, x, e), device_damage(gpu_solver, x, e)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _raw(solver, ene, stride, S, T, e, up, lf, n_table, out):
    """The entry point itself, on the handle's own stream (NULL): the caller orders it with torch by hand."""
    p = lambda t: None if t is None else t.data_ptr()
    rc = solver._lib.dvh_cycle_damage(solver._h, p(ene), stride, S, T, p(e), p(up), p(lf), n_table, p(out), None)
    return rc, solver._lib.dvh_last_error(solver._h).decode()


def test_unsupported_and_bad_arguments(gpu_solver):
    import torch
    f64 = dict(dtype=torch.float64, device="cuda:0")
    ene, e, out = torch.zeros(4, 16, **f64), torch.ones(4, **f64), torch.full((4,), -1.0, **f64)
    up, lf = torch.as_tensor(UPPER).to(**f64), torch.as_tensor(LIFE).to(**f64)
    n = len(UPPER)
    torch.cuda.synchronize()
    T = _lib.RAINFLOW_MAX_T + 1   # refused before anything is launched: the rows are never read
    rc, msg = _raw(gpu_solver, ene, T, 4, T, e, up, lf, n, out)
    assert rc == _lib.DVH_ERR_UNSUPPORTED and "LDS" in msg
    for args in [(ene, 16, -1, 16, e, up, lf, n, out), (ene, 16, 4, -1, e, up, lf, n, out),
                 (ene, 15, 4, 16, e, up, lf, n, out), (None, 16, 4, 16, e, up, lf, n, out),
                 (ene, 16, 4, 16, None, up, lf, n, out), (ene, 16, 4, 16, e, None, lf, n, out),
                 (ene, 16, 4, 16, e, up, None, n, out), (ene, 16, 4, 16, e, up, lf, n, None),
                 (ene, 16, 4, 16, e, up, lf, 0, out), (ene, 16, 4, 16, e, up, lf, _lib.RAINFLOW_MAX_TABLE + 1, out)]:
        rc, msg = _raw(gpu_solver, *args)
        assert rc == _lib.DVH_ERR_ARG and len(msg) > 8, args[1:4]
    assert gpu_solver._lib.dvh_cycle_damage(None, ene.data_ptr(), 16, 4, 16, e.data_ptr(), up.data_ptr(), lf.data_ptr(),
                                            n, out.data_ptr(), None) == _lib.DVH_ERR_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1.0).all()          # no refused call wrote anything
    rc, _ = _raw(gpu_solver, ene, 16, 4, 16, e, up, lf, n, out)   # and the same call, well formed, runs
    assert rc == 0
    gpu_solver._check(gpu_solver._lib.dvh_synchronize(gpu_solver._h), "dvh_synchronize")
    assert np.array_equal(out.cpu().numpy(), degradation.cycle_damage(np.zeros((4, 16)), 1.0, UPPER, LIFE))
