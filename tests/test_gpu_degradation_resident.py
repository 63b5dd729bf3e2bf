"""GPU: the wear update between two window positions on the device (dvh_degradation_update,
degradation.DeviceDegradation) and the degradation-coupled sweep that keeps its capacities in HBM
(DegradationSweep.run(resident=True)).  The update equals Degradation.update field for field on a hand-built batch;
the resident sweep equals the existing spec-built sweep for equality, and holds device tensors only until its one
gather at the end."""
import ctypes
import warnings

import numpy as np
import pytest

from dervet_hip import _lib, degradation
from dervet_hip.lp import scenarios
from dervet_hip.packed import PackedBatch

pytestmark = pytest.mark.gpu
S, T = 5, 12
N = 3 * T + 1          # battery + demand-charge window: x = [ch, dis, ene, tau], the SOE profile at 2 T .. 3 T - 1


def _hand_batch(x, status):
    """A packed batch of S solved windows of which only what the update reads is meaningful: descriptors, x, istats."""
    import torch
    desc = np.zeros((S, 8), np.int64)
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3] = N, 1, 1, 1
    desc[:, 4], desc[:, 5], desc[:, 6], desc[:, 7] = 2 * np.arange(S), np.arange(S), N * np.arange(S), np.arange(S)
    z = np.zeros
    pb = PackedBatch(desc=desc, indptr=z(2 * S, np.int32), indices=z(S, np.int32), data=z(S), c=z(S * N), c0=z(S),
                     q=z(S), l=z(S * N), u=z(S * N)).to_torch("cuda:0").alloc_outputs()
    pb.x.copy_(torch.as_tensor(np.ascontiguousarray(x).ravel()))
    pb.istats[:, 0] = torch.as_tensor(np.asarray(status, np.int32)).to("cuda:0")
    return pb


def _profiles(rng, e_rated, deep):
    x = rng.normal(size=(S, N)) * 1e6                                    # ch / dis / tau: must not be read
    ene = rng.uniform(0.2, 0.8, (S, T)) * e_rated[:, None]
    ene[deep] = np.tile([0.0, e_rated[deep]], T // 2)                    # full cycles: this battery wears fast
    x[:, 2 * T:3 * T] = ene
    return x, ene


def test_update_equals_degradation_update_on_a_hand_built_batch(gpu_solver):
    """Three successive updates; battery 1 sits at its state of health and is replaced, battery 2 (the same, not
    replaceable) stays worn; one window per update is not OPTIMAL."""
    import torch
    rng = np.random.default_rng(8)
    e_rated = np.array([4000.0, 900.0, 900.0, 5200.5, 777.0])

    def make():
        d = degradation.Degradation(e_rated, yearly_degrade=[2.0, 1.5, 1.5, 0.0, 3.25], eol_condition=77.5,
                                    state_of_health=[73, 90, 90, 73, 60], replaceable=[True, True, False, True, False])
        d.degrade_perc[1:3] = 0.0999   # capacity 810.09 kWh: just above 90 % of 900, below it after one window
        return d

    host, mirror = make(), make()
    dd = degradation.DeviceDegradation(mirror, gpu_solver, "cuda:0")
    assert np.array_equal(dd.capacity.cpu().numpy(), host.capacity())
    for k, status in enumerate(([0, 0, 0, 3, 0], [1, 0, 0, 0, 0], [0, 0, 4, 0, 0])):
        x, ene = _profiles(rng, e_rated, 1)
        ene[2] = ene[1]
        x[2, 2 * T:3 * T] = ene[2]
        days = T / 24.0 + 0.37 * k
        cap_before = dd.capacity
        want = host.update(ene, days, valid=np.array(status) == 0, year=2017 + k)
        got = dd.update(_hand_batch(x, status), T, days, year=2017 + k)
        assert isinstance(got, torch.Tensor) and got.is_cuda and dd.capacity.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), k
        assert np.array_equal(dd.degrade_perc.cpu().numpy(), host.degrade_perc), k
        assert np.array_equal(dd.capacity.cpu().numpy(), host.capacity()), k
        assert np.array_equal(dd.replacements.cpu().numpy(), host.replacements)
        assert np.array_equal(dd.skipped.cpu().numpy(), host.skipped)
        assert dd.capacity is not cap_before            # the tensor a builder was handed stays what it was
    assert host.replacements[1] >= 1 and host.replacements[2] == 0 and list(host.skipped) == [1, 0, 1, 1, 0]
    assert host.capacity()[2] <= 0.9 * 900.0
    dd.sync_to(mirror)
    for f in ("degrade_perc", "replacements", "skipped"):
        assert np.array_equal(getattr(mirror, f), getattr(host, f)), f
    assert mirror.years_degraded == host.years_degraded
    assert host.years_degraded[1] == {2017} and host.years_degraded[2] == {2017, 2018, 2019}


def test_update_with_the_module_off_writes_zeros(gpu_solver):
    rng = np.random.default_rng(9)
    e_rated = np.array([4000.0, 900.0, 900.0, 5200.5, 777.0])
    deg = degradation.Degradation(e_rated, yearly_degrade=10.0, incl_cycle_degrade=False)
    dd = degradation.DeviceDegradation(deg, gpu_solver, "cuda:0")
    x, ene = _profiles(rng, e_rated, 1)
    got = dd.update(_hand_batch(x, [0] * S), T, 0.5)
    assert np.array_equal(got.cpu().numpy(), deg.update(ene, 0.5)) and not got.cpu().numpy().any()
    assert np.array_equal(dd.capacity.cpu().numpy(), e_rated) and not dd.reached.cpu().numpy().any()
    assert not dd.degrade_perc.cpu().numpy().any() and not dd.skipped.cpu().numpy().any()


def test_update_never_reads_a_profile_outside_its_window(gpu_solver):
    """ene_col + T beyond the window's n: caught on the device (the descriptors live there); the window is not
    counted -- calendar loss only, skipped -- and nothing outside it is read."""
    rng = np.random.default_rng(10)
    e_rated = np.array([4000.0, 900.0, 900.0, 5200.5, 777.0])
    host = degradation.Degradation(e_rated, yearly_degrade=2.0)
    dd = degradation.DeviceDegradation(degradation.Degradation(e_rated, yearly_degrade=2.0), gpu_solver, "cuda:0")
    x, ene = _profiles(rng, e_rated, 1)
    pb = _hand_batch(x, [0] * S)
    pb.desc[3, 0] = 3 * T - 1            # window 3 now ends inside its SOE block
    want = host.update(ene, 0.5, valid=np.arange(S) != 3)
    assert np.array_equal(dd.update(pb, T, 0.5).cpu().numpy(), want)
    assert list(dd.skipped.cpu().numpy()) == [0, 0, 0, 1, 0]


def test_update_refuses_bad_arguments(gpu_solver):
    import torch
    e_rated = np.array([4000.0, 900.0, 900.0, 5200.5, 777.0])
    dd = degradation.DeviceDegradation(degradation.Degradation(e_rated), gpu_solver, "cuda:0")
    pb = _hand_batch(np.zeros((S, N)), [0] * S)
    p = pb.as_ctypes()
    st = _lib.DegradationState()
    st.incl_cycle_degrade = 1
    out = {f: torch.full((S,), -1, dtype=t, device="cuda:0")
           for f, t in (("capacity", torch.float64), ("degradation", torch.float64), ("reached", torch.int32))}
    for f in ("e_rated", "yearly", "soh", "replaceable", "degrade_perc", "replacements", "skipped"):
        setattr(st, f, getattr(dd, f).data_ptr())
    for f, t in out.items():
        setattr(st, f, t.data_ptr())
    lib, h = gpu_solver._lib, gpu_solver._h
    stream = None          # the handle's own stream: ordered with torch by hand (synchronize) below
    torch.cuda.synchronize()

    def call(first=0, n=S, steps=T, col=2 * T, days=0.5, eol=80.0, n_table=len(dd.upper), state=st, batch=p):
        rc = lib.dvh_degradation_update(h, None if batch is None else ctypes.byref(batch), first, n, steps, col, days,
                                        eol, dd.upper.data_ptr(), dd.life.data_ptr(), n_table,
                                        None if state is None else ctypes.byref(state), stream)
        return rc, lib.dvh_last_error(h).decode()

    for kw in (dict(n=-1), dict(steps=-1), dict(col=-1), dict(first=-1), dict(first=1), dict(col=S * N),
               dict(days=float("nan")), dict(days=float("inf")), dict(eol=float("nan")), dict(n_table=0),
               dict(n_table=65), dict(state=None), dict(batch=None)):
        rc, msg = call(**kw)
        assert rc == _lib.DVH_ERR_ARG and len(msg) > 8, kw
    rc, msg = call(steps=_lib.RAINFLOW_MAX_T + 1, col=0)
    assert rc in (_lib.DVH_ERR_ARG, _lib.DVH_ERR_UNSUPPORTED)    # (beyond this small batch's columns: an argument error)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == -1).all() for t in out.values())
    assert call()[0] == 0
    torch.cuda.synchronize()
    host = degradation.Degradation(e_rated)          # (a flat profile is one zero-range half cycle)
    assert np.array_equal(out["degradation"].cpu().numpy(), host.update(np.zeros((S, T)), 0.5))
    assert np.array_equal(out["capacity"].cpu().numpy(), host.capacity())


def _host_sweep(ids, E, solver, positions):
    deg = degradation.Degradation(E, yearly_degrade=2.0)
    sw = degradation.DegradationSweep(lambda k, cap: scenarios.config4(ids, E=cap, only=[k], spec=True), positions, deg)
    return sw.run(solver), deg


def test_resident_sweep_equals_spec_built_sweep(gpu_solver):
    """6 config-4 scenarios x 4 positions: same dispatch, iterations, objective, wear and capacities as the existing
    device-built sweep, bit for bit; and the per-position results are device tensors until the one gather."""
    import torch
    ids = list(range(6))
    P = scenarios.sweep_parameters(ids)
    host, dh = _host_sweep(ids, P["E"], gpu_solver, range(4))
    deg = degradation.Degradation(P["E"], yearly_degrade=2.0)
    sw = degradation.DegradationSweep(lambda k, cap: scenarios.config4(ids, E=cap, only=[k], spec=True), range(4), deg)
    res = sw.run(gpu_solver, resident=True)
    assert len(res) == len(host) == 4
    for a, b in zip(host, res):
        assert set(a) == set(b) and a["k"] == b["k"]
        for f in ("ene", "iters", "status", "obj", "degradation", "capacity_before"):
            assert isinstance(b[f], np.ndarray) and np.array_equal(a[f], b[f]), f
        assert len(a["x"]) == len(b["x"]) and all(np.array_equal(u, v) for u, v in zip(a["x"], b["x"]))
    assert (res[3]["capacity_before"] < P["E"]).all()
    # the loop's own products: device tensors, one set per position, nothing on the host
    assert len(sw.device_results) == 4
    for p in sw.device_results:
        for f in ("ene", "istats", "obj", "degradation", "capacity_before", "x"):
            assert isinstance(p[f], torch.Tensor) and p[f].is_cuda, f
    assert sw.device_deg.capacity.is_cuda
    # the host object is where the host path leaves it (run ends with sync_to; once more changes nothing)
    for d in (deg, sw.device_deg.sync_to(degradation.Degradation(P["E"], yearly_degrade=2.0))):
        assert np.array_equal(d.capacity(), dh.capacity())
        assert np.array_equal(d.replacements, dh.replacements) and np.array_equal(d.skipped, dh.skipped)
    assert np.array_equal(sw.device_deg.capacity.cpu().numpy(), dh.capacity())


def test_resident_sweep_without_x_and_timed(gpu_solver):
    ids = list(range(3))
    P = scenarios.sweep_parameters(ids)
    host, _ = _host_sweep(ids, P["E"], gpu_solver, range(2))
    deg = degradation.Degradation(P["E"], yearly_degrade=2.0)
    sw = degradation.DegradationSweep(lambda k, cap: scenarios.config4(ids, E=cap, only=[k], spec=True), range(2), deg)
    res = sw.run(gpu_solver, resident=True, keep_x=False, timed=True)
    for a, b in zip(host, res):
        assert "x" not in b
        for f in ("ene", "iters", "status", "obj", "degradation", "capacity_before"):
            assert np.array_equal(a[f], b[f]), f
    ms = sw.device_deg.update_ms()
    assert len(ms) == 2 and all(0.0 < t < 1e3 for t in ms)


def test_resident_needs_device_builder_specs(gpu_solver):
    ids = list(range(2))
    P = scenarios.sweep_parameters(ids)
    deg = degradation.Degradation(P["E"], yearly_degrade=2.0)
    sw = degradation.DegradationSweep(lambda k, cap: scenarios.config4(ids, E=cap, only=[k]), range(2), deg)
    with pytest.raises(ValueError, match="spec"):
        sw.run(gpu_solver, resident=True)
    assert not deg.degrade_perc.any()


def test_resident_sweep_warns_about_windows_not_optimal(gpu_solver):
    """The RuntimeWarning of the host path, issued at the gather: an iteration limit of 50 leaves windows ITER_LIMIT."""
    from dervet_hip import BatchSolver
    ids = list(range(3))
    P = scenarios.sweep_parameters(ids)
    deg = degradation.Degradation(P["E"], yearly_degrade=2.0)
    sw = degradation.DegradationSweep(lambda k, cap: scenarios.config4(ids, E=cap, only=[k], spec=True), range(2), deg)
    with BatchSolver(0, max_iters=50) as s:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            res = sw.run(s, resident=True, keep_x=False)
    assert any(issubclass(x.category, RuntimeWarning) and "not OPTIMAL" in str(x.message) for x in w)
    assert (res[0]["status"] != 0).any() and deg.skipped.sum() == sum(int((p["status"] != 0).sum()) for p in res)
