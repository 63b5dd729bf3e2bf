"""GPU: the device builder's EV block (csrc/dvh_build.hip has_ev via lp/gpu_builder.py): the windows it expands in HBM
are bit-identical to builder.battery_group(ev=...)'s, descriptors included, and solve within the project's bars; a
descriptor or a code array that disagrees with the layout is DVH_ERR_ARG with a message, and nothing is written."""
import ctypes

import numpy as np
import pytest
import torch

import ev_ref as ref
from dervet_hip import _lib
from dervet_hip.lp import builder, gpu_builder
from oracle import window_lp
from planted_lp import from_window

pytestmark = pytest.mark.gpu

FIELDS = ("desc", "indptr", "indices", "data", "c", "c0", "q", "l", "u")
G = 3
NAMES = ["T5J1", "T65J4", "T129J1", "T744J4"]
BY_ID = dict(zip(ref.IDS, ref.SHAPES))


def _pair(name, da=False):
    """(host group, device-builder spec) of a shared shape with G = 3 windows of different EV ratings."""
    T, J, pl, tg = BY_ID[name]
    load, retail, masks, dprice = ref.series(T, J, G)
    ev = dict(ch_max=np.array([50.0, 40.0, 62.5]), ene_target=np.array([tg, 0.75 * tg, tg]),
              fixed_om=np.array([3.0, 0.0, 1.25]), plugged=pl)
    kw = dict(retail_price=retail, demand_masks=masks, demand_prices=dprice, ev=ev)
    if da:
        kw["da_price"] = 0.5 * retail[:, ::-1]
    return (builder.battery_group(T, 1.0, load, ref.BAT, **kw),
            gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, **kw))


def _assert_same(dev, host):
    for f in FIELDS:
        a = getattr(dev, f).cpu().numpy()
        b = np.asarray(getattr(host, f))
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tobytes() == b.tobytes(), (f, np.flatnonzero(a != b)[:5])


@pytest.mark.parametrize("name", NAMES)
def test_device_builder_is_bit_identical_and_the_batch_solves(gpu_solver, name):
    host, spec = _pair(name)
    dev = gpu_builder.pack_specs_device([spec], gpu_solver)
    _assert_same(dev, builder.pack_groups([host]))
    try:
        gpu_solver.set_kernel_path("load_shift")
        gpu_solver.solve_packed(dev)
        ks = gpu_solver.kernel_stats()
    finally:
        gpu_solver.set_kernel_path("default")
    torch.cuda.synchronize()
    assert ks["band_windows"] == G and ks["ell_windows"] == ks["generic_windows"] == 0, ks
    ist = dev.istats.cpu().numpy()
    for k, lp in enumerate(builder.group_window_lps(host)):
        x = dev.window(k)["x"]
        h = window_lp.solve_highs(from_window(lp))
        obj = float(lp.c @ x) + lp.c0
        pres = window_lp.primal_residual_rel(from_window(lp), x)[0]
        print(f"EV device-built {name} window {k}: obj {obj:.9g} HiGHS {h['obj']:.9g} primal residual {pres:.2e}")
        assert h["status"] == 0 and ist[k, 0] == 0, (k, ist[k])
        assert abs(obj - h["obj"]) <= 1e-5 * abs(h["obj"]) and pres <= 1e-6, (k, obj, h["obj"], pres)


def test_mixed_groups_with_da_prices_in_one_batch(gpu_solver):
    """An EV group between two plain ones, DA and retail prices both: the EV rows shift nothing of their neighbours."""
    T, J, pl, tg = BY_ID["T65J4"]
    load, retail, masks, dprice = ref.series(T, J, G)
    kw = dict(retail_price=retail, demand_masks=masks, demand_prices=dprice)
    plain_h = builder.battery_group(T, 1.0, load, ref.BAT, **kw)
    plain_s = gpu_builder.battery_group_spec(T, 1.0, load, ref.BAT, **kw)
    ev_h, ev_s = _pair("T65J4", da=True)
    small_h, small_s = _pair("T5J1")
    assert "ev DA" in ev_h.terms
    dev = gpu_builder.pack_specs_device([plain_s, ev_s, small_s, plain_s], gpu_solver)
    _assert_same(dev, builder.pack_groups([plain_h, ev_h, small_h, plain_h]))


def _call(gpu_solver, spec, edit_desc=None, edit_group=None, code=None):
    """dvh_build_battery_group on sentinel-filled arrays; returns (rc, message, arrays untouched)."""
    desc, sz = gpu_builder.desc_of([spec])
    if edit_desc:
        edit_desc(desc, sz)
    dev = torch.device("cuda:0")
    from dervet_hip.packed import PackedBatch
    f64 = dict(dtype=torch.float64, device=dev)
    pb = PackedBatch(desc=torch.as_tensor(desc).to(dev), indptr=torch.full((sz["rows"],), -7, dtype=torch.int32, device=dev),
                     indices=torch.full((sz["nnz"],), -7, dtype=torch.int32, device=dev), data=torch.full((sz["nnz"],), -7.0, **f64),
                     c=torch.full((sz["n"],), -7.0, **f64), c0=torch.full((len(desc),), -7.0, **f64),
                     q=torch.full((sz["m"],), -7.0, **f64), l=torch.full((sz["n"],), -7.0, **f64),
                     u=torch.full((sz["n"],), -7.0, **f64)).alloc_outputs()
    up = lambda a, t=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=t)  # noqa: E731
    keep = dict(dcm_t=up(spec.dcm_t, torch.int32), dcm_j=up(spec.dcm_j, torch.int32), base=up(spec.base),
                retail=up(spec.retail), demand=up(spec.demand), c0=up(spec.c0), chm=up(spec.ev["ch_max"]),
                tgt=up(spec.ev["ene_target"]), **{k: up(v) for k, v in spec.scal.items()})
    g = _lib.BatteryGroup()
    g.T, g.J, g.G, g.mI, g.dt, g.has_retail, g.has_ev = spec.T, spec.J, spec.G, len(spec.dcm_t), spec.dt, 1, 1
    for name in ("dcm_t", "dcm_j", "base", "retail", "demand", "c0", *spec.scal):
        setattr(g, name, keep[name].data_ptr())
    g.ev_ch_max, g.ev_target = keep["chm"].data_ptr(), keep["tgt"].data_ptr()
    code = np.ascontiguousarray(spec.ev["code"] if code is None else code, np.int32)
    g.ev_code = code.ctypes.data
    if edit_group:
        edit_group(g)
    torch.cuda.synchronize()
    p = pb.as_ctypes()
    rc = gpu_solver._lib.dvh_build_battery_group(gpu_solver._h, ctypes.byref(g), ctypes.byref(p), 0)
    msg = gpu_solver._lib.dvh_last_error(gpu_solver._h).decode()
    gpu_solver._check(gpu_solver._lib.dvh_synchronize(gpu_solver._h), "dvh_synchronize")
    torch.cuda.synchronize()
    clean = all(bool((getattr(pb, f) == -7).all()) for f in FIELDS[1:])
    return rc, msg, clean


def _desc(col, delta):
    def edit(desc, sz):
        desc[:, col] += delta
    return edit


def test_a_valid_direct_call_builds(gpu_solver):
    rc, msg, clean = _call(gpu_solver, _pair("T65J4")[1])
    assert rc == 0 and not clean, msg


@pytest.mark.parametrize("case", ["m_eq_of_the_battery", "one_row_short", "one_entry_short", "n_without_the_block",
                                  "codes_of_another_mask", "recurrence_on_the_last_step", "unknown_flag", "null_codes",
                                  "null_ch_max", "with_ice"])
def test_a_descriptor_or_codes_that_disagree_are_refused_and_nothing_is_written(gpu_solver, case):
    spec = _pair("T65J4")[1]
    T, code = spec.T, spec.ev["code"]
    other = builder.ev_codes(ref._mask(T, [20, 21, 22, 40, 41, 62, 63, 64]), T)  # one more session: three more start rows
    last = code.copy()
    last[T - 1] &= ~(builder.EV_LAST | builder.EV_END_R)
    flag = code.copy()
    flag[3] |= 128
    kw = {"m_eq_of_the_battery": dict(edit_desc=lambda d, sz: d.__setitem__((slice(None), 2), T + 1)),
          "one_row_short": dict(edit_desc=_desc(1, -1)), "one_entry_short": dict(edit_desc=_desc(3, -1)),
          "n_without_the_block": dict(edit_desc=_desc(0, -2 * T)), "codes_of_another_mask": dict(code=other),
          "recurrence_on_the_last_step": dict(code=last), "unknown_flag": dict(code=flag),
          "null_codes": dict(edit_group=lambda g: setattr(g, "ev_code", None)),
          "null_ch_max": dict(edit_group=lambda g: setattr(g, "ev_ch_max", None)),
          "with_ice": dict(edit_group=lambda g: setattr(g, "has_ice", 1))}[case]
    assert not np.array_equal(other, code)
    rc, msg, clean = _call(gpu_solver, spec, **kw)
    assert rc == _lib.DVH_ERR_ARG and len(msg) > 8 and clean, (rc, msg, clean)
