"""CPU: the bill of an EV window (dervet_hip/valuation.py bill_windows_host with has_ev), the C layout of the fields
the EV adds to dvh_battery_group and dvh_bill_group, the entry points' argument errors, and the device builder's
step-code validator (csrc/dvh_build_validate.h) under AddressSanitizer / UBSan in a stand-alone program."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ev_ref as ref
from dervet_hip import _lib, valuation as V
from dervet_hip.lp import builder
from oracle import window_lp
from planted_lp import from_window

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "der-vet_amd", "csrc")


@pytest.mark.parametrize("T,J,pl,tg", ref.SHAPES[:6], ids=ref.IDS[:6])
def test_host_bill_reproduces_the_window_objective(T, J, pl, tg):
    """Retail energy charge + demand charge (at the dispatch's own peaks) + variable O&M + the constants the bill does
    not carry (the battery's and the EV's fixed O&M) is the window's objective with tau at those peaks."""
    g = ref.group(T, J, pl, tg)
    inp = V.bill_inputs(g)
    assert inp.has_ev and inp.need == g.n == 5 * T + J
    xs = []
    for w in builder.group_window_lps(g):
        h = window_lp.solve_highs(from_window(w))
        assert h["status"] == 0
        xs.append(h["x"])
    x = np.array(xs)
    bills, peaks, bad = V.bill_windows_host(g, x)
    assert not bad.any()
    ch, dis, ev_ch = x[:, :T], x[:, T:2 * T], x[:, 3 * T + J:4 * T + J]
    assert np.array_equal(peaks, np.array([[(((g.inputs["base"][k] + ch[k]) - dis[k]) + ev_ch[k])[g.inputs["dcm_t"][g.inputs["dcm_j"] == j]].max()
                                            for j in range(J)] for k in range(g.G)]).reshape(g.G, J))
    x_pk = x.copy()
    x_pk[:, 3 * T:3 * T + J] = peaks
    terms = builder.evaluate_terms(g, x_pk)
    want = (g.c * x_pk).sum(axis=1) + g.c0
    got = bills[:, V.RETAIL] + bills[:, V.DEMAND] + bills[:, V.VAR_OM] + terms["ev fixed_om"] + terms["es fixed_om"]
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)
    # the EV is a DER: the original rows are the site load's alone
    plain, _, _ = V.bill_windows_host(ref.group(T, J, pl, tg, ch_max=None), x[:, :3 * T + J])
    assert np.array_equal(bills[:, V.ORIG_RETAIL:], plain[:, V.ORIG_RETAIL:])
    # and the optimum's tau are the peaks within the solver's tolerance
    assert np.allclose(x[:, 3 * T:3 * T + J], peaks, rtol=1e-7, atol=1e-6)


def test_a_short_solution_is_a_bad_window_and_ctrl_load_groups_are_still_refused():
    import ctrl_load_ref as cl
    T, J, pl, tg = ref.SHAPES[0]
    g = ref.group(T, J, pl, tg)
    _, _, bad = V.bill_windows_host(g, [np.zeros(g.n), np.zeros(3 * T + J)])
    assert bad.tolist() == [0, V.BAD_WINDOW]
    with pytest.raises(NotImplementedError):
        V.bill_inputs(cl.group(24, 1, [0]))


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dervet_hip.h"\nint main() { std::printf("%zu %zu %zu %zu '
                   '%zu %zu %zu %d %d\\n", sizeof(dvh_battery_group), sizeof(dvh_bill_group), '
                   'offsetof(dvh_battery_group, has_ev), offsetof(dvh_battery_group, ev_ch_max), '
                   'offsetof(dvh_battery_group, ev_target), offsetof(dvh_battery_group, ev_code), '
                   'offsetof(dvh_bill_group, has_ev), DVH_EV_START, DVH_EV_TRAIL); }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    B, L = _lib.BatteryGroup, _lib.BillGroup
    assert got == [ctypes.sizeof(B), ctypes.sizeof(L), B.has_ev.offset, B.ev_ch_max.offset, B.ev_target.offset,
                   B.ev_code.offset, L.has_ev.offset, builder.EV_START, builder.EV_TRAIL]
    assert B.ice_cost.offset < B.has_ev.offset and L.ice_cost.offset < L.has_ev.offset  # appended: older fields stay put
    assert (builder.EV_PLUGGED, builder.EV_START_TARGET, builder.EV_LAST, builder.EV_END_TARGET, builder.EV_END_R) == \
        (1, 4, 8, 16, 32)


def test_null_handle_and_null_arguments_are_codes():
    lib = _lib.load()
    g = _lib.BatteryGroup()
    g.has_ev = 1
    assert lib.dvh_build_battery_group(None, ctypes.byref(g), None, 0) == _lib.DVH_ERR_ARG
    b = _lib.BillGroup()
    b.has_ev = 1
    assert lib.dvh_bill_windows(None, ctypes.byref(b), None, 0, None, None, None, None) == _lib.DVH_ERR_ARG


@pytest.fixture(scope="module")
def sanitized_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("asan") / "ev_codes_sanitize")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "native", "ev_codes_sanitize.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)


def test_sanitized_run_is_clean(sanitized_run):
    p = sanitized_run
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    assert p.stdout.rstrip().endswith("done") and "failures=0" in p.stdout and "FAILED" not in p.stdout
    for case in ("one_session", "leading_and_trailing", "one_step_session", "month"):
        assert f"{case} ok" in p.stdout


@pytest.mark.parametrize("case", ["null_codes", "null_out", "empty", "unknown_flag", "negative", "start_value_without_row",
                                  "end_value_inside_cycle", "two_end_values", "recurrence_on_last_step",
                                  "start_inside_cycle", "cycle_without_start", "trail_not_plugged",
                                  "trail_not_reaching_end", "R_elsewhere", "trail_without_R", "start_on_trail",
                                  "no_start_row"])
def test_malformed_codes_are_refused_with_a_message(sanitized_run, case):
    m = re.search(rf"^{case} err=(.*)$", sanitized_run.stdout, re.M)
    assert m and len(m.group(1)) > 8, sanitized_run.stdout[-1500:]


def test_the_validator_accepts_what_the_builder_emits(tmp_path):
    """Every shared shape's codes through the C validator (a plain build of the same header): D and the entry count are
    the host group's."""
    src = tmp_path / "scan.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "dvh_build_validate.h"\nint main(int argc, char** argv) {\n'
                   '  std::vector<int32_t> c;\n  for (int i = 1; i < argc; ++i) c.push_back(std::atoi(argv[i]));\n'
                   '  dvh::EvScan s;\n  const std::string msg = dvh::scan_ev_codes(c.data(), (int32_t)c.size(), &s);\n'
                   '  std::printf("%s|%d %d %d\\n", msg.c_str(), s.D, s.nnz, s.n_trail);\n}\n')
    exe = str(tmp_path / "scan")
    subprocess.run(["g++", "-std=c++17", "-I", CSRC, str(src), "-o", exe], check=True)
    for T, J, pl, tg in ref.SHAPES:
        g = ref.group(T, J, pl, tg, G=1)
        code = g.ev["code"]
        out = subprocess.run([exe] + [str(int(k)) for k in code], capture_output=True, text=True, check=True).stdout
        msg, nums = out.strip().split("|")
        nnz_ev = int(g.indptr[g.m_eq] - g.indptr[T + 1])
        assert msg == "" and [int(v) for v in nums.split()] == \
            [g.m_eq - 2 * T - 1, nnz_ev, int(np.count_nonzero(code & builder.EV_TRAIL))], (T, out)
