"""The three-step band form's plain iteration with its LDS reads issued first behind each barrier and the Halpern blends
and late rows run under their latency.  Only the order of independent work changes: every value is produced by the same
operations in the same order, so the new library must return the parent commit's bits.

Windows (tests/band_cases.py: READS_SEEDS): those of tests/test_gpu_band_wave0.py (non-zero soc_target and llsoc, forced
"band3") at T = 2, 3, 4, 192, 193, 576, 577, 766, 767, 768 with J = 1, and T = 193 with J = 2 and J = 4, which take the generic
instantiation's other loop body (the per-column tau path on wave 0).

Bars:
  host restatement   iterations within 128 of oracle/pdlp_ref.py, objective within 1e-7 relative, and the result contract
                     recomputed from the returned x, y (tests/result_contract.py; reference optimum: HiGHS);
  unchanged kernel   objective within 1e-9 relative of the one-step form ("band1", whose machine code does not change);
  between variants   bit for bit: the static single-demand-period instantiation against the forced generic one
                     (DVH_BAND_J1=0), the persistent grid against the one-workgroup launch (DVH_BAND_QUEUE=0);
  against the parent bit for bit: the SHA-256 of x || y, the iterations and the status at iteration limits around the check
                     period, cold and from a carried start (tests/band_limits.py), as scripts/dump_band_limits.py
                     recorded them with the parent commit's library in tests/golden/band_limits_parent.json -- work that
                     is pending at a loop exit (in front of a check, at max_iters) is what the other bars could miss;
  restarts           for every T the reference restarts inside one of the runs compared here (asserted on the reference).
"""
import json
import os

import pytest

import band_cases as bc
import band_limits
import result_contract as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, STATIC = bc.GENERIC, bc.STATIC  # kernel_stats()["band_variant"]
FORM_TOL = 1e-9
CASES = bc.READS_SEEDS  # (T, J): seed
KEYS = tuple(CASES)
IDS = [f"T{T}-J{J}" for T, J in KEYS]


@pytest.fixture(scope="module")
def solver():
    yield from bc.open_solver()


@pytest.fixture(scope="module")
def windows():
    return {(T, J): bc.case_window((T, J, CASES[(T, J)])) for T, J in KEYS}


@pytest.fixture(scope="module")
def refs(windows):
    """The oracle dict, pdlp_ref at check period 64, the HiGHS optimum and the reference's restarts of every window
    (the J = 1 windows share the computation with tests/test_gpu_band_wave0.py)."""
    out = {}
    for key, lp in windows.items():
        case = key + (CASES[key],)
        ref, trace = bc.reference(case)
        out[key] = (bc.oracle_lp(lp), ref, bc.optimum(case), bc.restarts(trace))
    return out


@pytest.fixture(scope="module")
def solved(solver, windows):
    """Every window by the default launch of the three-step form, once."""
    return {key: bc.solve(solver, [lp], band_variant=STATIC if key[1] == 1 else GENERIC)[0]
            for key, lp in windows.items()}


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_against_the_host_restatement(solved, refs, key):
    olp, ref, opt, restarts = refs[key]
    r = solved[key]
    print(f"{key}: reference {ref['iters']} iterations, {restarts} restarts")
    assert restarts >= 1, f"{key}: the reference does not restart inside the run"
    assert ref["y"][0] != 0.0, f"{key}: the reference's init-row dual is zero"
    bc.agrees(r, ref, 64, f"{key}")
    rc.check_both(olp, r, opt, f"T {key[0]} J {key[1]}", "band3_J1" if key[1] == 1 else "band3")


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_against_the_one_step_form(solver, windows, solved, key):
    """The one-step form's machine code does not change; the two forms group the tau partial sums differently."""
    a = solved[key]
    b = bc.solve(solver, [windows[key]], "band1")[0]
    print(f"{key}: three-step {a.iters} iterations obj {a.obj!r}; one-step {b.iters} iterations obj {b.obj!r}")
    assert a.status == b.status == 0, (a.status_name, b.status_name)
    assert abs(a.obj - b.obj) <= FORM_TOL * abs(b.obj), f"{key}: obj {a.obj!r} vs the one-step form's {b.obj!r}"


@pytest.mark.parametrize("key", [k for k in KEYS if k[1] == 1], ids=[i for i, k in zip(IDS, KEYS) if k[1] == 1])
def test_static_equals_generic(solver, windows, solved, key):
    with bc.env("DVH_BAND_J1", "0"):
        b = bc.solve(solver, [windows[key]], band_variant=GENERIC)[0]
    bc.same(solved[key], b, f"{key} static / generic")


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_persistent_equals_one_workgroup(solver, windows, solved, key):
    with bc.env("DVH_BAND_QUEUE", "0"):  # (the static instantiation exists in the persistent unit only)
        b = bc.solve(solver, [windows[key]], band_variant=GENERIC)[0]
    bc.same(solved[key], b, f"{key} persistent / one workgroup per window")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "band_limits_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("T", (3, 193, 577, 768))
def test_bits_of_the_parent_at_iteration_limits(solver, golden, T):
    """Every case of tests/band_limits.py: the digest, iterations and status the parent commit's library gave."""
    assert tuple(sorted(int(k) for k in golden)) == band_limits.STEPS
    lp, nb = band_limits.windows()[T]
    want = golden[str(T)]
    assert band_limits.lp_digest(lp) == want["lp"] and band_limits.lp_digest(nb) == want["neighbour"], f"T {T}: not the recorded windows"
    got = band_limits.digests(solver, {T: (lp, nb)})[str(T)]
    assert got["start_iters"] == want["start_iters"] and got["start"] == want["start"], \
        f"T {T}: the carried start differs ({got['start_iters']} vs {want['start_iters']} iterations)"
    assert set(got["cases"]) == set(want["cases"]) and len(want["cases"]) == 2 * len(band_limits.LIMITS)
    bad = [(c, got["cases"][c], want["cases"][c]) for c in want["cases"] if got["cases"][c] != want["cases"][c]]
    for c, g, w in bad:
        print(f"T {T} {c}: iterations {g['iters']} / {w['iters']}, status {g['status']} / {w['status']}, "
              f"digest equal: {g['sha256'] == w['sha256']}")
    assert not bad, f"T {T}: {len(bad)} of {len(want['cases'])} cases differ from the parent's bits: {[c for c, _, _ in bad]}"


def test_limit_cases_cover_both_sides_of_a_check(golden):
    """The recorded cases end before, at and behind a check, and the carried runs at (64, 129) pass two checks."""
    for T, rec in golden.items():
        it = {c: v["iters"] for c, v in rec["cases"].items()}
        for kind in ("cold", "carried"):
            assert [it[f"{kind} check_every 64 max_iters {m}"] for m in (1, 2, 63, 64, 65)] == [1, 2, 63, 64, 65], (T, kind)
            assert it[f"{kind} check_every 1 max_iters 3"] == 3 and it[f"{kind} check_every 2 max_iters 5"] == 5, (T, kind)
