"""The three-step band form's plain iteration with its LDS reads issued first behind each barrier and the Halpern blends
and late rows run under their latency.  Only the order of independent work changes: every value is produced by the same
operations in the same order, so the new library must return the parent commit's bits.

Windows: those of tests/test_gpu_band_wave0.py (non-zero soc_target and llsoc, forced "band3") at
T = 2, 3, 4, 192, 193, 576, 577, 766, 767, 768 with J = 1, and T = 193 with J = 2 and J = 4, which take the generic
instantiation's other loop body (the per-column tau path on wave 0).

Bars:
  host restatement   iterations within 128 of oracle/pdlp_ref.py, objective within 1e-7 relative, and the result contract
                     recomputed from the returned x, y (tests/result_contract.py; reference optimum: HiGHS);
  unchanged kernel   objective within 1e-9 relative of the one-step form ("band1", whose machine code does not change);
  between variants   bit for bit: the static single-demand-period instantiation against the forced generic one
                     (DVH_BAND_J1=0), the persistent grid against the one-workgroup launch (DVH_BAND_QUEUE=0);
  against the parent bit for bit: the SHA-256 of x || y, the iterations and the status at iteration limits around the check
                     period, cold and from a carried start, as scripts/dump_band_limits.py recorded them with the parent
                     commit's library in tests/golden/band_limits_parent.json -- work that is pending at a loop exit
                     (in front of a check, at max_iters) is what the other bars could miss;
  restarts           for every T the reference restarts inside one of the runs compared here (asserted on the reference).
"""
import contextlib
import importlib.util
import json
import os

import pytest

import result_contract as rc
import test_gpu_band_wave0 as w0
from dervet_hip import BatchSolver
from oracle import pdlp_ref, window_lp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, STATIC, ONE_STEP = w0.GENERIC, w0.STATIC, 9000012  # kernel_stats()["band_variant"] / ["variant"]
ITER_TOL = 128
OBJ_TOL = 1e-7
FORM_TOL = 1e-9
# (T, J): seed.  J = 1: the windows of test_gpu_band_wave0; J = 2, 4 on its T = 193 window's seed
CASES = {(T, 1): seed for T, seed in w0.SEEDS.items()}
CASES[(193, 2)] = w0.SEEDS[193]
CASES[(193, 4)] = w0.SEEDS[193]
KEYS = tuple(CASES)
IDS = [f"T{T}-J{J}" for T, J in KEYS]


def _dump_module():
    spec = importlib.util.spec_from_file_location("dump_band_limits", os.path.join(ROOT, "scripts", "dump_band_limits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def solver():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no GPU is visible (run with -m 'not gpu' on CPU hosts)")
    with BatchSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def windows():
    return {(T, J): w0._window(T, J, CASES[(T, J)])[0] for T, J in KEYS}


def _restarts(trace):
    """Restarts in a pdlp_ref trace: checks at which the iterations since the last restart fell back."""
    ks = [t[1] for t in trace]
    return sum(1 for u, v in zip(ks, ks[1:]) if v <= u)


@pytest.fixture(scope="module")
def refs(windows):
    """pdlp_ref at check period 64 with its trace, and the HiGHS optimum of every window, computed once."""
    out = {}
    for key, lp in windows.items():
        olp = w0._oracle_lp(lp)
        h = window_lp.solve_highs(olp)
        assert h["status"] == 0, key
        trace = []
        ref = pdlp_ref.solve(olp, dict(check_every=64, kkt_every=1), trace=trace)
        out[key] = (olp, ref, h["obj"], _restarts(trace))
    return out


@contextlib.contextmanager
def _env(name, value):
    """An A/B switch the library reads at every launch, for the solves inside."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _variant(J):
    return STATIC if J == 1 else GENERIC


def _solve(s, lp, band_variant, path="band3", **options):
    opts = dict(check_every=64, kkt_every=1, kkt_predict=0, max_iters=100000, warm_start=0)
    opts.update(options)
    s.set_options(**opts)
    s.set_kernel_path(path)
    r = s.solve([lp])[0]
    st = s.kernel_stats()
    if path == "band3":
        assert st["band_windows"] == 1 and st["variant"] == GENERIC and st["band_variant"] == band_variant, st
    else:
        assert st["band_windows"] == 1 and st["variant"] == ONE_STEP, st
    return r


@pytest.fixture(scope="module")
def solved(solver, windows):
    """Every window by the default launch of the three-step form, once."""
    return {key: _solve(solver, lp, _variant(key[1])) for key, lp in windows.items()}


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_against_the_host_restatement(solved, refs, key):
    olp, ref, opt, restarts = refs[key]
    r = solved[key]
    print(f"{key}: reference {ref['iters']} iterations, {restarts} restarts")
    assert restarts >= 1, f"{key}: the reference does not restart inside the run"
    assert ref["y"][0] != 0.0, f"{key}: the reference's init-row dual is zero"
    w0._agrees(r, ref, 64, f"{key}")
    rc.check_both(olp, r, opt, f"T {key[0]} J {key[1]}", "band3_J1" if key[1] == 1 else "band3")


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_against_the_one_step_form(solver, windows, solved, key):
    """The one-step form's machine code does not change; the two forms group the tau partial sums differently."""
    a = solved[key]
    b = _solve(solver, windows[key], None, path="band1")
    print(f"{key}: three-step {a.iters} iterations obj {a.obj!r}; one-step {b.iters} iterations obj {b.obj!r}")
    assert a.status == b.status == 0, (a.status_name, b.status_name)
    assert abs(a.obj - b.obj) <= FORM_TOL * abs(b.obj), f"{key}: obj {a.obj!r} vs the one-step form's {b.obj!r}"


@pytest.mark.parametrize("key", [k for k in KEYS if k[1] == 1], ids=[i for i, k in zip(IDS, KEYS) if k[1] == 1])
def test_static_equals_generic(solver, windows, solved, key):
    with _env("DVH_BAND_J1", "0"):
        b = _solve(solver, windows[key], GENERIC)
    w0._same(solved[key], b, f"{key} static / generic")


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_persistent_equals_one_workgroup(solver, windows, solved, key):
    with _env("DVH_BAND_QUEUE", "0"):  # (the static instantiation exists in the persistent unit only)
        b = _solve(solver, windows[key], GENERIC)
    w0._same(solved[key], b, f"{key} persistent / one workgroup per window")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "band_limits_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dump():
    return _dump_module()


@pytest.mark.parametrize("T", (3, 193, 577, 768))
def test_bits_of_the_parent_at_iteration_limits(solver, golden, dump, T):
    """Every case of scripts/dump_band_limits.py: the digest, iterations and status the parent commit's library gave."""
    assert tuple(sorted(int(k) for k in golden)) == dump.STEPS
    lp, nb = w0._window(T, 1, w0.SEEDS[T])[0], w0._window(T, 1, w0.SEEDS[T], load_scale=1.03)[0]
    want = golden[str(T)]
    assert dump.lp_digest(lp) == want["lp"] and dump.lp_digest(nb) == want["neighbour"], f"T {T}: not the recorded windows"
    got = dump.digests(solver, {T: (lp, nb)})[str(T)]
    assert got["start_iters"] == want["start_iters"] and got["start"] == want["start"], \
        f"T {T}: the carried start differs ({got['start_iters']} vs {want['start_iters']} iterations)"
    assert set(got["cases"]) == set(want["cases"]) and len(want["cases"]) == 2 * len(dump.LIMITS)
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
