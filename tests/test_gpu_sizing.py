"""Reliability sizing on the GPU (dervet_hip.reliability.size_for_reliability: dvh_outage_first_uncovered,
dvh_sizing_windows, dvh_size_reliability) vs the oracle's outage simulation, HiGHS, the host LP builder, the
reference's golden sizes and the CPU restatement of the loop (tests/sizing_ref.py)."""
from dataclasses import replace

import numpy as np
import pytest

import sizing_ref
from dervet_hip import reliability
from dervet_hip.lp import sizing

pytestmark = pytest.mark.gpu


def _random_case(rng, N, dt=1.0, max_out=24, pv=True, dg=True, shed=True):
    """As test_gpu_outage._random_case, every outage starting from soc_init x E."""
    cl = rng.uniform(200.0, 1500.0, N).round(5)
    E = float(rng.uniform(500, 6000))
    ess = dict(E=E, P_ch=E / rng.uniform(2, 6), P_dis=E / rng.uniform(2, 6), rte=float(rng.uniform(0.8, 0.95)),
               llsoc=float(rng.uniform(0, 0.2)), ulsoc=float(rng.uniform(0.85, 1.0)))
    pvs = [np.maximum(0.0, rng.normal(600, 400, N))] if pv else []
    return reliability.OutageCase(
        critical_load=cl, dt=dt, max_outage_duration=max_out, ess=ess, init_soe=None,
        soc_init=float(rng.uniform(0.3, 1.0)), pv_max=pvs, pv_nu=[float(rng.uniform(0.2, 1.0))] if pv else [],
        pv_gamma=[float(rng.uniform(0.3, 1.0))] if pv else [], dg_power=[float(rng.uniform(0, 600))] if dg else [],
        load_shed_pct=rng.choice([100.0, 80.0, 50.0, 30.0], size=max_out) if shed else None)


def test_scan_first_uncovered_bit_exact(gpu_solver):
    """first / n_uncovered of every case equal the oracle's: PV, generators, shedding, llsoc / ulsoc, a series
    shorter than the data window (N = 13), dt = 0.5, more than one workgroup per case (N = 700), a generously sized
    ESS (nothing uncovered) and a tiny one (the first start uncovered)."""
    rng = np.random.default_rng(20250611)
    cases = [_random_case(rng, 700), _random_case(rng, 700, pv=False), _random_case(rng, 700, dg=False, shed=False),
             _random_case(rng, 700, pv=False, dg=False), _random_case(rng, 13, max_out=40),
             _random_case(rng, 300, dt=0.5, max_out=12)]
    cases[2] = replace(cases[2], ess=dict(cases[2].ess, E=1e6, P_ch=1e5, P_dis=1e5), soc_init=1.0)
    cases[3] = replace(cases[3], ess=dict(cases[3].ess, E=1.0))
    e = cases[5].ess  # (halved: as drawn it covers every start)
    cases[5] = replace(cases[5], ess=dict(e, E=0.5 * e["E"], P_ch=0.5 * e["P_ch"], P_dis=0.5 * e["P_dis"]))
    steps = [4, 6, 5, 3, 4, 5]
    hours = [L * c.dt for L, c in zip(steps, cases)]
    first, count = reliability.first_uncovered(cases, hours, gpu_solver)
    for k, (c, L) in enumerate(zip(cases, steps)):
        f, n = sizing_ref.scan_case(c, L)
        print(f"case {k}: first {first[k]} (oracle {f}), uncovered {count[k]} (oracle {n})")
        assert (int(first[k]), int(count[k])) == (f, n), f"case {k}"
    assert first[2] == -1 and count[2] == 0
    assert first[3] == 0 and count[3] > 256
    assert first[5] > 0 and count[5] > 0, "the half-hour case must have a covered first start and uncovered later ones"


def test_sizing_lp_built_on_the_device_is_the_host_lp(gpu_solver):
    """dvh_sizing_windows builds the LPs on the device from the resident series; solving them must take the same
    iterations and return bit-equal x as solving lp.sizing.sizing_lp's arrays (deterministic kernels: only
    bit-identical LPs do), the sizes within 1e-6 relative of HiGHS."""
    fam = sizing_ref.random_family(5, 4)  # no PV / PV, generator, shedding + dt 0.5, llsoc > 0
    fam[0] = (replace(fam[0][0], soc_init=1.0), fam[0][1])   # soc_init > ulsoc
    fam[1] = (replace(fam[1][0], soc_init=0.7), fam[1][1])   # soc_init < ulsoc
    cases, specs = [c for c, _ in fam], [s for _, s in fam]
    assert cases[0].soc_init > cases[0].ess["ulsoc"] and cases[1].soc_init < cases[1].ess["ulsoc"]
    assert any(c.pv_max for c in cases) and any(not c.pv_max for c in cases)
    assert any(c.load_shed_pct is not None and c.dt == 0.5 for c in cases) and all(c.ess["llsoc"] > 0 for c in cases)
    starts = []
    for c, s in fam:
        N = len(c.critical_load)
        st = [int(v) for v in sizing.seed_starts(c, s)] + [N - 2, 17, N // 2]  # N - 2: runs past the series end
        starts.append(st)
        assert len(st) <= 13 and sizing.outage_steps(c, s) <= 6
    lps = [sizing.sizing_lp(c, s, st) for (c, s), st in zip(fam, starts)]
    host = gpu_solver.solve(lps)
    dev = reliability.sizing_windows(cases, specs, starts, gpu_solver)
    for k, (lp, a, b) in enumerate(zip(lps, host, dev)):
        x, st = sizing_ref.solve_highs(lp)
        print(f"case {k}: iters host {a.iters} device {b.iters} status {b.status_name} E {b.x[0]!r} P {b.x[1]!r} "
              f"HiGHS {x[0]!r} {x[1]!r}")
        assert st == 0 and a.status == 0 and b.status == 0, k
        assert a.iters == b.iters, k
        np.testing.assert_array_equal(a.x, b.x, err_msg=f"case {k}")
        np.testing.assert_array_equal(a.y, b.y, err_msg=f"case {k}")
        assert abs(b.x[0] - x[0]) <= 1e-6 * abs(x[0]) and abs(b.x[1] - x[1]) <= 1e-6 * abs(x[1]), k
        assert b.obj == a.obj


def test_golden_sizes(gpu_solver):
    """The reference's golden sizes of its load-shedding sizing runs, both cases in one call."""
    g = sizing_ref.golden_cases()
    names = sorted(g)
    cases, specs = [g[n][0] for n in names], [g[n][1] for n in names]
    res = reliability.size_for_reliability(cases, specs, gpu_solver, with_min_soe=True)
    print(reliability.last_sizing_ms(gpu_solver), [(r.rounds, r.lp_iters) for r in res])
    for n, c, r in zip(names, cases, res):
        ref = sizing_ref.golden_reference(n)
        print(n, r.energy, r.power, r.status, r.rounds, list(r.starts))
        assert (r.energy, r.power) == (g[n][2]["Energy Rating (kWh)"], g[n][2]["Discharge Rating (kW)"]), n
        assert r.status == "SIZED" and r.rounds == 4, n
        assert list(r.starts) == ref.starts, n
        assert r.capex == 100.0 * r.power + 800.0 * r.energy
        want = reliability.min_soe([reliability.sized_case(c, r)], [4], gpu_solver)[0]
        np.testing.assert_array_equal(r.min_soe, want)
        assert r.min_soe.max() > 0


@pytest.mark.parametrize("seed", sizing_ref.FAMILY_SEEDS)
def test_random_family_matches_the_cpu_loop(gpu_solver, seed):
    """Sizes, rounds and starts equal the CPU loop's (HiGHS + the oracle's simulation) integer for integer.  A case
    is left out only when HiGHS's optimum of a sized quantity lay within 1e-3 above an integer in some round (the two
    loops could then round apart); at most one per seed."""
    fam = sizing_ref.random_family(seed)
    refs = sizing_ref.family_reference(seed)
    res = reliability.size_for_reliability([c for c, _ in fam], [s for _, s in fam], gpu_solver)
    print(reliability.last_sizing_ms(gpu_solver))
    left_out = 0
    for k, ((c, s), ref, r) in enumerate(zip(fam, refs, res)):
        print(f"case {k}: GPU {r.energy} {r.power} {r.status} rounds {r.rounds} iters {r.lp_iters} | "
              f"CPU {ref.energy} {ref.power} {ref.status} rounds {ref.rounds}")
        if sizing_ref.near_integer(ref, s):
            left_out += 1
            continue
        assert (r.energy, r.power, r.status, r.rounds) == (ref.energy, ref.power, ref.status, ref.rounds), k
        assert list(r.starts) == ref.starts, k
    assert left_out <= 1


def test_round_limit_keeps_the_last_candidate(gpu_solver):
    case, spec, _ = sizing_ref.golden_cases()["wo_ls1"]
    r = reliability.size_for_reliability([case], [replace(spec, max_rounds=1)], gpu_solver)[0]
    ref = sizing_ref.golden_reference("wo_ls1", 1)
    assert (ref.energy, ref.power, ref.status) == (10744.0, 2711.0, "ROUND_LIMIT")
    assert (r.energy, r.power, r.status, r.rounds) == (10744.0, 2711.0, "ROUND_LIMIT", 1)
    assert list(r.starts) == ref.starts and len(r.starts) == 10


def test_finished_cases_drop_out_of_the_batch(gpu_solver):
    """Two cases that finish in different rounds: each gets the result it gets alone."""
    fam = sizing_ref.random_family(sizing_ref.FAMILY_SEEDS[0])
    refs = sizing_ref.family_reference(sizing_ref.FAMILY_SEEDS[0])
    a = max(range(len(fam)), key=lambda k: refs[k].rounds)
    b = min(range(len(fam)), key=lambda k: refs[k].rounds)
    assert refs[a].rounds > refs[b].rounds
    pair = [fam[a], fam[b]]
    both = reliability.size_for_reliability([c for c, _ in pair], [s for _, s in pair], gpu_solver)
    assert both[0].rounds != both[1].rounds
    for (c, s), r in zip(pair, both):
        alone = reliability.size_for_reliability([c], [s], gpu_solver)[0]
        assert (r.energy, r.power, r.status, r.rounds, r.lp_iters) == \
            (alone.energy, alone.power, alone.status, alone.rounds, alone.lp_iters)
        assert list(r.starts) == list(alone.starts)


def test_bad_spec_and_bad_starts_are_refused(gpu_solver):
    case, spec, _ = sizing_ref.golden_cases()["wo_ls1"]
    with pytest.raises(ValueError, match="ccost_kwh"):
        reliability.size_for_reliability([case], [replace(spec, ccost_kwh=0.0)], gpu_solver)
    with pytest.raises(Exception, match="outside the series"):
        reliability.sizing_windows([case], [spec], [[0, len(case.critical_load)]], gpu_solver)
    # the loop tightens eps for its own solves only: the same LP takes the same iterations before and after
    lp = sizing.sizing_lp(case, spec, sizing.seed_starts(case, spec))
    before = gpu_solver.solve([lp])[0]
    reliability.size_for_reliability([case], [replace(spec, max_rounds=1)], gpu_solver)
    after = gpu_solver.solve([lp])[0]
    assert before.status == 0 and (before.iters, before.obj) == (after.iters, after.obj)
