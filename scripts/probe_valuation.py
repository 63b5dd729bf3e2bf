"""Timing probe of the scenario valuation: bills, pro forma, NPV, payback and IRR of a solved config-4 sweep on the
device (dervet_hip/valuation.py value_sweep: dvh_bill_windows + dvh_value_scenarios, [S, 7] numbers copied back)
against the host path it replaces (the dispatch copied to the host, builder.evaluate_terms over the dense [G, n]
coefficient arrays, the valuation in numpy).

In one process, per size (scenarios; 12 monthly windows each): the sweep is built on the device and solved once
(SeededSweep, as bench.py does), then `--reps` repeats of each path on that solved batch:
  device: value_sweep and the copy of its values to the host (wall), and the two kernels' times from HIP events
          (dvh_last_valuation_ms) next to the solve's total_ms of the same step;
  host:   dev.x copied to the host, evaluate_terms of every window group (the groups' term arrays are built before the
          clock starts: the host path has them from building the LPs), the original charges of the base load, and
          valuation.value_scenarios_host.  None of it goes through the new device calls.
Prints the bill kernel's achieved bytes/s (what it must read once: ch, dis, base and retail of every window, 32 T
bytes, plus the 64 + 8 J bytes it writes) beside the copy rate the GPU reaches (~6.3 TB/s of the 8 TB/s HBM3E peak), and
the keep-criterion (profiles/INDEX.md): the device path's slowest repeat is faster than the host path's fastest.

Usage: python scripts/probe_valuation.py [--sizes 1000 10000] [--reps 5]
"""
import argparse
import functools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "der-vet_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from dervet_hip import BatchSolver, valuation as V  # noqa: E402
from dervet_hip.lp import builder, scenarios  # noqa: E402
from dervet_hip.sweep import SeededSweep  # noqa: E402

HBM_COPY_GBPS = 6300.0


def host_terms(sw):
    """Per packed window group: the retailETS and DCM terms (dense [G, n] coefficients, constants) and what the
    original charges need, from the host builder -- one window position at a time, so that only the terms stay."""
    out = []
    for ids in (sw.seed_ids, sw.rest_ids):
        for k in range(12):
            if not len(ids):
                continue
            g = scenarios.config4(ids, only=[k])[0]
            keep = builder.WindowGroup(T=g.T, J=g.J, m_eq=g.m_eq, indptr=None, indices=None, data=g.c[:, :0], c=g.c[:, :0],
                                       c0=None, q=None, l=None, u=None,
                                       terms={t: g.terms[t] for t in ("retailETS", "DCM")}, tags=g.tags)
            out.append((keep, g.inputs))
    return out


def host_path(dev, groups, ptr, idx, year, fin):
    x = dev.x.cpu().numpy()
    desc = dev.desc.cpu().numpy()
    rows, k = [], 0
    for g, inp in groups:
        G, n = g.G, int(desc[k, 0])
        off = int(desc[k, 6])
        t = builder.evaluate_terms(g, x[off:off + G * n].reshape(G, n))
        b = np.zeros((G, V.BILL_ROWS))
        b[:, V.RETAIL], b[:, V.DEMAND] = t["retailETS"], t["DCM"]
        base = inp["base"]
        b[:, V.ORIG_RETAIL] = (inp["retail"] * inp["dt"] * base).sum(axis=1)
        for j in range(g.J):
            b[:, V.ORIG_DEMAND] += inp["demand"][:, j] * base[:, inp["dcm_t"][inp["dcm_j"] == j]].max(axis=1)
        rows.append(b)
        k += G
    return V.value_scenarios_host(np.concatenate(rows), None, ptr, idx, year, fin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=32)
    a = ap.parse_args()
    ok = True
    with BatchSolver(0) as s:
        for S in a.sizes:
            ids = np.arange(S)
            P = scenarios.sweep_parameters(ids)
            sw = SeededSweep(functools.partial(scenarios.config4, spec=True), ids, P["E"], stride=a.stride,
                             features=scenarios.sweep_features(P))
            dev = sw.to_device(s, "cuda:0")
            tm, _ = sw.solve(s, dev)
            torch.cuda.synchronize()
            fin = V.Financials(years=20, opt_years=(0,), rate=0.06, growth=[2.2, 2.2, 0.0, 0.0, 0.0],
                               capex=400.0 * P["E"], fixed_om=1.25 * P["E"], extra=np.full((1, 21), 100.0))
            _, ptr, idx, year = V.sweep_map(sw.tags, fin)
            nbytes = sum(sp.G * (32 * sp.T + 64 + 8 * sp.J) for sp in sw.specs)
            optimal = int((dev.istats[:, 0] == 0).sum())
            print(f"== {S} scenarios, {dev.count} windows ({optimal} optimal), solve total_ms {tm['total_ms']:.2f} "
                  f"(one run), x {dev.x.numel() * 8 / 1e6:.1f} MB", flush=True)

            def device_once():
                torch.cuda.synchronize()
                t = time.perf_counter()
                val = V.value_sweep(sw, s, dev, fin)
                out = val.numpy()
                wall = time.perf_counter() - t
                return wall, V.last_ms(s), out

            device_once()  # warm-up: code objects, the allocator's blocks
            dr = [device_once() for _ in range(a.reps)]
            dwall = [r[0] * 1e3 for r in dr]
            bill = [r[1]["bill_ms"] for r in dr]      # (the last group's launch: see below)
            print(f"device path wall ms per repeat: {' '.join(f'{w:.2f}' for w in dwall)}")
            # the bill runs one launch per window group (24 here); dvh_last_valuation_ms times the last, so the whole
            # bill is timed with events around the call instead
            evs = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                b = V.bill_windows(s, dev, sw.specs)
                e1.record()
                torch.cuda.synchronize()
                evs.append(e0.elapsed_time(e1))
                del b
            val_ms = [r[1]["valuation_ms"] for r in dr]
            print(f"bill kernels (all {len(sw.specs)} groups, HIP events) ms: {' '.join(f'{v:.3f}' for v in evs)}; last "
                  f"group's launch alone: {' '.join(f'{v:.3f}' for v in bill)}")
            print(f"valuation kernel (HIP events) ms: {' '.join(f'{v:.3f}' for v in val_ms)}")
            print(f"bill + valuation kernels per 12-window-per-scenario step: {min(evs) + min(val_ms):.3f} .. "
                  f"{max(evs) + max(val_ms):.3f} ms, next to the solve's total_ms {tm['total_ms']:.2f}")
            gbps = [nbytes / (v * 1e-3) / 1e9 for v in evs]
            print(f"bill kernel: {nbytes / 1e6:.1f} MB read + written once -> {min(gbps):.0f} .. {max(gbps):.0f} GB/s "
                  f"achieved, {100 * max(gbps) / HBM_COPY_GBPS:.1f} % of the ~{HBM_COPY_GBPS:.0f} GB/s a copy reaches")

            groups = host_terms(sw)
            host_path(dev, groups, ptr, idx, year, fin)  # warm-up
            hwall, hv = [], None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                hv = host_path(dev, groups, ptr, idx, year, fin)
                hwall.append((time.perf_counter() - t) * 1e3)
            print(f"host path wall ms per repeat: {' '.join(f'{w:.1f}' for w in hwall)}")
            # the two paths value the same dispatch: the device bills its own peaks, the host path the LP's tau
            got = dr[-1][2]
            rel = np.nanmax(np.abs(got.pv_benefit - hv.pv_benefit) / np.abs(hv.pv_benefit))
            rel_n = np.nanmax(np.abs(got.npv - hv.npv) / np.abs(hv.pv_cost))
            print(f"device against host path (the LP's tau against the dispatch's own peak, both within solver "
                  f"tolerance): present-value benefit max rel diff {rel:.2e}, lifetime present value max diff "
                  f"{rel_n:.2e} of the present-value cost; valid {int(got.valid.sum())} / {S}")
            keep = max(dwall) < min(hwall)
            ok &= keep
            print(f"criterion (device slowest {max(dwall):.2f} ms < host fastest {min(hwall):.1f} ms): "
                  f"{'met' if keep else 'NOT met'}; ratio of medians {np.median(hwall) / np.median(dwall):.1f}x", flush=True)
            del dev, groups
            torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
