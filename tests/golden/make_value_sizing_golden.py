"""Write tests/golden/uc1_sizing.{json,npz}: the reference's Usecase 1 economic-sizing goldens (run where the
reference's tree is available; reads CSV data files only, never reference code).

Sources (relative to the reference tree, test/test_validation_report_sept1):
  * Results/Usecase1/<case>/sizeuc3.csv, objective_valuesuc3.csv          (golden sizes, the objective row)
  * Model_params/Usecase1/Model_Parameters_Template_Usecase1_UnPlanned_<CASE>.csv  (active parameters)
  * the time series CSV the parameters name (site load, PV profile), datasets/tariff_refernce_case_1.csv (tariff)
Cases: es (ene / ch / dis ratings 0: sized), es+pv (a fixed PV beside the sized ESS).

Usage:  python tests/golden/make_value_sizing_golden.py <reference tree>
"""
import csv
import json
import os
import sys

import numpy as np

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
VR = os.path.join(REF, "test", "test_validation_report_sept1")
CASES = {"es": "ES", "es+pv": "ES+PV"}


def read_cols(path):
    with open(path, encoding="utf-8-sig") as f:
        rows = list(csv.reader(f))
    head = [h.strip() for h in rows[0]]
    return {h: [r[i] if i < len(r) else "" for r in rows[1:]] for i, h in enumerate(head)}


def fcol(cols, name):
    return np.array([float(v) if v.strip() != "" else np.nan for v in cols[name]], dtype=np.float64)


def read_params(path):
    """Active model parameters (Tag, Key) -> Optimization Value."""
    with open(path, encoding="utf-8-sig") as f:
        rows = list(csv.DictReader(f))
    active = {r["Tag"].strip() for r in rows if r.get("Active", "").strip().lower() in ("yes", "y", "1")}
    out = {}
    for r in rows:
        if r["Tag"].strip() in active and r["Key"] is not None:
            out.setdefault(r["Tag"].strip(), {})[r["Key"].strip()] = (r["Optimization Value"] or "").strip()
    return out


def read_tariff(path):
    c = read_cols(path)
    num = lambda v: float(v) if v.strip() != "" else None  # noqa: E731
    ints = lambda k: [int(float(v)) for v in c[k]]  # noqa: E731
    return {"billing_period": ints("Billing Period"), "start_month": ints("Start Month"), "end_month": ints("End Month"),
            "start_time": ints("Start Time"), "end_time": ints("End Time"),
            "excl_start": [num(v) for v in c["Excluding Start Time"]], "excl_end": [num(v) for v in c["Excluding End Time"]],
            "weekday": ints("Weekday?"), "value": [float(v) for v in c["Value"]],
            "charge": [v.strip().lower() for v in c["Charge"]]}


def ref_path(p):
    """A path of the parameter files (written on a case-insensitive file system) inside the reference tree."""
    cur = REF
    for part in p.replace("\\", "/").lstrip("./").split("/"):
        names = {n.lower(): n for n in os.listdir(cur)}
        cur = os.path.join(cur, names.get(part.lower(), part))
    return cur


def main():
    meta, arrays = {}, {}
    for name, tag in CASES.items():
        res = os.path.join(VR, "Results", "Usecase1", name)
        params = read_params(os.path.join(VR, "Model_params", "Usecase1",
                                          f"Model_Parameters_Template_Usecase1_UnPlanned_{tag}.csv"))
        size = read_cols(os.path.join(res, "sizeuc3.csv"))
        obj = read_cols(os.path.join(res, "objective_valuesuc3.csv"))
        ts = read_cols(ref_path(params["Scenario"]["time_series_filename"]))
        rows = {d.strip(): i for i, d in enumerate(size["DER"])}
        es = rows["es"]
        arrays[f"{name}__site_load"] = fcol(ts, "Site Load (kW)")
        arrays[f"{name}__pv_profile"] = fcol(ts, "PV Gen (kW/rated kW)")
        meta[name] = {
            "source_results": f"test/test_validation_report_sept1/Results/Usecase1/{name}",
            "params": {t: params[t] for t in ("Scenario", "Finance", "Battery", "PV", "DCM", "retailTimeShift") if t in params},
            "active_tags": sorted(params.keys()),
            "tariff": read_tariff(ref_path(params["Finance"]["customer_tariff_filename"])),
            "golden_size": {k: float(size[k][es]) for k in ("Energy Rating (kWh)", "Charge Rating (kW)", "Discharge Rating (kW)",
                                                            "Capital Cost ($)", "Capital Cost ($/kW)", "Capital Cost ($/kWh)")},
            "golden_objective": {k: float(v[0]) for k, v in obj.items() if k != ""},
        }
        for p in ("time_series_filename", "monthly_data_filename"):   # (paths of the reference tree: not needed)
            meta[name]["params"]["Scenario"].pop(p, None)
        print(name, meta[name]["golden_size"], meta[name]["golden_objective"], len(arrays[f"{name}__site_load"]))
    np.savez_compressed(os.path.join(HERE, "uc1_sizing.npz"), **arrays)
    with open(os.path.join(HERE, "uc1_sizing.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
