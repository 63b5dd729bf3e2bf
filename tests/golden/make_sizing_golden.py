"""Write tests/golden/reliability_sizing.json: the reference's golden reliability sizes of its load-shedding
sizing runs (run where the reference's tree is available; reads CSV data files only, never reference code).

Sources (relative to the reference tree):
  * test/test_load_shedding/results/Sizing/{w_ls1,wo_ls1}/size_2mw_5hr.csv             (golden ratings, unit costs)
  * test/test_load_shedding/mp/Sizing/Model_Parameters_Template_DER_{w,wo}_ls1.csv     (Reliability target)
The critical-load series (and the load-shed percentages) are those of the post-facto runs already committed in
reliability_cases.npz under the names recorded here.

Usage:  python tests/golden/make_sizing_golden.py <reference tree>
"""
import csv
import json
import os
import sys

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
LS = os.path.join(REF, "test", "test_load_shedding")

CASES = {"w_ls1": "ls_w_ls1", "wo_ls1": "ls_wo_ls1"}


def size_row(path):
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if row["DER"].strip().lower() == "es":
                return row
    raise SystemExit(f"no ES row in {path}")


def param(path, tag, key):
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if row["Tag"] == tag and row["Key"] == key:
                return row["Optimization Value"]
    raise SystemExit(f"{tag}/{key} not in {path}")


def main():
    out = {"source": "test/test_load_shedding/results/Sizing/<case>/size_2mw_5hr.csv", "cases": {}}
    for name, series in CASES.items():
        r = size_row(os.path.join(LS, "results", "Sizing", name, "size_2mw_5hr.csv"))
        mp = os.path.join(LS, "mp", "Sizing", f"Model_Parameters_Template_DER_{name}.csv")
        out["cases"][name] = {
            "series": series,
            "Energy Rating (kWh)": float(r["Energy Rating (kWh)"]),
            "Discharge Rating (kW)": float(r["Discharge Rating (kW)"]),
            "Charge Rating (kW)": float(r["Charge Rating (kW)"]),
            "target_hours": float(param(mp, "Reliability", "target")),
            "ccost": float(r["Capital Cost ($)"]),
            "ccost_kw": float(r["Capital Cost ($/kW)"]),
            "ccost_kwh": float(r["Capital Cost ($/kWh)"]),
            "rte": float(r["Round Trip Efficiency (%)"]),
            "llsoc": float(r["Lower Limit on SOC (%)"]),
            "ulsoc": float(r["Upper Limit on SOC (%)"]),
        }
    with open(os.path.join(HERE, "reliability_sizing.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
