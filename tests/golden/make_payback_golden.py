"""Extract the payback and cost-benefit results of the Usecase 2 monthly cases (es; es + PV + DG) from the reference's
own test data into tests/golden/uc2_payback.json (run in the build container only).

Reads two CSV *result* files per case under test/test_validation_report_sept1/Results/Usecase2/<case>/step2 --
payback<suffix>.csv and cost_benefit<suffix>.csv -- and records their numbers; it never imports or executes reference
code.  The file's "Cost-Benefit Ratio" column is cost / benefit (an older reference version; dervet/CBA.py:510-523
computes benefit / cost): it is recorded under the file's own name.

Usage:  python tests/golden/make_payback_golden.py <reference root>
"""
import csv
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"es": ("Results/Usecase2/es/step2", "uc3_es_step2"),
         "es+pv+dg": ("Results/Usecase2/es+pv+dg/step2", "uc3_es+pv+dg_step2")}


def num(v):
    v = (v or "").strip()
    return None if v == "" else float(v)


def main(ref):
    vr = os.path.join(ref, "test", "test_validation_report_sept1")
    out = {}
    for name, (resdir, suf) in CASES.items():
        with open(os.path.join(vr, resdir, f"payback{suf}.csv"), encoding="utf-8-sig") as f:
            rows = list(csv.DictReader(f))
        pay = {}
        for r in rows:  # one row per unit; a metric sits in the row of its unit, blank elsewhere (blank everywhere: None)
            for k, v in r.items():
                if k != "Unit" and num(v) is not None:
                    pay[k] = num(v)
        for k in rows[0]:
            if k != "Unit":
                pay.setdefault(k, None)
        with open(os.path.join(vr, resdir, f"cost_benefit{suf}.csv"), encoding="utf-8-sig") as f:
            cb = list(csv.reader(f))
        out[name] = {"source_results": os.path.join("test/test_validation_report_sept1", resdir), "payback": pay,
                     "cost_benefit": {r[0]: {"cost": float(r[1]), "benefit": float(r[2])} for r in cb[1:] if r and r[0]}}
    with open(os.path.join(HERE, "uc2_payback.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote uc2_payback.json", sorted(out))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
