#!/usr/bin/env python3
"""Records tests/golden/pg_solve_paths.json: what every configuration of tests/test_gpu_pg_solve_paths.py (its own CONFIGS
table, its own run_config) gives with the library that is loaded.  The fixture pins the pose-graph solver's host driver
against a KNOWN-GOOD library, so it is recorded from the build of the commit BEFORE a change to the driver, loaded through
LSLAM_LIB:

    LSLAM_LIB=/path/to/parent/liblslam_hip.so python tools/record_pg_solve_paths.py [-o tests/golden/pg_solve_paths.json]

and never from the tree under test.  Record twice (-o to two files) and compare the files before trusting the fixture: the
test compares every field exactly.  Needs the GPU the tests run on."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("LSLAM_DEBUG_HOOKS", "1")  # as tests/conftest.py: two configurations use the abort hooks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "pg_solve_paths.json"))
    args = ap.parse_args()
    if not os.environ.get("LSLAM_LIB"):
        sys.exit("LSLAM_LIB is not set: the fixture is recorded from the parent commit's library, never from the tree under test")
    pkg = importlib.import_module("the-cooper-mapper_amd")
    sys.modules.setdefault("cooper_mapper_amd", pkg)
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import test_gpu_pg_solve_paths as T
    out = {}
    for name in T.CONFIGS:
        r = out[name] = T.run_config(pkg, synth, name)
        its = [s["iterations"] for s in r["solves"]]
        tripped = next((k for k, n in enumerate(its) if n > 300), None)  # (automatic second level: on after such a solve)
        print(name, "rc", r["rc"], "solve iterations", its, "first solve over 300 iterations:", tripped,
              "LM", r["stats"]["iterations"], "trials", r["stats"]["lm_trials"], "cg", r["stats"]["cg_iterations"],
              "fused", r["stats"]["fused_solves"], "chi2", float.fromhex(r["stats"]["chi2_final"]),
              "row-sharded", r["row_sharded_solves"], "gathered", r["row_gathered_solves"], r.get("robust_info", ""), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("library:", pkg.lib_path(), "->", args.out)


if __name__ == "__main__":
    main()
