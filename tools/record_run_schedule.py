#!/usr/bin/env python3
"""Records tests/golden/run_schedule.json: what every configuration of tests/test_gpu_run_schedule.py (its own CONFIGS table,
its own run_config) does with the library that is loaded.  The fixture pins the driver's launch schedule against a KNOWN-GOOD
library, so it is recorded from the build of the commit BEFORE a change to the driver, loaded through LSLAM_LIB:

    LSLAM_LIB=/path/to/parent/liblslam_hip.so python tools/record_run_schedule.py [-o tests/golden/run_schedule.json]

and never from the tree under test.  Needs the GPU the tests run on."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "golden", "run_schedule.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    sys.modules.setdefault("cooper_mapper_amd", pkg)
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import test_gpu_run_schedule as T
    pr = synth.make_problem(rings=16, azimuth_steps=900, world_half=60.0)  # conftest.py's small_problem
    out = {}
    for name in T.CONFIGS:
        out[name] = T.run_config(pkg, synth, pr, name)
        print(name, [(r["status"], r["stats"][0]["iterations"], r["stats"][0]["sweep_launches"],
                      {k: v for k, v in r["sweep_launches"].items() if v}, r["grid_launches"]) for r in out[name]], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("library:", pkg.lib_path(), "->", args.out)


if __name__ == "__main__":
    main()
