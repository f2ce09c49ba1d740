"""Writes tests/golden/icp_fit_parent.npz: R, t, W and the det sign that lslam_debug_icp_fit returned on the exact sums of the
base, planar and slab cases of tests/icp_ref.py WHEN ITS svd3 WAS STILL THE ONE lslam_icp_align HAD BEFORE THE COMPLETION OF
RANK-DEFICIENT FACTORS (the entry point was added first, around the unedited function; then this was run; then svd3 was
changed).  tests/test_icp_ref.py holds the present library to these bits: full-rank and rank-2 inputs must not move.
Running it again records the present library, which is only meaningful as long as that test passes."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import icp_ref as I  # noqa: E402

FAMILIES = ("base", "planar", "planar_tilted", "slab")


def main():
    scan_match = importlib.import_module("the-cooper-mapper_amd.scan_match")
    out = {}
    for c in I.cases():
        if c["family"] not in FAMILIES or c["degenerate"]:
            continue
        st = I.ref_step(c["target"], c["source"], c["T"], c["gate"])
        if st["fit"] is None:
            continue
        f = scan_match.icp_fit(st["sums"])
        out[c["name"] + "/sums"] = st["sums"]
        out[c["name"] + "/fit"] = np.concatenate([f["R"].ravel(), f["t"], f["W"], [float(f["det_sign"])]])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "icp_fit_parent.npz"), **out)
    print(len(out) // 2, "cases recorded")


if __name__ == "__main__":
    main()
