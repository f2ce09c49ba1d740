#!/usr/bin/env python3
"""The survey-cloud feature map extractor (lslam_survey_extract, csrc/lslam_survey.hip) on a generated survey of a few million
points: the whole extraction through the C ABI, its stages one by one through the stage taps on the same block (each tap's time
includes its own upload and download), and the numpy restatement (tests/survey_map_ref.py) on a stated subset as the CPU figure
beside it.  Host wall clock around calls that wait for their result (PCIe-inclusive); medians of --repeats
runs after one untimed run.  Writes the table to --out (kept as profiles/rNN_survey_map.txt).

The survey: a floor of --extent x --extent metres and two walls 5 m high at --spacing, in-plane jitter a fifth of the spacing,
Gaussian noise 0.5 mm, seeded; everything inside one 50 m partition cell, so the whole cloud is ONE block -- the largest the
reference's defaults can make, and the case where the label sweeps have the farthest to carry a label."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_survey(extent, spacing, seed):
    rng = np.random.default_rng(seed)

    def sheet(nu, nv):
        g = np.stack(np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"), -1).reshape(-1, 2) * spacing
        return g + rng.uniform(-0.2 * spacing, 0.2 * spacing, g.shape), rng.normal(0.0, 0.0005, len(g))
    n, h = int(extent / spacing), int(5.0 / spacing)
    a, na = sheet(n, n)
    floor = np.stack([2.0 + a[:, 0], 3.0 + a[:, 1], 0.5 + na], 1)
    b, nb = sheet(n, h)
    wall1 = np.stack([2.0 + nb, 3.0 + b[:, 0], 0.5 + b[:, 1]], 1)
    c, nc = sheet(n, h)
    wall2 = np.stack([2.0 + c[:, 0], 3.0 + nc, 0.5 + c[:, 1]], 1)
    return np.concatenate([floor, wall1, wall2], 0).astype(np.float32)


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, (max(ts) - min(ts)) * 1e3, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--extent", type=float, default=40.0)
    ap.add_argument("--spacing", type=float, default=0.03)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-crop", type=float, default=2.0, help="side [m] of the floor/wall corner the restatement is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_survey_map.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    import survey_map_ref as R
    sm = pkg.survey_map
    cloud = make_survey(a.extent, a.spacing, a.seed)
    ctx = pkg.Context(0)
    lines = ["survey: %d points (floor %g x %g m, two walls 5 m high, spacing %g m, seed %d), one partition block"
             % (len(cloud), a.extent, a.extent, a.spacing, a.seed),
             "host wall clock, median of %d runs after one untimed run (spread = max - min); every call waits for its result" % a.repeats, ""]

    def whole():
        m = sm.extract(ctx, cloud)
        st = m.info()
        m.close()
        return st
    ms, spread, st = timed(whole, a.repeats)
    lines.append("%-44s %10.1f ms  (spread %.1f)" % ("lslam_survey_extract, reference defaults", ms, spread))
    lines.append("  stats: " + ", ".join("%s %d" % kv for kv in st.items()))
    assert st["blocks_kept"] == 1 and st["n_surf"] > 0 and st["n_corner"] > 0
    # the stages through their taps, on the same block
    P = R.DEFAULTS
    xyzw = np.zeros((len(cloud), 4), np.float32)
    xyzw[:, :3] = cloud
    ms, spread, filt = timed(lambda: sm.voxel_grid_min(ctx, xyzw, P["filter_leaf"], P["filter_min_points"]), a.repeats)
    lines.append("%-44s %10.1f ms  (spread %.1f)  %d -> %d points" % ("filter (lslam_voxel_grid_min 0.05 / 3)", ms, spread, len(cloud), len(filt)))
    ms, spread, (nrm, cnt) = timed(lambda: sm.debug_normals(ctx, cloud, filt, P["normal_radius"]), a.repeats)
    ok = ~np.isnan(nrm[:, 0])
    lines.append("%-44s %10.1f ms  (spread %.1f)  neighbours %d .. %d, undefined %d" % ("normals (radius 0.05 over the block)", ms, spread, cnt.min(), cnt.max(), int((~ok).sum())))
    pts, nrm = filt[ok], nrm[ok]
    ms, spread, lists = timed(lambda: sm.debug_knn(ctx, pts, P["knn_k"], 4 * P["filter_leaf"]), a.repeats)
    lines.append("%-44s %10.1f ms  (spread %.1f)  %d lists of %d" % ("K-nearest lists (K = 60)", ms, spread, len(pts), P["knn_k"]))
    cth = R.cos_threshold(P["smoothness_angle"])
    ms, spread, (labels, sweeps) = timed(lambda: sm.debug_region(ctx, nrm, lists, cth), a.repeats)
    lines.append("%-44s %10.1f ms  (spread %.1f)  %d label-sweep launches, %d regions" % ("region labels", ms, spread, sweeps, len(np.unique(labels))))
    ms, spread, (flags, gaps) = timed(lambda: sm.debug_boundary(ctx, pts, nrm, P["boundary_radius"], P["boundary_angle"]), a.repeats)
    lines.append("%-44s %10.1f ms  (spread %.1f)  %d boundary points" % ("boundary (radius 0.1)", ms, spread, int(flags.sum())))
    assert int(flags.sum()) == st["boundary_points"] and len(filt) == st["filtered_points"]
    ctx.close()
    # the CPU figure: the restatement on the corner where floor and both walls meet
    crop = cloud[np.all(cloud < np.array([2.0, 3.0, 0.5], np.float32) + np.float32(a.cpu_crop), axis=1)]
    t0 = time.perf_counter()
    ref = R.extract(crop, partition_min_points=1)
    cpu = time.perf_counter() - t0
    lines += ["", "numpy restatement (tests/survey_map_ref.py, brute-force searches) on the %g m corner of the same survey: %d points -> "
              "%d filtered, %.1f s" % (a.cpu_crop, len(crop), ref["stats"]["filtered_points"], cpu),
              "  (quadratic in the block size: it is the parity yardstick, not a tuned CPU implementation; the reference's own PCL "
              "pipeline is not available to time)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
