#!/usr/bin/env python3
"""Loop candidates by appearance (lslam_sc_*, csrc/lslam_sc.hip) over stores of --sizes keyframes: the describe pass, one
query against the whole store, a batch of --batch queries, and the numpy restatement (tests/place_recognition_ref.py) on 100
candidates as the CPU figure beside them.  Host wall clock around calls that wait for their result once;
medians of --repeats runs after one untimed run.  Writes the table to --out (kept as profiles/rNN_place_recognition.txt).

The stores: --distinct synthetic 16 x 450 scans of the test world (seeded positions and yaws), uploaded once as device
tensors and added in rotation (lslam_kfs_add_device), so a large store costs HBM but little time to make.  Identical
descriptors change neither the describe nor the query kernel's work: both are data independent but for the points a cloud holds.
The describe figure includes the slabs' allocation: parameters are switched to drop the descriptors before each timed pass."""
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

HBM_TBS = 6.29      # float4 copy, measured (the MI355X guide)
FP32_TFLOPS = 157.3  # vector peak, 2 flop per multiply-add


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 65536])
    ap.add_argument("--distinct", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_place_recognition.txt"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import place_recognition_ref as R
    world = synth.make_problem(rings=16, azimuth_steps=900, world_half=60.0)["world"]
    rng = np.random.default_rng(a.seed)
    scans = []
    for i in range(a.distinct):
        x, y, yaw = rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(-np.pi, np.pi)
        c, s, _ = synth.make_scan(world, 16, 450, gt_pose=(0.0, 0.0, yaw, x, y, synth.SENSOR_HEIGHT), seed=5000 + i)
        scans.append((c, s))
    p = R.params(up_axis=2)
    n_ring, n_sector = p["n_ring"], p["n_sector"]
    form_bytes, macs = (n_ring + 1) * n_sector * 4, n_ring * n_sector * n_sector
    pts = np.mean([len(c) + len(s) for c, s in scans])
    lines = ["scan context %d x %d, up_axis 2; %d distinct 16 x 450 scans (mean %.0f points), added in rotation" % (n_ring, n_sector, a.distinct, pts),
             "host wall clock, median of %d runs after one untimed run (spread = max - min); every call waits once" % a.repeats,
             "per pair: %d B of candidate read, %d multiply-adds; yardsticks: %.2f TB/s HBM (measured copy), %.1f TFLOPS fp32 vector peak"
             % (form_bytes, macs, HBM_TBS, FP32_TFLOPS), ""]
    ctx = pkg.Context(0)
    dev = [(torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda()) for c, s in scans]
    for n in a.sizes:
        store = pkg.KeyframeStore(ctx, max_points=1 << 30, max_keyframes=max(n, 1))
        t0 = time.perf_counter()
        for i in range(n):
            store.add(*dev[i % a.distinct])
        t_add = time.perf_counter() - t0
        flip = [0]

        def describe():
            flip[0] ^= 1
            store.sc_setup(**dict(p, height_offset=2.0 + 0.5 * flip[0]))
            t = time.perf_counter()
            store.sc_descriptor(0)
            return time.perf_counter() - t
        describe()
        ds = [describe() for _ in range(a.repeats)]
        store.sc_setup(**p)
        store.sc_descriptor(0)
        info = store.sc_info()
        ms1, sp1, one = timed(lambda: store.sc_query([n - 1], [n - 2], a.top_k), a.repeats)
        qs = [int(v) for v in rng.integers(0, n, a.batch)]
        msb, spb, _ = timed(lambda: store.sc_query(qs, [n - 1] * a.batch, a.top_k), a.repeats)
        d_ms = statistics.median(ds) * 1e3
        lines += ["store of %d keyframes (made in %.1f s; descriptors %.1f MB)" % (n, t_add, info["descriptor_bytes"] / 1e6),
                  "  %-40s %9.3f ms  = %.2f us per keyframe" % ("describe all (one launch + slab allocation)", d_ms, d_ms * 1e3 / n),
                  "  %-40s %9.3f ms  (spread %.3f)  %.1f GB/s of candidate reads (%.1f %% of HBM), %.2f TFLOPS (%.1f %% of peak)"
                  % ("one query, top %d" % a.top_k, ms1, sp1, (n - 1) * form_bytes / ms1 / 1e6, (n - 1) * form_bytes / ms1 / 1e6 / (HBM_TBS * 10),
                     2 * (n - 1) * macs / ms1 / 1e9, 2 * (n - 1) * macs / ms1 / 1e9 / FP32_TFLOPS * 100),
                  "  %-40s %9.3f ms  (spread %.3f)  = %.3f ms per query, %.2f TFLOPS (%.1f %% of peak)"
                  % ("%d queries in one call" % a.batch, msb, spb, msb / a.batch, 2 * a.batch * n * macs / msb / 1e9,
                     2 * a.batch * n * macs / msb / 1e9 / FP32_TFLOPS * 100),
                  "  best of the single query: ids %s dist %s" % (one[0][0].tolist(), [round(float(v), 4) for v in one[0][2]]), ""]
        store.close()
    ctx.close()
    # the CPU figure
    D = [R.descriptor(c, s, p) for c, s in scans[:101]]
    t0 = time.perf_counter()
    for C in D[1:101]:
        R.distance(D[0], C)
    cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    for c, s in scans[:20]:
        R.descriptor(c, s, p)
    cpu_d = (time.perf_counter() - t0) / 20
    lines += ["numpy restatement (tests/place_recognition_ref.py): one query against 100 candidates %.1f ms (%.2f ms per pair, float64); "
              "a descriptor %.2f ms" % (cpu * 1e3, cpu * 10, cpu_d * 1e3),
              "  (the parity yardstick, not a tuned CPU implementation)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
