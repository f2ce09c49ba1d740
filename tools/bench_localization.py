#!/usr/bin/env python3
"""Localisation over a prebuilt map per sweep, three ways, taken in turn in one process through the C ABI with buffers made once:

  A  the composed path of the four existing calls: lslam_voxel_grid2 (the sweep's clouds go up, come down filtered),
     lslam_fmap_update, lslam_fmap_to_cubemap, lslam_scanmatch_scan with variant-C options (the filtered clouds go up again)
  B  the localisation node (lslam_loc_match: the two filters and FeatureMap::scanMatchScan on the device, one wait), grid path on
  C  the node with the grid path off (every point through its cube's tree)

on seeded 16 x 1800 and 64 x 1800 sweeps against a saved map of the bench world (synth.World(), 350 m across), loaded with
the 1.0 m per-cube filter by both.  Every sweep starts from the same perturbed pose in A, B and C.  Every call ends in its own
wait, so the host clock around it is the time per sweep.  Medians over --sweeps sweeps per variant, --repeats repeats of the
whole measurement (the spread of A's medians is the noise a difference has to beat).  B must agree with A to the project's
pose tolerances and with C bit for bit, or the script exits non-zero.  Bytes over PCIe: counted from the shapes for A,
reported by the node for B and C; waits: A's are the ones its four calls are known to make (voxel_grid2 1, to_cubemap 1,
scanmatch_scan 1; more when the active area changes), the node's are counted by the node.  Prints a table and one JSON line."""
import argparse
import ctypes as C
import gc
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIMS = (121, 121, 11)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rings", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--world-half", type=float, default=175.0)
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    capi = importlib.import_module("the-cooper-mapper_amd.capi")
    fp = lambda a: a.ctypes.data_as(capi.c_float_p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx = pkg.Context(0)
    lib = ctx.lib
    world = synth.World(half_extent=args.world_half, wall_half=min(90.0, args.world_half - 5.0))
    map_c, map_s = synth.make_map(world, 0.2, 0.4, seed=77)
    tmp = tempfile.mkdtemp(prefix="lslam_loc_bench_")
    saver = pkg.FeatureMap(ctx, *DIMS)
    saver.add_feature_cloud(map_c, map_s, np.eye(4, dtype=np.float32))
    saver.save_cloud_to_files(tmp)
    saver.close()
    fm = pkg.FeatureMap(ctx, *DIMS)
    fm.setup_filter_size(1.0, 1.0, 2.0)
    fm.load_cloud_from_files(tmp)
    nodes = {}
    for v, grid in (("B", True), ("C", False)):
        nodes[v] = pkg.LaserLocalization(ctx, *DIMS)
        nodes[v].load_map(tmp)
        nodes[v].set_search(grid)
    info = nodes["B"].info()
    print("map: %d + %d points saved, %d + %d after the 1.0 m per-cube filter, %d + %d cube trees" %
          (len(map_c), len(map_s), info["n_points"][0], info["n_points"][1], info["cubes_with_tree"][0], info["cubes_with_tree"][1]))
    opts = ctx.default_opts()
    opts.max_iterations, opts.delta_t_abort, opts.delta_r_abort, opts.use_score = 10, 0.05, 0.05, 0
    result = {}
    rc_all = 0
    for rings in args.rings:
        sweeps = []
        for k in range(4):
            gt = (0.01, -0.015, 0.3 + 0.02 * k, 3.0 + 0.5 * k, -2.0 + 0.2 * k, synth.SENSOR_HEIGHT)
            c, s, _ = synth.make_scan(world, rings, 1800, gt_pose=gt, seed=1234 + k)
            sweeps.append((np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32),
                           synth.perturb_pose(gt, seed=99 + k, dt=0.2, dr_deg=1.0)))
        cap = max(max(len(c), len(s)) for c, s, _ in sweeps)
        oa, ob = np.zeros((cap, 4), np.float32), np.zeros((cap, 4), np.float32)
        na, nb = C.c_size_t(), C.c_size_t()
        st = capi.LslamStats()
        filtered = [0, 0]

        def run_a(c, s, p0):
            pose = p0.copy()
            pos = np.ascontiguousarray(pose[3:], np.float32)
            rc = lib.lslam_voxel_grid2(ctx.h, vp(c), len(c), vp(s), len(s), 16, 1.0, fp(oa), cap, C.byref(na), fp(ob), cap, C.byref(nb))
            if rc >= 0:
                rc = lib.lslam_fmap_update(fm.h, fp(pos))
            if rc >= 0:
                rc = lib.lslam_fmap_to_cubemap(fm.h)
            if rc >= 0:
                rc = lib.lslam_scanmatch_scan(ctx.h, vp(oa), na.value, vp(ob), nb.value, 16, fp(pose), C.byref(opts), C.byref(st))
            if rc < 0:
                raise pkg.LslamError(rc, lib.lslam_last_error().decode())
            filtered[0], filtered[1] = na.value, nb.value
            return pose, st.iterations, st.n_rows

        def run_node(v):
            h = nodes[v].h

            def f(c, s, p0):
                pose = p0.copy()
                rc = lib.lslam_loc_match(h, vp(c), len(c), vp(s), len(s), 16, fp(pose), C.byref(st))
                if rc < 0:
                    raise pkg.LslamError(rc, lib.lslam_last_error().decode())
                return pose, st.iterations, st.n_rows
            return f
        variants = {"A": run_a, "B": run_node("B"), "C": run_node("C")}
        for c, s, p0 in sweeps[:3]:
            (pa, ia, ra), (pb, ib, rb), (pc, ic, rcn) = (variants[v](c, s, p0) for v in "ABC")
            if not np.array_equal(pb.view(np.uint32), pc.view(np.uint32)):
                print("FAIL: the node's pose depends on its search path")
                rc_all = 1
            if (ia, ra) != (ib, rb) or np.abs(pa[3:] - pb[3:]).max() > 1e-4 or np.abs(pa[:3] - pb[:3]).max() > 1e-5:
                print("FAIL: the node and the composed path disagree: iterations %d / %d, rows %d / %d, |dt| %.2e, |dr| %.2e" %
                      (ia, ib, ra, rb, np.abs(pa[3:] - pb[3:]).max(), np.abs(pa[:3] - pb[:3]).max()))
                rc_all = 1
        for i in range(args.warmup):
            for f in variants.values():
                f(*sweeps[i % len(sweeps)])
        gc.collect(); gc.freeze(); gc.disable()
        med = {v: [] for v in variants}
        for _ in range(args.repeats):
            host = {v: [] for v in variants}
            for i in range(args.sweeps):
                sw = sweeps[i % len(sweeps)]
                for v, f in variants.items():
                    t = time.perf_counter()
                    f(*sw)
                    host[v].append(time.perf_counter() - t)
            for v in variants:
                med[v].append(float(np.median(host[v]) * 1e3))
        gc.enable()
        n_in = int(np.mean([len(c) + len(s) for c, s, _ in sweeps]))
        n_f = filtered[0] + filtered[1]
        rows = {"A": dict(up=n_in * 16 + n_f * 16 + 24, down=n_f * 16 + 24, waits=3)}
        shares = {}
        for v in ("B", "C"):
            variants[v](*sweeps[0])
            ss = nodes[v].search_stats()
            rows[v] = dict(up=ss["bytes_up"][0], down=ss["bytes_down"][0], waits=ss["host_waits"][0])
            sw = max(ss["swept"][0], 1)
            shares[v] = dict(swept=ss["swept"][0], grid_proven=ss["grid_proven"][0] / sw, cube_refused=ss["cube_refused"][0] / sw,
                             to_trees=ss["to_trees"][0] / sw, fallback_sweeps=ss["fallback_sweeps"][0])
        print("%d x 1800 (%d points in, %d after the scan filters), medians of %d sweeps, %d repeats (min .. max of the medians)" %
              (rings, n_in, n_f, args.sweeps, args.repeats))
        for v in variants:
            h = med[v]
            rows[v].update(host_ms=float(np.median(h)), host_ms_min=min(h), host_ms_max=max(h))
            print("  %s host %.3f ms (%.3f .. %.3f)   up %8d B  down %8d B  waits %d" %
                  (v, rows[v]["host_ms"], min(h), max(h), rows[v]["up"], rows[v]["down"], rows[v]["waits"]))
        print("  B search shares over the loop's sweeps: proven by the grid %.1f %%, refused by the cube check %.2f %%, sent to cube trees %.1f %% of %d" %
              (100 * shares["B"]["grid_proven"], 100 * shares["B"]["cube_refused"], 100 * shares["B"]["to_trees"], shares["B"]["swept"]))
        spread_a = max(med["A"]) - min(med["A"])
        gain = rows["A"]["host_ms"] - rows["B"]["host_ms"]
        print("  A - B = %.3f ms (spread of A's repeats %.3f ms): %s;  C - B = %.3f ms (what the grid path saves)" %
              (gain, spread_a, "B is faster" if gain > spread_a else "no gain beyond the noise", rows["C"]["host_ms"] - rows["B"]["host_ms"]))
        result["%dx1800" % rings] = dict(points=n_in, filtered=n_f, variants=rows, shares=shares, a_minus_b_ms=gain, a_spread_ms=spread_a,
                                         c_minus_b_ms=rows["C"]["host_ms"] - rows["B"]["host_ms"])
    print(json.dumps(dict(tool="bench_localization", sweeps=args.sweeps, repeats=args.repeats, map_points=list(info["n_points"]), result=result)))
    for n in nodes.values():
        n.close()
    fm.close()
    ctx.close()
    return rc_all


if __name__ == "__main__":
    sys.exit(main())
