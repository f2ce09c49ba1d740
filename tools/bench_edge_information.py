#!/usr/bin/env python3
"""What one pose-graph edge's information costs (lslam_keyframe_edge_information), for a keyframe-sized pair: two consecutive
keyframes of bench.py's final_feature_map leg (16 x 1800 sweeps, 0.26 m apart), the first as the reference.

  edge       lslam_keyframe_edge_information: local clouds, VoxelGrid x 4, map set, scan set, sweep, reduction, download, Jacobi
  info       lslam_match_information on what that call left resident: sweep with device taps, reduction, download, Jacobi
  sweep      lslam_sweep_ex at the same pose, sums only (no taps): the sweep that feeds the reduction
  sweep+taps lslam_sweep_ex with all four taps downloaded: what a caller had to do before this entry point existed
  set-up     edge - info;  new kernel (reduction + download + Jacobi, an upper bound: the taps' stores are in it) = info - sweep

Host clocks around calls that end in a device wait, after a warm-up; medians over --repeats.  Prints one JSON line.

    python tools/bench_edge_information.py [--repeats 50] [--device 0]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import synth_gpu
    ctx = pkg.Context(args.device)  # raises without a GPU: nothing here falls back
    world = synth.World(half_extent=300.0, wall_half=295.0, pole_pitch=2.5)
    lidar = synth_gpu.GpuLidar(world, args.device)
    traj = synth_gpu.loop_trajectory(5000)
    store = pkg.KeyframeStore(ctx)
    ids, T = [], []
    for k in range(2):
        c, s = lidar.scan(traj[k], 16, 1800, seed=555000 + k)
        ids.append(store.add(np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32)))
        T.append(ctx.pose_to_isometry(traj[k].astype(np.float32)).astype(np.float64))
    rel = (np.linalg.inv(T[0]) @ T[1]).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)[None]
    pose = ctx.isometry_to_pose(rel)
    counts = [store.counts(i) for i in ids]

    # the resident scan the call leaves: the new keyframe through VoxelGrid 0.2 / 0.4
    voxel_grid = importlib.import_module("the-cooper-mapper_amd.feature_map").voxel_grid
    n = len(voxel_grid(ctx, store.get(ids[1], 0), 0.2)) + len(voxel_grid(ctx, store.get(ids[1], 1), 0.4))
    info = store.edge_information([ids[0]], eye, ids[1], rel)
    out = dict(tool="bench_edge_information", keyframe_points=[list(map(int, c)) for c in counts], n_rows=int(info.n_rows),
               n_line=int(info.n_line), n_plane=int(info.n_plane), eig=[float(v) for v in info.eig], repeats=args.repeats)
    out["edge_ms"], out["edge_ms_min"] = median_ms(lambda: store.edge_information([ids[0]], eye, ids[1], rel), args.repeats)
    out["info_ms"], out["info_ms_min"] = median_ms(lambda: ctx.match_information(pose, 0), args.repeats)
    out["sweep_ms"], out["sweep_ms_min"] = median_ms(lambda: ctx.sweep(pose, jtj_mode=1, taps=False, search_mode=0), args.repeats)
    ctx.n_scan = n  # the taps' host buffers
    out["scan_points"] = n
    out["sweep_taps_ms"], out["sweep_taps_ms_min"] = median_ms(lambda: ctx.sweep(pose, jtj_mode=1, taps=True, search_mode=0), args.repeats)
    out["setup_ms"] = out["edge_ms"] - out["info_ms"]
    out["new_kernel_ms"] = out["info_ms"] - out["sweep_ms"]
    store.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
