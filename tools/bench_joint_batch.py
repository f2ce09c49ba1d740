"""Joint LiDAR + stereo scan match of a batch of resident scans (lslam_stereo_set_batch) against the LiDAR-only batch.

K scans (default 64 of 64 rings x 1800, ray cast by tools/synth_gpu.py) at distinct poses in one world, each with its own
stereo observations at its ground truth (synth.make_stereo, default 2 000, camera weight 1e-3).  run_batch is timed LiDAR-only
and joint on the same resident scans, warmed up, the two alternated in one process, as the median of --calls calls each.
Checks of the same run: two sampled scans against oracle.scanmatch_joint (1e-4 m, 1e-5 rad), three bit-equal to their single
joint runs (lslam_stereo_set + scanmatch_scan).  Prints one JSON line.

    python tools/bench_joint_batch.py [--scans 64] [--obs 2000] [--calls 20] [--no-oracle]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRID = 3  # LSLAM_SEARCH_GRID: what AUTO takes for a batch of this size, stated so that the single runs take it too


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--obs", type=int, default=2000)
    ap.add_argument("--weight", type=float, default=1e-3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()

    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import synth_gpu

    t_setup = time.perf_counter()
    world = synth.World(half_extent=175.0, wall_half=90.0)
    map_c, map_s = synth.make_map(world, seed=77)
    lidar = synth_gpu.GpuLidar(world, 0)
    rng = np.random.default_rng(7)
    pts = np.concatenate([map_c, map_s])
    # the cameras' candidates: map points within reach of the whole trajectory (make_stereo culls by view and depth)
    near = pts[np.abs(pts[:, :2]).max(axis=1) < 110.0]
    scans, gts, inits, sets = [], [], [], []
    for k in range(a.scans):
        ang = 2 * np.pi * k / a.scans
        gt = (0.01 * rng.standard_normal(), 0.01 * rng.standard_normal(), ang + 0.3,
              35.0 * np.cos(ang), 35.0 * np.sin(ang), synth.SENSOR_HEIGHT)
        qc, qs = lidar.scan(gt, a.rings, 1800, seed=7000 + k)
        scans.append((qc, qs))
        gts.append(np.asarray(gt, np.float64))
        inits.append(synth.perturb_pose(gt, seed=8000 + k))
        lm, ob, w = synth.make_stereo(near, gt, n=a.obs, seed=9000 + k)
        sets.append((lm, ob, w))
    inits = np.stack(inits).astype(np.float32)
    t_setup = time.perf_counter() - t_setup

    ctx = pkg.Context(0)
    ctx.map_set(map_c, map_s)
    cam = ctx.default_stereo_cam()
    for i, v in enumerate(synth.T_CAM_LIDAR.reshape(-1)):
        cam.T_cl[i] = float(v)
    cam.weight = a.weight
    opts = ctx.default_opts()
    opts.search_mode = GRID

    # single joint runs of three sampled scans (before the batch is resident: scanmatch_scan replaces it)
    sample_bits = [0, a.scans // 2, a.scans - 1]
    singles = {}
    for k in sample_bits:
        ctx.stereo_set(*sets[k], cam)
        singles[k] = ctx.scanmatch_scan(scans[k][0], scans[k][1], inits[k], opts)
    ctx.stereo_clear()

    ctx.scan_set_batch(scans)
    ms = {"lidar": [], "joint": []}
    last = {}

    def call(kind):
        if kind == "joint":
            ctx.stereo_set_batch(sets, cam)
        else:
            ctx.stereo_clear()
        t0 = time.perf_counter()
        _, poses, stats = ctx.run_batch(inits, opts)
        dt = time.perf_counter() - t0
        last[kind] = (poses, stats)
        return dt

    for _ in range(a.warmup):
        call("lidar")
        call("joint")
    for i in range(a.calls):  # alternated, the order flipped every other round
        for kind in (("lidar", "joint") if i % 2 == 0 else ("joint", "lidar")):
            ms[kind].append(1e3 * call(kind))
    ctx.stereo_clear()

    lid_ms, jnt_ms = float(np.median(ms["lidar"])), float(np.median(ms["joint"]))
    poses_j, stats_j = last["joint"]
    _, stats_l = last["lidar"]
    pr_l = sum(s.point_residuals for s in stats_l)
    pr_j = sum(s.point_residuals for s in stats_j)
    stereo_rows = sum(s.n_rows for s in stats_j) - sum(s.n_rows for s in stats_l)

    bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
    bit_equal = all(np.array_equal(bits(poses_j[k]), bits(singles[k][1])) and stats_j[k].iterations == singles[k][2].iterations
                    and stats_j[k].n_rows == singles[k][2].n_rows for k in sample_bits)
    oracle_ok, oracle_err = None, None
    if not a.no_oracle:
        from oracle_lib import Oracle
        from test_oracle_stereo import default_cam
        oracle = Oracle()
        ocam = default_cam(weight=a.weight)
        oracle_ok, oracle_err = True, []
        for k in (1, a.scans // 3):
            ok, opose, ost, used = oracle.scanmatch_joint(map_c, map_s, scans[k][0], scans[k][1], *sets[k], ocam, inits[k])
            dm = float(np.abs(poses_j[k][3:] - opose[3:]).max())
            dr = float(np.abs(poses_j[k][:3] - opose[:3]).max())
            oracle_err.append([dm, dr])
            oracle_ok = oracle_ok and dm <= 1e-4 and dr <= 1e-5 and stats_j[k].iterations == ost.iterations
    out = {
        "metric": "joint_batch_ms",
        "scans": a.scans, "rings": a.rings, "obs_per_scan": a.obs, "weight": a.weight, "calls": a.calls,
        "lidar_ms": round(lid_ms, 4), "joint_ms": round(jnt_ms, 4), "overhead": round(jnt_ms / lid_ms, 4),
        "lidar_point_residuals_per_s": pr_l / (lid_ms * 1e-3),
        "joint_point_residuals_per_s": pr_j / (jnt_ms * 1e-3),
        "joint_rows_per_s": sum(s.n_rows * s.sweeps for s in stats_j) / (jnt_ms * 1e-3),
        "stereo_rows_last_sweep": int(stereo_rows),
        "iterations_lidar": int(sum(s.iterations for s in stats_l)), "iterations_joint": int(sum(s.iterations for s in stats_j)),
        "bit_equal_singles": bool(bit_equal), "oracle_ok": oracle_ok, "oracle_err_m_rad": oracle_err,
        "setup_s": round(t_setup, 1),
    }
    print(json.dumps(out))
    ctx.close()
    return 0 if bit_equal and oracle_ok is not False else 1


if __name__ == "__main__":
    sys.exit(main())
