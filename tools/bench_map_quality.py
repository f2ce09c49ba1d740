#!/usr/bin/env python3
"""Cost of the map-quality evaluation (lslam_mapq_eval_device) on the bench's map: the surround of the 10k-frame voxel map of
BASELINE configs[1] (the generator call of tools/dump_bench_workload.py) -- its surf half and the whole map, corner + surf -- at
r = 0.15, 0.3 and 0.6.  Per (cloud, radius), after WARM warm-up calls, REPS calls: the call between two HIP events on the
library's stream, and the library's own stage times (lslam_mapq_stats.ms_*: sort, kernel = the neighbourhood sums,
reduce = the per-point tail with the aggregates' reduction); medians with min and max.  One JSON line each.

  --normals   instead: one lslam_debug_survey_normals call per radius on the surf half (the parent's radius search with PCA,
              sv_normals_kernel), for a `rocprofv3 --kernel-trace --stats` run of its own: that kernel's time is the
              yardstick, not the tap's uploads
  --workload  npz with map_corner / map_surf to use instead of building the map (written by --save-workload)
Bench infrastructure, not product code."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
RADII = (0.15, 0.3, 0.6)
WARM, REPS = 2, 5


def workload(pkg, ctx, frames):
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import synth_gpu
    world_model = synth.World(half_extent=300.0, wall_half=295.0, pole_pitch=2.5)
    lidar = synth_gpu.GpuLidar(world_model, 0)
    traj = synth_gpu.loop_trajectory(frames)
    fm, stats = synth_gpu.build_voxel_map(pkg, ctx, lidar, traj, rings=16, progress=2000)
    fm.update(traj[-1][3:].astype(np.float32))
    sc, ss = fm.get_surround_feature()
    fm.close()
    return sc, ss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--workload")
    ap.add_argument("--save-workload")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("the-cooper-mapper_amd")
    ctx = pkg.Context(0)
    if args.workload:
        z = np.load(args.workload)
        sc, ss = z["map_corner"], z["map_surf"]
    else:
        sc, ss = workload(pkg, ctx, args.frames)
    if args.save_workload:
        np.savez(args.save_workload, map_corner=sc, map_surf=ss)
    clouds = {"surf": np.ascontiguousarray(ss[:, :4], np.float32), "whole": np.ascontiguousarray(np.concatenate([sc, ss])[:, :4], np.float32)}
    if args.normals:
        for r in RADII:
            out, cnt = pkg.survey_map.debug_normals(ctx, clouds["surf"], clouds["surf"], r)
            print(json.dumps({"normals_radius": r, "points": int(len(cnt)), "mean_neighbors": float(cnt.mean()),
                              "defined": int(np.isfinite(out[:, 0]).sum())}), flush=True)
        ctx.close()
        return
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    stream = C.c_void_p(ctx.lib.lslam_stream(ctx.h))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    spread = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for name, cloud in clouds.items():
        d = torch.from_numpy(cloud).to("cuda:%d" % ctx.device)
        for r in RADII:
            rows = []
            for rep in range(WARM + REPS):
                assert hip.hipEventRecord(ev[0], stream) == 0
                st = pkg.map_quality.evaluate(ctx, d, radius=r)
                assert hip.hipEventRecord(ev[1], stream) == 0
                assert hip.hipEventSynchronize(ev[1]) == 0
                t = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
                rows.append(dict(call=t.value, sort=st["ms_sort"], kernel=st["ms_kernel"], reduce=st["ms_reduce"]))
            rows = rows[WARM:]
            line = {"cloud": name, "points": int(len(cloud)), "radius": r, "reps": REPS,
                    "ms": {k: spread([row[k] for row in rows]) for k in ("call", "sort", "kernel", "reduce")},
                    "ns_per_point_kernel": round(1e6 * statistics.median([row["kernel"] for row in rows]) / len(cloud), 3),
                    "mean_neighbors": round(st["mean_neighbors"], 3), "max_neighbors": st["max_neighbors"], "n_defined": st["n_defined"],
                    "n_sparse": st["n_sparse"], "mme": st["mean_entropy"], "mpv": st["mean_plane_variance"]}
            print(json.dumps(line), flush=True)
    for e in ev:
        hip.hipEventDestroy(e)
    ctx.close()


if __name__ == "__main__":
    main()
