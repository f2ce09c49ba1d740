#!/usr/bin/env python3
"""Cost of the occupancy grid over a keyframe store: CLOUDS keyframes of synth.make_scan(rings=16, azimuth_steps=1800) along a
street integrated into a grid of 0.1 m cells fitted to the poses (max_range 40 m), timed with HIP events on the library's own
stream (lslam_stream).  Figures, each the median of REPS after 10 warm-up calls:
  integrate  one clear + lslam_occ_integrate call over every keyframe: the jobs' upload, per chunk of LSLAM_OCC_KF_CHUNK keyframes
             the zeroing of its bit planes, the ray kernel and the merge, the counters' download, the wait
  kernel     the ray kernels of that call alone (lslam_debug_occ_integrate: 5 passes per sample, the time per pass, the zeroing of
             the bit planes included)
  values     the int8 values from the counts plus their download
and rays per second = rays cast / time.  `cpu_reference` is tests/occupancy_ref.py (numpy) on 2000 points of the first keyframe and a 40 m x 40 m
corner of the grid, as rays per second: the CPU figure.  Prints one JSON line and, with an argument, writes it to that file
(profiles/r24_occupancy.txt is the one DESIGN 8i quotes)."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS = int(os.environ.get("REPS", "30"))
CLOUDS = int(os.environ.get("CLOUDS", "16"))
TAP_PASSES = 5


def pose_matrix(p6):
    rx, ry, rz = p6[:3]
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, p6[3:6]
    return T


def main():
    import torch
    import occupancy_ref as R
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = pkg.Context(0)
    store = pkg.KeyframeStore(ctx)
    world = synth.World(half_extent=60.0, wall_half=55.0)
    ids, poses, clouds = [], [], []
    for k in range(CLOUDS):
        gt = (0.0, 0.0, 0.3 + 0.05 * k, 3.0 + 0.5 * k, -2.0 + 0.2 * k, synth.SENSOR_HEIGHT)
        corner, surf, _ = synth.make_scan(world, 16, 1800, gt_pose=gt, seed=500 + k)
        ids.append(store.add(corner, surf))
        poses.append(pose_matrix(np.asarray(gt, np.float64)).astype(np.float32))
        clouds.append((corner, surf))
    params = pkg.occupancy.fit_bounds(poses, up_axis=2)
    store.occ_setup(params)
    stream = C.c_void_p(ctx.lib.lslam_stream(ctx.h))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(call, per=1):
        ms = []
        for _ in range(REPS + 10):
            assert hip.hipEventRecord(ev[0], stream) == 0
            call()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
            ms.append(t.value / per)
        ms = ms[10:]
        return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "p90_us": 1e3 * sorted(ms)[int(0.9 * len(ms))]}

    before = store.info()
    store.occ_integrate(ids, poses)
    info = store.occ_info()
    values = store.occ_values()
    out = {"clouds": CLOUDS, "points": int(sum(len(c) + len(s) for c, s in clouds)), "width": params.width, "height": params.height,
           "rays_cast": info["rays_cast"], "rays_obstacle": info["rays_obstacle"], "rays_ground": info["rays_ground"],
           "rays_dropped": info["rays_dropped"], "grid_bytes": info["grid_bytes"], "scratch_bytes": info["scratch_bytes"], "reps": REPS,
           "cells_occupied": int((values >= 65).sum()), "cells_free": int(((values >= 0) & (values <= 19)).sum()),
           "cells_unknown": int((values < 0).sum())}

    def whole():
        store.occ_clear()
        store.occ_integrate(ids, poses)

    out["integrate"] = timed(whole)
    out["kernel"] = timed(lambda: store._check(ctx.lib.lslam_debug_occ_integrate(store.h, TAP_PASSES)), per=TAP_PASSES)

    def fresh_values():
        whole()
        assert hip.hipEventRecord(ev[0], stream) == 0  # only the values are timed
        store.occ_values()

    out["values"] = timed(fresh_values)
    for k in ("integrate", "kernel"):
        out[k]["rays_per_s"] = info["rays_cast"] / (out[k]["median_us"] * 1e-6)
    after = store.info()
    out["cloud_bytes_moved"] = (after["cloud_bytes_uploaded"] - before["cloud_bytes_uploaded"]) + (after["cloud_bytes_downloaded"] - before["cloud_bytes_downloaded"])
    # the CPU figure: the numpy reference on 2000 points of one keyframe and a 400 x 400 cell corner around it
    a0 = float(poses[0][0, 3]) - 20.0
    b0 = float(poses[0][1, 3]) - 20.0
    small = R.params(up_axis=2, origin=(a0, b0), width=400, height=400)
    t0 = time.perf_counter()
    _, _, st = R.keyframe_vote(clouds[0][0][:500], clouds[0][1][:1500], poses[0], None, small)
    dt = time.perf_counter() - t0
    out["cpu_reference"] = {"rays": st["cast"], "seconds": dt, "rays_per_s": st["cast"] / dt}
    out["compute_units"] = torch.cuda.get_device_properties(0).multi_processor_count
    for e in ev:
        hip.hipEventDestroy(e)
    store.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("tools/bench_occupancy.py on one MI355X (its one JSON line)\n" + line + "\n")


if __name__ == "__main__":
    main()
