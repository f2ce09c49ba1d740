#!/usr/bin/env python3
"""Cost of the visibility votes over a keyframe store: CLOUDS keyframes of synth.make_scan(rings=16, azimuth_steps=1800) along a
street, every point of every keyframe (in the graph frame) voted on by VOTERS voters (the keyframes in turn), timed with HIP
events on the library's own stream (lslam_stream).  Figures, each the median of REPS after 20 warm-up calls:
  images  one lazy build of all range images (new parameters drop them, the next call rebuilds: fill + image kernel)
  votes   one lslam_vis_votes_device call: the voters' upload, the zeroing of the votes, the vote kernel, the wait
  kernel  the vote kernel alone (lslam_debug_vis_votes: 10 launches per sample, the time per launch, the zeroing included)
and votes per second = query points x voters / time: every (point, voter) pair counts, also those the range gate ends early;
`gate_share` says how many passed it (from the returned votes of single voters this cannot be read, so it is computed on the
host from the poses: the share of pairs closer than max_range).  Prints one JSON line."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "100"))
CLOUDS = int(os.environ.get("CLOUDS", "16"))
VOTERS = int(os.environ.get("VOTERS", "16"))
TAP_LAUNCHES = 10


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
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = pkg.Context(0)
    store = pkg.KeyframeStore(ctx)
    params = dict(up_axis=2)
    store.vis_setup(**params)
    world = synth.World(half_extent=60.0, wall_half=55.0)
    ids, poses, query = [], [], []
    for k in range(CLOUDS):
        gt = (0.0, 0.0, 0.3 + 0.05 * k, 3.0 + 0.5 * k, -2.0 + 0.2 * k, synth.SENSOR_HEIGHT)
        corner, surf, _ = synth.make_scan(world, 16, 1800, gt_pose=gt, seed=500 + k)
        ids.append(store.add(corner, surf))
        T = pose_matrix(np.asarray(gt, np.float64))
        poses.append(T)
        for c in (corner, surf):
            g = np.zeros((len(c), 4), np.float32)
            g[:, :3] = c[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            query.append(g)
    query = np.ascontiguousarray(np.concatenate(query))
    v_ids = [ids[k % CLOUDS] for k in range(VOTERS)]
    v_poses = [poses[k % CLOUDS] for k in range(VOTERS)]
    d_query = torch.from_numpy(query).to("cuda:%d" % ctx.device)
    stream = C.c_void_p(ctx.lib.lslam_stream(ctx.h))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(call, per=1):
        ms = []
        for _ in range(REPS + 20):
            assert hip.hipEventRecord(ev[0], stream) == 0
            call()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
            ms.append(t.value / per)
        ms = ms[20:]
        return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "p90_us": 1e3 * sorted(ms)[int(0.9 * len(ms))]}

    before = store.info()
    words = store.vis_votes(v_ids, v_poses, query)  # host points: arms the measurement tap
    nf, nh = pkg.visibility.split_votes(words)
    pairs = float(len(query)) * float(VOTERS)
    max_range = store.vis_info()["max_range"]
    near = sum(int((np.linalg.norm(query[:, :3] - T[:3, 3].astype(np.float32), axis=1) <= max_range).sum()) for T in v_poses)
    out = {"clouds": CLOUDS, "voters": VOTERS, "query_points": int(len(query)), "pairs": pairs, "gate_share": near / pairs,
           "reps": REPS, "points_with_free_votes": int((nf > 0).sum()), "points_with_hit_votes": int((nh > 0).sum()),
           "dynamic": int(pkg.visibility.dynamic_mask(words, store.vis_info()["min_free_votes"]).sum())}

    def rebuild():
        store.vis_setup(window=0, **params)
        store.vis_setup(**params)
        store.vis_range_image(ids[0])

    out["images"] = timed(rebuild)
    out["votes"] = timed(lambda: store.vis_votes(v_ids, v_poses, d_query))
    store.vis_votes(v_ids, v_poses, query)
    out["kernel"] = timed(lambda: store._check(ctx.lib.lslam_debug_vis_votes(store.h, TAP_LAUNCHES)), per=TAP_LAUNCHES)
    for k in ("votes", "kernel"):
        out[k]["pair_votes_per_s"] = pairs / (out[k]["median_us"] * 1e-6)
    after = store.info()
    out["cloud_bytes_moved"] = (after["cloud_bytes_uploaded"] - before["cloud_bytes_uploaded"]) + (after["cloud_bytes_downloaded"] - before["cloud_bytes_downloaded"])
    out["compute_units"] = torch.cuda.get_device_properties(0).multi_processor_count
    for e in ev:
        hip.hipEventDestroy(e)
    store.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
