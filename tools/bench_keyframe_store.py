#!/usr/bin/env python3
"""A/B of the pose-graph node's two cloud-heavy steps with the keyframes' clouds on the host (A: today's path) and in the
keyframe store (B: lslam_kfs_*), on the same keyframes, through the C ABI with every buffer made once:

  * Graph::getFinalFeatureMap over the keyframes of bench.py's final_feature_map leg (300 keyframes, 16 x 1800 sweeps, 0.26 m
    apart, cube grid 21 x 21 x 11, with the bootstrap): per keyframe update -> surround counts -> VoxelGrid 0.2 / 0.3 ->
    surround to map -> scan match -> addFeatureCloud;
  * 50 LoopDetector::matching_nearest calls: two candidates, a new keyframe beside them, a perturbed guess -- candidates'
    clouds assembled, ICP, VoxelGrid x 4, full scan match.

A and B alternate, after a warm-up pass of each; times are host clocks around calls that end in a device wait.  Prints ms per
keyframe and per loop match for both (median and spread over the repeats) and the store's two byte counters, and exits
non-zero unless A and B agree in every bit of the poses, the flags and the final map.

    python tools/bench_keyframe_store.py [--keyframes 300] [--loops 50] [--repeats 5] [--device 0]
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=300)
    ap.add_argument("--loops", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    capi = importlib.import_module("the-cooper-mapper_amd.capi")
    lc = importlib.import_module("the-cooper-mapper_amd.loop_closure")
    import synth_gpu
    ctx = pkg.Context(args.device)  # raises without a GPU: nothing here falls back
    lib = ctx.lib
    fp = lambda a: a.ctypes.data_as(capi.c_float_p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def check(rc):
        if rc < 0:
            raise pkg.LslamError(rc, lib.lslam_last_error().decode())
        return rc

    # ---- the keyframes of bench.py's final_feature_map leg ------------------------------------------------------------------
    world = synth.World(half_extent=300.0, wall_half=295.0, pole_pitch=2.5)
    lidar = synth_gpu.GpuLidar(world, args.device)
    traj = synth_gpu.loop_trajectory(5000)
    rng = np.random.default_rng(77)
    n_kf = args.keyframes
    clouds, ests = [], []
    for k in range(n_kf):
        c, s = lidar.scan(traj[k], 16, 1800, seed=555000 + k)
        est = ctx.pose_to_isometry(traj[k].astype(np.float32)).astype(np.float64)
        est[:3, 3] += rng.normal(0.0, 0.02, 3)
        clouds.append((np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32)))
        ests.append(est)
    store = pkg.KeyframeStore(ctx)
    t0 = time.perf_counter()
    ids = [store.add(c, s) for c, s in clouds]
    t_upload = time.perf_counter() - t0
    up_once = store.info()["cloud_bytes_uploaded"]
    n_max = max(max(len(c), len(s)) for c, s in clouds)
    fc, fs = np.zeros((n_max, 4), np.float32), np.zeros((n_max, 4), np.float32)  # the filtered clouds' buffers, made once
    opts = ctx.default_opts()

    def final_map(resident):
        """-> (seconds, matched flags, poses (n, 16) float32, full map)"""
        h = C.c_void_p()
        check(lib.lslam_fmap_create(ctx.h, 21, 21, 11, C.byref(h)))
        check(lib.lslam_fmap_setup_filter_size(h, 0.2, 0.2, 0.4))
        matched, poses = np.zeros(n_kf, np.int32), np.zeros((n_kf, 16), np.float32)
        nc, ns, mc, ms = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        pose, st = np.zeros(6, np.float32), pkg.LslamStats()
        t0 = time.perf_counter()
        for k in range(n_kf):
            c, s = clouds[k]
            T = ests[k].astype(np.float32).reshape(16)
            pos = np.array([T[3], T[7], T[11]], np.float32)
            check(lib.lslam_fmap_update(h, fp(pos)))
            check(lib.lslam_fmap_surround_counts(h, C.byref(nc), C.byref(ns)))
            if not resident:
                check(lib.lslam_voxel_grid(ctx.h, vp(c), len(c), 16, 0.2, fp(fc), len(c), C.byref(mc)))
                check(lib.lslam_voxel_grid(ctx.h, vp(s), len(s), 16, 0.3, fp(fs), len(s), C.byref(ms)))
            enough = nc.value >= 50 and ns.value >= 100
            ok = False
            if enough:
                check(lib.lslam_fmap_surround_to_map(h))
                lib.lslam_isometry_to_pose(fp(T), fp(pose))
                if resident:
                    rc = check(lib.lslam_kfs_scanmatch(store.h, ids[k], 0.2, 0.3, fp(pose), C.byref(opts), C.byref(st)))
                else:
                    rc = check(lib.lslam_scanmatch_scan(ctx.h, vp(fc), mc.value, vp(fs), ms.value, 16, fp(pose), C.byref(opts), C.byref(st)))
                if rc != 1:
                    lib.lslam_pose_to_isometry(fp(pose), fp(T))
                ok = rc == 0
            if ok or not enough:
                if resident:
                    check(lib.lslam_kfs_add_to_fmap(store.h, ids[k], h, fp(T)))
                else:
                    check(lib.lslam_fmap_add_feature_cloud(h, vp(c), len(c), vp(s), len(s), 16, fp(T)))
            matched[k] = ok
            poses[k] = T
        dt = time.perf_counter() - t0
        n = C.c_size_t()
        check(lib.lslam_fmap_get_full_map(h, None, 0, C.byref(n)))
        full = np.zeros((n.value, 4), np.float32)
        check(lib.lslam_fmap_get_full_map(h, fp(full), n.value, C.byref(n)))
        lib.lslam_fmap_destroy(h)
        return dt, matched, poses, full

    # ---- the loop matches ---------------------------------------------------------------------------------------------------
    n_loops = min(args.loops, n_kf - 3)
    step = max(1, (n_kf - 3) // n_loops)
    sets = []
    for j in range(n_loops):
        a = j * step
        inv = np.linalg.inv(ests[a])
        rel = np.stack([np.eye(4, dtype=np.float32), (inv @ ests[a + 1]).astype(np.float32)])
        g = ests[a + 2].copy()
        g[:3, 3] += rng.normal(0.0, 0.1, 3)
        sets.append(([a, a + 1], rel, a + 2, (inv @ g).astype(np.float32)))
    ds = [np.zeros((2 * n_max, 4), np.float32) for _ in range(4)]

    def loop_matches(resident):
        """-> (seconds, stages, guesses (n, 16))"""
        stages, guesses = np.zeros(n_loops, np.int32), np.zeros((n_loops, 16), np.float32)
        stage, its, fit, conv, st = C.c_int32(), C.c_int32(), C.c_double(), C.c_int32(), pkg.LslamStats()
        pose = np.zeros(6, np.float32)
        t0 = time.perf_counter()
        for j, (cand, rel, new, guess) in enumerate(sets):
            g = guess.reshape(16).copy()
            if resident:
                cid = np.array([ids[c] for c in cand], np.int32)
                check(lib.lslam_kfs_loop_match(store.h, len(cid), cid.ctypes.data_as(capi.c_int32_p), fp(rel.reshape(-1)), ids[new], fp(g), 10,
                                               C.byref(opts), C.byref(stage), C.byref(fit), C.byref(its), C.byref(st)))
                stages[j] = stage.value
            else:  # LoopDetector.matching_nearest's calls
                corner = np.concatenate([clouds[cand[0]][0]] + [lc.transform_cloud(clouds[c][0], rel[i]) for i, c in enumerate(cand) if i])
                surf = np.concatenate([clouds[cand[0]][1]] + [lc.transform_cloud(clouds[c][1], rel[i]) for i, c in enumerate(cand) if i])
                nc_, ns_ = clouds[new]
                sg = 0
                if len(surf):
                    check(lib.lslam_icp_align(ctx.h, vp(surf), len(surf), vp(ns_), len(ns_), 16, fp(g), 10, 0.0, 0.0, C.byref(fit),
                                              C.byref(conv), C.byref(its)))
                    sg = 1
                    if conv.value:
                        m = []
                        for buf, (a, leaf) in zip(ds, ((corner, 0.2), (surf, 0.4), (nc_, 0.2), (ns_, 0.4))):
                            n = C.c_size_t()
                            check(lib.lslam_voxel_grid(ctx.h, vp(a), len(a), 16, leaf, fp(buf), len(a), C.byref(n)))
                            m.append(n.value)
                        lib.lslam_isometry_to_pose(fp(g), fp(pose))
                        rc = check(lib.lslam_scanmatch_full(ctx.h, vp(ds[0]), m[0], vp(ds[1]), m[1], 16, vp(ds[2]), m[2], vp(ds[3]), m[3], 16,
                                                            fp(pose), C.byref(opts), C.byref(st)))
                        lib.lslam_pose_to_isometry(fp(pose), fp(g))
                        sg = 3 if rc == 0 else 2
                stages[j] = sg
            guesses[j] = g
        return time.perf_counter() - t0, stages, guesses

    # ---- warm-up, then A and B alternating -----------------------------------------------------------------------------------
    import gc
    ref = {}
    for resident in (False, True):
        ref["final", resident] = final_map(resident)
        ref["loop", resident] = loop_matches(resident)
    up0, down0 = store.info()["cloud_bytes_uploaded"], store.info()["cloud_bytes_downloaded"]
    times = {("final", False): [], ("final", True): [], ("loop", False): [], ("loop", True): []}
    agree = True
    for _ in range(args.repeats):
        for resident in (False, True):
            gc.collect()
            for what, fn in (("final", final_map), ("loop", loop_matches)):
                r = fn(resident)
                times[what, resident].append(r[0])
                base = ref[what, False]
                for got, want in zip(r[1:], base[1:]):
                    agree = agree and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    info = store.info()
    ms = lambda v, n: 1e3 * np.array(v) / n
    print("keyframe store A/B: %d keyframes of 16 x 1800 (%.0f points each on average), %d loop matches, %d repeats after a warm-up of each"
          % (n_kf, np.mean([len(c) + len(s) for c, s in clouds]), n_loops, args.repeats))
    print("%-34s %12s %12s %12s" % ("", "median", "min", "max"))
    for what, n, unit in (("final", n_kf, "ms per keyframe"), ("loop", n_loops, "ms per loop match")):
        for resident, name in ((False, "A host clouds"), (True, "B keyframe store")):
            t = ms(times[what, resident], n)
            print("%-34s %12.4f %12.4f %12.4f" % ("%s, %s" % (unit, name), np.median(t), t.min(), t.max()))
    print("matched %d of %d keyframes; loop stages %s" % (int(ref["final", False][1].sum()), n_kf, np.bincount(ref["loop", False][1], minlength=4).tolist()))
    print("store: upload of all keyframes once %.1f ms (%d bytes); cloud_bytes_uploaded during the timed passes %d, cloud_bytes_downloaded %d"
          % (1e3 * t_upload, up_once, info["cloud_bytes_uploaded"] - up0, info["cloud_bytes_downloaded"] - down0))
    print("A and B agree in every bit of poses, flags, guesses and the final map: %s" % ("yes" if agree else "NO"))
    store.close()
    ctx.close()
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
