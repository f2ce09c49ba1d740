#!/usr/bin/env python3
"""The sliding-window local mapper per sweep, against what a user could compose before it existed.

    python tools/bench_local_mapping.py [--sweeps 100] [--warmup 10] [--windows 30,120] [--step 0.4] [--out FILE]

Workload: a seeded synthetic drive along a street of synth's Manhattan world, VLP-16 (16 x 1800) features, `--step` metres per
sweep, measured at two steady-state windows (queue_distance 30 m = 75 frames, 120 m = 300 frames).  Four variants take the
same sweeps in turn -- sweep k through each of them before sweep k + 1, each on a context of its own:

  1. LaserMappingLocal.process, key-ordered window (LSLAM_LMAP_KEY_ORDERED)
  2. LaserMappingLocal.process, full re-filter (LSLAM_LMAP_REFILTER)
  3. the composed baseline: frames kept on the host, np.concatenate, voxel_grid twice, ctx.map_set, ctx.scanmatch_scan
  4. LaserMapping.process (the cube map) on the same drive, for scale

Per variant: median and p99 of the wall clock per call and of the device span (HIP events on the context's stream around the
call) over `--sweeps` sweeps after the window is full and `--warmup` more have passed.  The three local variants must return
identical poses, bit for bit, on every sweep of the run: the tool exits non-zero otherwise.

    --count-launches VARIANT   only that variant (1, 2 or 4), window 30 m, to be run under `rocprofv3 --kernel-trace --stats`
                               with two values of --sweeps: the difference of the dispatch counts is the launches per sweep
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

REFILTER, KEY_ORDERED = 1, 2


def transform_cloud(T, c):
    """p' = R p + t in float32 in the device kernel's operation order (elementwise numpy does not fuse)."""
    out = c.copy()
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


class Composed:
    """The parent commit's public API only: host-side frames (FrameUpdater and clean() in float64), np.concatenate, two
    voxel_grid calls, map_set, scanmatch_scan."""

    def __init__(self, pkg, ctx, queue_distance):
        self.pkg, self.ctx, self.qd = pkg, ctx, queue_distance
        ctx.defer_trees(True)
        self.queue, self.accum, self.prev = [], 0.0, None
        self.opts = ctx.default_opts()
        self.opts.delta_t_abort = self.opts.delta_r_abort = 0.1
        self.opts.use_score = 0
        self.odom_last = np.eye(4, dtype=np.float32)
        self.mapped_last = np.eye(4, dtype=np.float32)
        self.feature_map = None

    def process(self, corner_last, surf_last, odom_new):
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        out = np.zeros(16, np.float32)
        a, b, c = (np.ascontiguousarray(m, np.float32).reshape(16) for m in (self.odom_last, odom_new, self.mapped_last))
        self.ctx.lib.lslam_transform_associate(fp(a), fp(b), fp(c), fp(out))
        new = out.reshape(4, 4).copy()
        cds, sds = self.pkg.voxel_grid2(self.ctx, corner_last, surf_last, 1.0)
        if self.queue:
            mc = self.pkg.voxel_grid(self.ctx, np.concatenate([f[0] for f in self.queue]), 0.2)
            ms = self.pkg.voxel_grid(self.ctx, np.concatenate([f[1] for f in self.queue]), 0.4)
            self.ctx.map_set(mc, ms)
            status, pose, st = self.ctx.scanmatch_scan(cds, sds, self.ctx.isometry_to_pose(new), self.opts)
            if int(status) != 1:
                new = self.ctx.pose_to_isometry(pose)
        self.mapped_last, self.odom_last = new.copy(), np.array(odom_new, np.float32)
        P = new.astype(np.float64)
        if self.prev is not None:
            Q, d = self.prev, np.zeros(3)
            for k in range(3):
                u = (Q[0, k] * P[0, 3] + Q[1, k] * P[1, 3]) + Q[2, k] * P[2, 3]
                v = (Q[0, k] * Q[0, 3] + Q[1, k] * Q[1, 3]) + Q[2, k] * Q[2, 3]
                d[k] = u + (-v)
            self.accum += float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        self.prev = P
        self.queue.append((transform_cloud(new, cds), transform_cloud(new, sds), self.accum))
        n = 0
        for f in self.queue:
            if f[2] > self.accum - self.qd:
                break
            n += 1
        if n:
            del self.queue[:n + 1]
        return new


class StreamTimer:
    """HIP events on a context's stream (the runtime the product library is linked against, reached through the library)."""

    def __init__(self, pkg, ctx):
        self.hip = C.CDLL(pkg.lib_path())
        self.stream = C.c_void_p(ctx.lib.lslam_stream(ctx.h))
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            if self.hip.hipEventCreate(C.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def start(self):
        self.hip.hipEventRecord(self.e0, self.stream)

    def stop_ms(self):
        self.hip.hipEventRecord(self.e1, self.stream)
        self.hip.hipEventSynchronize(self.e1)
        ms = C.c_float()
        self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1)
        return ms.value


def make_drive(synth, n, step):
    """n sweeps along the street x = 157 of the Manhattan world: features and a drifting odometry."""
    import synth_gpu
    world = synth.World(half_extent=300.0, wall_half=295.0, pole_pitch=2.5)
    lidar = synth_gpu.GpuLidar(world, 0)
    sweeps = []
    for k in range(n):
        gt = np.array([0.0, 0.0, np.pi / 2 + 0.01 * np.sin(0.05 * k), 157.0 + 0.2 * np.sin(0.03 * k), -140.0 + step * k, 1.8])
        c, s = lidar.scan(gt, 16, 1800, seed=5000 + k)
        R, t = synth.pose_to_Rt(gt)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        Rd, td = synth.pose_to_Rt(np.array([0.0, 0.0, 0.0003 * k, 0.004 * k, -0.002 * k, 0.0]))
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = Rd, td
        sweeps.append((np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32), (T @ D).astype(np.float32)))
    return sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", default="30,120")
    ap.add_argument("--step", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--count-launches", type=int, default=0)
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    windows = [30.0] if args.count_launches else [float(w) for w in args.windows.split(",")]
    fills = [int(np.ceil(w / args.step)) + 2 for w in windows]
    drive = make_drive(synth, max(fills) + args.warmup + args.sweeps, args.step)
    lines, results, ok = [], [], True
    lines.append("# python tools/bench_local_mapping.py --sweeps %d --warmup %d --windows %s --step %g"
                 % (args.sweeps, args.warmup, args.windows, args.step))
    lines.append("# per sweep: %d corner / %d surf features (median), 16 x 1800" % (np.median([len(d[0]) for d in drive]),
                                                                                    np.median([len(d[1]) for d in drive])))
    for qd, fill in zip(windows, fills):
        n_total = fill + args.warmup + args.sweeps
        names = {1: "LaserMappingLocal key-ordered", 2: "LaserMappingLocal re-filter", 3: "composed baseline (host frames)",
                 4: "LaserMapping (cube map)"}
        which = [args.count_launches] if args.count_launches else [1, 2, 3, 4]
        ctxs = {v: pkg.Context(0) for v in which}
        nodes = {}
        for v in which:
            if v == 1:
                nodes[v] = pkg.LaserMappingLocal(ctxs[v], queue_distance=qd, max_points=1 << 21, mode=KEY_ORDERED)
            elif v == 2:
                nodes[v] = pkg.LaserMappingLocal(ctxs[v], queue_distance=qd, max_points=1 << 21, mode=REFILTER)
            elif v == 3:
                nodes[v] = Composed(pkg, ctxs[v], qd)
            else:
                nodes[v] = pkg.LaserMapping(ctxs[v], cube_dims=(21, 21, 11), map_filter_corner=0.2, map_filter_surf=0.4, map_filter=0.6)
        timers = {v: StreamTimer(pkg, ctxs[v]) for v in which}
        wall = {v: [] for v in which}
        dev = {v: [] for v in which}
        iters = {v: [] for v in which}
        mismatches = 0
        for k in range(n_total):
            c, s, odom = drive[k]
            poses = {}
            for v in which:
                timers[v].start()
                t0 = time.perf_counter()
                poses[v] = nodes[v].process(c, s, odom)
                t1 = time.perf_counter()
                d_ms = timers[v].stop_ms()
                if k >= fill + args.warmup:
                    wall[v].append(1e3 * (t1 - t0))
                    dev[v].append(d_ms)
                    st = getattr(nodes[v], "last_stats", None)
                    iters[v].append(st.iterations if st is not None else -1)
            local = [poses[v].view(np.uint32) for v in which if v in (1, 2, 3)]
            for p in local[1:]:
                if not np.array_equal(local[0], p):
                    mismatches += 1
        info = nodes[which[0]].feature_map.info() if which[0] in (1, 2) else {}
        lines.append("")
        lines.append("window: queue_distance %.0f m at %.2f m per sweep -> %s frames, %s corner / %s surf points live; %d sweeps timed after %d"
                     % (qd, args.step, info.get("n_frames", "?"), info.get("n_corner", "?"), info.get("n_surf", "?"), args.sweeps,
                        fill + args.warmup))
        lines.append("%-34s %10s %10s %12s %12s %6s" % ("variant", "wall med", "wall p99", "device med", "device p99", "GN it"))
        for v in which:
            w, d = np.asarray(wall[v]), np.asarray(dev[v])
            lines.append("%-34s %7.3f ms %7.3f ms %9.3f ms %9.3f ms %6.1f"
                         % (names[v], np.median(w), np.percentile(w, 99), np.median(d), np.percentile(d, 99), np.mean(iters[v])))
            results.append(dict(window_m=qd, variant=names[v], wall_ms_median=float(np.median(w)), wall_ms_p99=float(np.percentile(w, 99)),
                                device_ms_median=float(np.median(d)), device_ms_p99=float(np.percentile(d, 99))))
        if 1 in nodes:
            lines.append("key-ordered window: (merged, resorted, re-filtered) per type and sweep so far = %s" % (nodes[1].feature_map.stats(),))
        if len(which) > 1:
            lines.append("poses of the three local variants: %s over %d sweeps" % ("identical, bit for bit" if not mismatches else
                                                                                  "%d sweeps DIFFER" % mismatches, n_total))
            ok = ok and mismatches == 0
        k_last = n_total - 1
        gt_last = np.array([157.0 + 0.2 * np.sin(0.03 * k_last), -140.0 + args.step * k_last, 1.8])
        err = float(np.abs(poses[which[0]][:3, 3] - gt_last).max())
        lines.append("last map pose against the drive's: %.3f m" % err)
        for v in which:
            if hasattr(nodes[v].feature_map, "close"):
                nodes[v].feature_map.close()
            ctxs[v].close()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="bench_local_mapping", poses_identical=bool(ok), results=results)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
