#!/usr/bin/env python3
"""bench.py -- point-residuals/s of the L_SLAM scan-to-map Gauss-Newton hot path on MI355X.

Workload (BASELINE.json configs[2] on the map of configs[1])
  * world: 600 x 600 m Manhattan grid (ground, box buildings, street poles, perimeter wall);
  * map: the "10k-frame voxel map" -- `--map-frames` (10 000) VLP-16 frames ray cast along a closed loop
    through the streets, each filtered and pushed at its ground-truth pose through
    FeatureMap::addFeatureCloud (util/FeatureMap.h:219-230,289-306; corner leaf 0.2 m, surf 0.4 m) on the
    device map; what is matched against is the active surround at the end of the loop
    (getSurroundFeature, :256-265), kd-trees built on the device;
  * queries: `--scans` (960) different synthetic 64-ring x 1800 scans (115 200 points each, every
    return a query) taken around the end of the loop, initial pose error +-0.3 m / +-2 deg.
A "step" is one pass of the hot path over that batch: the scanMatchScan Gauss-Newton loop
(ScanMatch.cpp:78-347: <= 10 iterations of transform -> kd-tree 5-NN -> line/plane fit -> residual +
Jacobian -> J^T J / J^T r -> 6x6 solve -> pose update) of every resident scan, `--batch` scans in
flight per launch sequence -- the way every keyframe is re-matched against the map in
pose_graph/graph.cpp:171-197.  Every call starts cold (no neighbour lists carried over).
Map, kd-trees and scans are resident in HBM before the timed region starts.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line (`--dump-outputs DIR`: and writes what the last timed step
returned as DIR/<name>.npy).  Everything else -- the same steps through the other search modes, the grid sweep's tally step,
the secondary legs, the CPU baseline and its parity check, the RCCL check -- runs with `--full` only.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment makes THIS process start N ranks
(python -m torch.distributed.run, one per GPU) before it touches the GPU, and relay rank 0's line; under
a launcher (WORLD_SIZE set) the rank count must equal --gpus.  The map is replicated, every rank matches
its own scans (independent problems, no data-path collective: SURVEY.md 8e row 2), `value` is the
whole-job aggregate.

The LAST stdout line (rank 0) is one compact JSON object (< 6 KB: the contract's keys and `roofline`; with `--full` also
`cpu_baseline` and one number per secondary leg that ran); the full report goes to bench_report.json and, as one line, to stderr.  `roofline` prices the
sweep's dominant kernel -- SURVEY.md 8d's algorithmic flops (and, beside them, bytes) per point-residual over its average
duration, measured with HIP events on the library's own stream inside the timed region -- next to what the committed
rocprofv3 counter passes of this same command say bounds it.  `cpu_baseline` (`--full`) is the oracle (a port of the reference's single-threaded CPU path,
including its per-call kd-tree rebuild) timed on this host on a sample of the same workload.
"""
import argparse
import importlib
import json
import os
import re
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ALG_BYTES_PER_POINT_RESIDUAL = 1700.0  # working set of nanoflann's unbounded search on the surveyed map
# What a bounded sweep of THIS workload touches per point (tools/traversal_stats.py on the bench map):
# 24.6 inner nodes x 16 B + 3.4 re-read parents x 16 B + 4.4 leaves x 10 slots x 16 B + the five previous
# neighbours (20 B of indices + 5 x 16 B of points) + the query (16 B) + what is written (20 B of indices, 36 B of
# per-block partial sums amortised to < 1 B) = 1.30 KB
ALG_BYTES_PER_POINT_BOUNDED = 24.6 * 16 + 3.4 * 16 + 4.4 * 160 + 100 + 16 + 20
POSE_TOL_M, POSE_TOL_RAD = 1e-4, 1e-5  # BASELINE.json north_star: pose within 1e-4 m of the CPU reference (tests: 1e-5 rad)
FLOPS_PER_POINT_RESIDUAL = 1200.0      # ~1.2 kflop per point-residual (distances 0.35 k, fit 0.4 k, transform + Jacobian 0.15 k, ...)
FP32_PEAK_TFLOPS = 157.3               # MI355X_MICROARCH.md: vector fp32
PG_CPU_ITERS = 25                      # LM iterations the compiled CPU pose-graph baseline runs (~0.5 s each)
HBM_PEAK_GBS = 8000.0                  # MI355X_MICROARCH.md: 8 TB/s spec
L2_PEAK_GBS = 34500.0                  # MI355X_MICROARCH.md: ~34.5 TB/s aggregate


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--scans", type=int, default=int(os.environ.get("LSLAM_SCANS", "960")),
                    help="resident query scans per GPU; one step matches all of them")
    ap.add_argument("--batch", type=int, default=int(os.environ.get("LSLAM_BATCH", "960")),
                    help="scans in flight per launch sequence (lslam_opts.scans_in_flight)")
    ap.add_argument("--map-frames", type=int, default=10000, help="frames accumulated into the voxel map")
    ap.add_argument("--map-rings", type=int, default=16, help="rings of the frames the map is built from (VLP-16)")
    ap.add_argument("--map-cache", default=None,
                    help="profiling passes: file to keep the built surround map in (built and saved on the first run, loaded "
                         "afterwards: rocprofv3 --pmc serialises the ~200 k dispatches of the 10k-frame build otherwise)")
    ap.add_argument("--jtj-mode", type=int, default=int(os.environ.get("LSLAM_JTJ_MODE", "1")))
    ap.add_argument("--search", default=os.environ.get("LSLAM_BENCH_SEARCH", "auto"), choices=["auto", "lane", "grid"],
                    help="lslam_opts.search_mode of every leg: the library's choice, the kd-tree walk, or the cell-grid probe")
    ap.add_argument("--grid-cell", type=float, default=0.0, help="lslam_opts.grid_cell [m] (0: the library's default)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-joint-stereo", action="store_true")
    ap.add_argument("--no-pose-graph", action="store_true")
    ap.add_argument("--no-single", action="store_true", help="skip the single-scan latency leg")
    ap.add_argument("--no-vlp16", action="store_true", help="skip the 16-ring x 1800 throughput leg")
    ap.add_argument("--no-mapping-frame", action="store_true", help="skip the per-frame mapping pipeline leg")
    ap.add_argument("--no-pipeline", action="store_true", help="skip the whole-chain (registration..mapping) leg")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: the timed region, the grid sweep's tally step and the RCCL check only (the command the "
                         "profiling passes wrap); implied without --full")
    ap.add_argument("--shard-points", action="store_true",
                    help="run the sharded-points leg even on one GPU (RCCL all-reduce over a world of 1)")
    ap.add_argument("--leg-timeout", type=int, default=1500, help="seconds the legs after the headline may take in all")
    ap.add_argument("--pg-iters", type=int, default=1000, help="LM iteration limit of the pose-graph leg")
    ap.add_argument("--cpu-scans", type=int, default=48, help="scans the single-core CPU baseline matches")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the other search modes, the secondary legs, the CPU baseline and its "
                         "parity check, the grid sweep's tally step and the RCCL check (the --no-* options pick among them). "
                         "Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (poses and per-scan statistics) as DIR/<name>.npy")
    return ap.parse_args()


_REAL_STDOUT = None  # main() keeps the process's stdout here and points descriptor 1 at stderr


def spawn_ranks(n):
    """`python bench.py --gpus N` outside a launcher: start the N ranks ourselves.  This parent has not
    imported torch or touched HIP; it only relays the children's output and exit code."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def main():
    args = parse_args()
    if not args.full:  # a plain run: the timed region and its line only
        args.headline_only = True
    if args.headline_only:
        args.no_cpu_baseline = args.no_joint_stereo = args.no_pose_graph = args.no_single = args.no_vlp16 = True
        args.no_mapping_frame = args.no_pipeline = True
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        print("bench.py: --gpus %d but the launcher started %s rank(s)" % (args.gpus, os.environ.get("WORLD_SIZE")),
              file=sys.stderr)
        sys.exit(2)
    # stdout carries ONE line, the JSON object rank 0 prints last.  Native libraries print there too -- librccl a version banner
    # whenever a communicator is made (this process makes one in every run since round 6), through C stdio, flushed when the
    # process exits, i.e. BEHIND the line.  So descriptor 1 is pointed at stderr for the whole run and the line goes to the
    # descriptor stdout was, by emit().
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch

    distmod = importlib.import_module("the-cooper-mapper_amd.dist")
    rank, local_rank, world = distmod.env_rank()
    if os.environ.get("LSLAM_BENCH_DRY_RUN"):  # launcher test (tests/test_dist_cpu.py): rendezvous only, no GPU
        dist = distmod.init("gloo")
        (n,), _ = distmod.aggregate(dist, [1.0], 0.0)
        per_rank = gather_per_rank(distmod, dist, rank, world, 1.0e9 * (rank + 1))
        if rank == 0:
            # the same emit() as a real run, on a report of the real run's shape (every leg present, long strings and all):
            # tests/test_dist_cpu.py holds the last stdout line to the driver's 8 KB tail
            out = dry_run_report(world, int(n), per_rank)
            emit(out)
        if dist is not None:
            dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP backend has no CPU fallback")
    dist = distmod.init("nccl")

    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import synth_gpu

    # ---- the world, the 10k-frame voxel map and the query scans -------------------------------------
    t_setup = time.perf_counter()
    world_model = synth.World(half_extent=300.0, wall_half=295.0, pole_pitch=2.5)  # poles / trunks every 2.5 m along the streets: ~10 % corner returns
    lidar = synth_gpu.GpuLidar(world_model, local_rank)
    traj = synth_gpu.loop_trajectory(args.map_frames)
    ctx = pkg.Context(local_rank)
    end_pose = traj[-1]
    cache = args.map_cache + (".rank%d.npz" % rank) if args.map_cache else None
    if cache and os.path.exists(cache):
        z = np.load(cache, allow_pickle=True)
        mapstats = dict(z["stats"].item(), loaded_from_cache=True)
        fm = pkg.FeatureMap(ctx, 21, 21, 11)
        fm.setup_filter_size(0.2, 0.4, 0.6)
        fm.update(end_pose[3:].astype(np.float32))
        fm.add_feature_cloud(z["corner"], z["surf"], np.eye(4, dtype=np.float32))  # already filtered: stays as it is
    else:
        fm, mapstats = synth_gpu.build_voxel_map(pkg, ctx, lidar, traj, rings=args.map_rings,
                                                 progress=2000 if rank == 0 else None)
        fm.update(end_pose[3:].astype(np.float32))
        if cache:
            sc, ss = fm.get_surround_feature()
            np.savez(cache, corner=sc, surf=ss, stats=np.array(mapstats, dtype=object))
    fm.surround_to_map()
    info = ctx.map_info()
    # query poses: on the loop within +-25 m of path around its end (the loop is closed), a little off the line
    rng = np.random.default_rng(4242 + rank)
    dense = synth_gpu.loop_trajectory(100000)
    per = 0.0
    seg = np.linalg.norm(np.diff(dense[:, 3:5], axis=0), axis=1).mean()
    span = int(25.0 / seg)
    scans, inits, gts = [], [], []
    for k in range(args.scans):
        g = dense[int(rng.integers(-span, span)) % len(dense)].copy()
        g[3:5] += rng.uniform(-1.0, 1.0, 2)
        g[2] += rng.uniform(-0.2, 0.2)
        qc, qs = lidar.scan(g, args.rings, 1800, seed=900000 + 1000 * rank + k)
        scans.append((qc, qs))
        gts.append(g.astype(np.float32))
        inits.append(synth.perturb_pose(g, seed=99 + 1000 * rank + k))
    n_pts = sum(len(c) + len(s) for c, s in scans)
    n_corner = sum(len(c) for c, _ in scans)
    ctx.scan_set_batch(scans)
    inits = np.stack(inits)
    gts = np.stack(gts)
    opts = ctx.default_opts()
    opts.jtj_mode = args.jtj_mode
    opts.profile = 1
    opts.scans_in_flight = args.batch
    opts.search_mode = {"auto": 0, "lane": 1, "grid": 3}[args.search]
    opts.grid_cell = args.grid_cell
    if os.environ.get("LSLAM_DEBUG_MAX_ITERS"):  # diagnostics only (tools/cert_stats.py): the loop cut short -- not a bench line
        opts.max_iterations = int(os.environ["LSLAM_DEBUG_MAX_ITERS"])
    setup_s = time.perf_counter() - t_setup
    # The interpreter holds ~170 k objects by now (torch, numpy): a generation-2 collection of the Python
    # garbage collector takes 25-35 ms and would land in whichever timed region happens to allocate the
    # triggering object.  Park everything allocated so far in the permanent generation (the same reason
    # timeit disables the collector); the library itself has no Python in its data path.
    quiet_gc()

    def barrier():
        distmod.barrier(dist)

    for _ in range(args.warmup):
        ctx.run_batch(inits, opts)
    # an experiment build with section clocks in the sweep kernel (-DLSLAM_EXP_SECTION_CLOCK, tools/section_clock.sh): counted over the timed steps
    section_clock = getattr(ctx.lib, "lslam_debug_section_clock", None) if hasattr(ctx.lib, "lslam_debug_section_clock") else None
    if section_clock is not None:
        import ctypes
        section_clock.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
        section_clock((ctypes.c_uint64 * 12)(), 1)

    barrier()
    t0 = time.perf_counter()
    pt_res = 0
    iters = 0
    sweep_ms = 0.0
    sweep_launches = 0
    loop_ms = 0.0
    last = None
    for _ in range(args.steps):
        status, poses, sts = ctx.run_batch(inits, opts)  # synchronises the library's stream
        pt_res += sum(s.point_residuals for s in sts)
        iters += sum(s.iterations for s in sts)
        sweep_ms += sts[0].gpu_ms_sweep
        sweep_launches += sts[0].sweep_launches
        loop_ms += sts[0].gpu_ms_total
        last = (status, poses, sts)
    barrier()
    elapsed = time.perf_counter() - t0

    (total_pt_res, total_iters), t = distmod.aggregate(dist, [pt_res, iters], elapsed)
    per_rank = gather_per_rank(distmod, dist, rank, world, pt_res / elapsed)
    if os.environ.get("LSLAM_DEBUG_CERT_STATS"):  # debug tap of the certificate path (read by lslam_ctx_create): searched / swept points
        import ctypes
        cs = (ctypes.c_uint64 * 3)()
        ctx.lib.lslam_debug_cert_stats(ctx.h, cs)
        print("certificate path: searched %d of %d points swept (%.1f %%)" % (cs[0], cs[1], 100.0 * cs[0] / max(1, cs[1])), file=sys.stderr)

    if hasattr(ctx.lib, "lslam_debug_pass2_hist"):  # (-DLSLAM_EXP_PASS2_CLASS builds: the second pass's searches by their starting bound)
        import ctypes
        h8 = (ctypes.c_uint64 * 8)()
        ctx.lib.lslam_debug_pass2_hist.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
        ctx.lib.lslam_debug_pass2_hist(h8, 1)
        print("pass-2 searches by starting bound (< 0.5, < 1, < 2, < 4.99 m^2, gate): %s" % [int(v) for v in h8[:5]], file=sys.stderr)
    section_ticks = None
    if section_clock is not None:
        sc_out = (ctypes.c_uint64 * 12)()
        section_clock(sc_out, 1)
        section_ticks = [int(v) for v in sc_out]

    status, poses, sts = last
    pose_err = np.abs(poses - gts)
    n_conv = int(sum(1 for s in sts if s.converged))

    out = None
    if rank == 0:
        roof = sweep_roofline(pt_res, sweep_ms, sweep_launches, float(info.n_corner + info.n_surf), grid=ctx.grid_launches() > 0)
        out = {
            "metric": "point-residuals/s",
            "value": total_pt_res / t,
            "unit": "point-residuals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * t / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "lm_iters_per_s": total_iters / t,
            "timed_region_s": t,
            "config": {
                "workload": "synthetic %d-ring x 1800 scan-to-map scanMatchScan GN loops (BASELINE configs[2]) against "
                            "the %d-frame voxel map of a 600 x 600 m world (configs[1]): %d scans per step and GPU"
                            % (args.rings, args.map_frames, args.scans),
                "scans_per_step_per_gpu": args.scans,
                "scans_in_flight_per_gpu": args.batch,
                "scan_points_per_step": n_pts,
                "scan_corner_share": n_corner / max(1, n_pts),
                "map": dict(mapstats, surround_corner=int(info.n_corner), surround_surf=int(info.n_surf),
                            kd_nodes=int(info.nodes_corner + info.nodes_surf),
                            kd_depth=int(max(info.depth_corner, info.depth_surf)),
                            tree_build_ms=float(info.build_ms + info.upload_ms), build_attempts=int(info.build_attempts)),
                "gn_iters_per_scan": iters / args.steps / args.scans,
                "sweep_launches_per_step": sweep_launches / args.steps,
                "jtj_mode": "mfma_f32_16x16x4" if args.jtj_mode == 1 else "valu_shuffle",
                "search": args.search + (" (cell %.2f m)" % args.grid_cell if args.search == "grid" and args.grid_cell > 0 else ""),
                "grid_sweep_launches": ctx.grid_launches(),
                "parallelism": "replicated map, scans sharded across %d GPU(s), no collective" % world,
                "setup_s_outside_timed_region": setup_s,
                "gpu_loop_ms_per_step": loop_ms / args.steps,
                "pose_err_vs_ground_truth_m": {"max": float(pose_err[:, 3:].max()), "median": float(np.median(pose_err[:, 3:].max(axis=1)))},
                # the bits of the last step's poses: two builds (or two runs) that print the same number computed the same poses
                "poses_crc32": "%08x" % (__import__("zlib").crc32(np.ascontiguousarray(poses, np.float32).tobytes()) & 0xFFFFFFFF),
                "pose_err_vs_ground_truth_rad": float(pose_err[:, :3].max()),
                "converged_scans": n_conv,
            },
            "roofline": roof,
            # what a multi-GPU run can be checked by: every rank's own rate over its own clock, and (filled in below, once the
            # library's communicator exists) the rank count RCCL itself reports
            "ranks": {"world": world, "per_rank_value": per_rank, "rccl_ranks": None},
        }
        if section_ticks is not None:
            names = ["block, state, point, transform, carried bound", "probe set-up (cell table loads, row table)", "candidate loop",
                     "survivors: exact distances, order, proof", "pass-2 list (workgroup barrier), carried state written",
                     "residual chain (neighbours fetched, fit, coefficient, Jacobian row)", "-", "wait for the workgroup's slowest wavefront",
                     "staging, MFMA contraction, record"]
            tot = float(sum(section_ticks[:9])) or 1.0
            out["section_clock"] = {"kernel": "sweep_grid_kernel (pass 1), one workgroup in sixteen reporting", "wavefronts": section_ticks[9],
                                    "ticks_per_wavefront": tot / max(1, section_ticks[9]),
                                    "candidates_per_point": section_ticks[10] / max(1, 64 * section_ticks[9]),
                                    "loop_rounds_per_wavefront": section_ticks[11] / max(1, 64 * section_ticks[9]),
                                    "loop_lane_use": section_ticks[10] / max(1, section_ticks[11]),
                                    "share": {names[i]: section_ticks[i] / tot for i in range(9) if i != 6}}
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, status, poses, sts, rank, world, np)
    if args.full and ctx.grid_launches() > 0:  # what share of the points the grid sweeps left to the tree search (one more step, counted; untimed)
        import ctypes
        opts.debug_stats = 1
        g0 = (ctypes.c_uint64 * 3)()
        g1 = (ctypes.c_uint64 * 3)()
        ctx.lib.lslam_debug_cert_stats(ctx.h, g0)
        b0 = ctx.grid_stats().astype(np.int64)
        ctx.run_batch(inits, opts)
        ctx.lib.lslam_debug_cert_stats(ctx.h, g1)
        by = ctx.grid_stats().astype(np.int64) - b0  # [type][sweep of the loop][listed, swept]
        opts.debug_stats = 0
        if rank == 0:
            out["grid_sweep"] = {"points_swept_per_step": int(g1[1] - g0[1]), "points_left_to_the_tree_search_per_step": int(g1[0] - g0[0]),
                                 "share_left_to_the_tree_search": (g1[0] - g0[0]) / max(1, g1[1] - g0[1]),
                                 "second_pass_launches_per_step": int(g1[2] - g0[2]),
                                 # the same share by feature type and by sweep of the Gauss-Newton loop (the last entry: that sweep and later ones)
                                 "share_by_type": {n: float(by[t, :, 0].sum() / max(1, by[t, :, 1].sum())) for t, n in ((0, "corner"), (1, "surf"))},
                                 "share_by_sweep": {n: [round(float(by[t, j, 0] / max(1, by[t, j, 1])), 4) for j in range(by.shape[1]) if by[t, j, 1] > 0]
                                                    for t, n in ((0, "corner"), (1, "surf"))},
                                 "points_by_sweep": [int(by[:, j, 1].sum()) for j in range(by.shape[1]) if by[:, j, 1].sum() > 0],
                                 "counted_by": "the second pass's planner from the lists' lengths (the sweep kernel runs the same code with the tap on)"}
    # ---- disclosure leg: the same steps through the library's other search paths.  The headline runs the library as shipped
    # (lslam_opts.search_mode AUTO: for a batch this size the grid sweep -- every point's five neighbours either PROVEN by a
    # 27-cell probe or searched in the kd-tree; no neighbour list is carried over without one or the other).  Beside it:
    # the kd-tree walk of every point (round 3's kernel) with its certificate sweep, and with every search executed.  Same
    # neighbours in all of them, hence the same residuals and poses up to summation order.
    if not args.headline_only:
        def timed_mode(search_mode, knn_cert, n0):
            o_s, o_c = opts.search_mode, opts.knn_cert
            opts.search_mode, opts.knn_cert = search_mode, knn_cert
            ctx.run_batch(inits, opts)
            barrier()
            t1 = time.perf_counter()
            pr0 = 0
            for _ in range(n0):
                st0, poses0, sts0 = ctx.run_batch(inits, opts)
                pr0 += sum(s.point_residuals for s in sts0)
            barrier()
            (tot0,), t0s = distmod.aggregate(dist, [pr0], time.perf_counter() - t1)
            opts.search_mode, opts.knn_cert = o_s, o_c
            return tot0 / t0s, poses0, sts0
        n0 = max(3, args.steps // 4)
        shipped_is_grid = args.search in ("auto", "grid") and ctx.grid_launches() > 0
        v_every, poses0, sts0 = timed_mode(opts.search_mode, 0, n0)      # the shipped search, certificates off (a no-op for the grid sweep)
        v_lane_cert, poses_l, sts_l = timed_mode(1, 1, n0)                # kd-tree walk + certificate sweep
        v_lane_every, poses_e, sts_e = timed_mode(1, 0, n0)               # kd-tree walk, every search executed
        if rank == 0:
            status, poses, sts = last
            out["certificate_sweep"] = {
                "what": "value = the library as shipped (%s); value_searching_every_point = the same search with lslam_opts.knn_cert = 0 "
                        "(no neighbour list carried over by certificate); kd_tree_walk = LSLAM_SEARCH_LANE, round 3's kernel, with its "
                        "certificate sweep and with every search executed" % ("the grid sweep: probe + proof, kd-tree search for the rest" if shipped_is_grid else "kd-tree walk + certificate sweep"),
                "value_searching_every_point": v_every, "steps_per_mode": n0,
                "kd_tree_walk": {"value": v_lane_cert, "value_searching_every_point": v_lane_every},
                "pose_diff_between_the_two_modes_m": float(max(np.abs(poses[:, 3:] - poses_e[:, 3:]).max(), np.abs(poses_l[:, 3:] - poses_e[:, 3:]).max())),
                "pose_diff_between_the_two_modes_rad": float(max(np.abs(poses[:, :3] - poses_e[:, :3]).max(), np.abs(poses_l[:, :3] - poses_e[:, :3]).max())),
                "iterations_equal": bool(all(a.iterations == b.iterations == c.iterations for a, b, c in zip(sts, sts_l, sts_e))),
                # match counts of the last sweep: equal up to a handful of threshold-adjacent points (the modes group their sums
                # differently, so their poses differ in the last bits from the second iteration on)
                "rows_equal": bool(all(abs(int(x) - int(y)) <= max(2, int(1e-4 * max(x, y)))
                                       for a, b, c in zip(sts, sts_l, sts_e)
                                       for x, y in ((a.n_rows, c.n_rows), (b.n_rows, c.n_rows), (a.n_line, c.n_line), (a.n_plane, c.n_plane)))),
            }
    if rank == 0 and not args.no_single:  # (replaces the resident scans: after every leg that runs the step's batch)
        out["single_scan"] = single_scan_leg(ctx, scans[0], inits[0], opts, 200)
    # ---- the same timed region on 16-ring x 1800 scans (VLP-16, MultiScanRegistration.h:90-92; BASELINE north star:
    # "throughput on synthetic 16- and 64-ring scans") -- every rank, same protocol, its own roofline object
    if not args.no_vlp16:
        try:
            v16 = vlp16_throughput_leg(ctx, lidar, synth, dense, span, rank, world, args, opts, distmod, dist, info, np)
        except Exception as e:  # never takes the headline line down
            v16 = {"error": repr(e)}
        if rank == 0:
            out["vlp16_throughput"] = v16
    # From here on the legs are secondary (and, with N > 1, use the library's own RCCL communicator, which no
    # builder-side run could exercise on more than one GPU): a leg that hangs must not cost the headline line.
    # Every rank arms a watchdog; if it fires, rank 0 prints the line it has and all ranks leave.
    import threading

    def give_up():
        if rank == 0 and out is not None:
            out["aborted_secondary_legs"] = "watchdog: a leg after the headline did not finish within %d s" % args.leg_timeout
            emit(out)
        os._exit(0 if rank != 0 or out is not None else 3)

    watchdog = threading.Timer(args.leg_timeout, give_up)
    watchdog.daemon = True
    watchdog.start()
    surround = None
    if rank == 0 and not (args.no_cpu_baseline and args.no_mapping_frame):
        surround = fm.get_surround_feature()  # the map the timed region matched against, on the host
    parity_failed = None
    if rank == 0 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cb = cpu_baseline(surround, scans, inits, poses, sts, min(args.cpu_scans, args.scans), np)
        # The timed kernel against the oracle on this run's own scans: a headline whose poses differ from the CPU
        # path's is not a result.  The line is still printed (with the failure in it) and the run exits non-zero.
        cb["pose_tolerance"] = {"m": POSE_TOL_M, "rad": POSE_TOL_RAD}
        if not (cb["pose_diff_gpu_vs_cpu_m"] <= POSE_TOL_M and cb["pose_diff_gpu_vs_cpu_rad"] <= POSE_TOL_RAD
                and cb["iterations_equal"] and cb["rows_equal"]):
            parity_failed = ("GPU and CPU-oracle results differ on the sampled scans: %.3g m, %.3g rad (bars %.0e m, %.0e rad), "
                             "iteration counts equal: %s, row counts equal: %s"
                             % (cb["pose_diff_gpu_vs_cpu_m"], cb["pose_diff_gpu_vs_cpu_rad"], POSE_TOL_M, POSE_TOL_RAD,
                                cb["iterations_equal"], cb["rows_equal"]))
            out["parity_failed"] = parity_failed
    if rank == 0 and not args.no_mapping_frame:
        try:
            out["mapping_frame"] = mapping_frame_leg(pkg, synth, ctx, surround, lidar, end_pose, opts, np, not args.no_cpu_baseline, 64)
            # BASELINE configs[1]: the same frame with a VLP-16 (16 x 1800) sweep
            out["mapping_frame_vlp16"] = mapping_frame_leg(pkg, synth, ctx, surround, lidar, end_pose, opts, np, not args.no_cpu_baseline, 16)
            out["mapping_frame_cubes"] = mapping_frame_leg(pkg, synth, ctx, surround, lidar, end_pose, opts, np, False, 64, cubes=True)
        except Exception as e:  # a secondary leg never takes the headline line down
            out["mapping_frame"] = {"error": repr(e)}
    fm.close()
    if rank == 0 and not args.no_pipeline:
        try:
            out["sweep_pipeline"] = {"vlp16": sweep_pipeline_leg(pkg, synth, ctx, 16, np),
                                     "rings64": sweep_pipeline_leg(pkg, synth, ctx, 64, np)}
        except Exception as e:
            out["sweep_pipeline"] = {"error": repr(e)}
    if rank == 0 and not args.no_pipeline:
        try:
            out["final_feature_map"] = final_feature_map_leg(pkg, synth, synth_gpu, lidar, local_rank, np)
        except Exception as e:
            out["final_feature_map"] = {"error": repr(e)}
    comm = None
    if args.full and world == 1 and not args.shard_points and rank == 0:
        # a world of one: the line still says that librccl loads on this box and that the library's communicator answers
        # (ncclCommCount), with the version it found -- no collective is on the data path at N = 1
        try:
            c1 = make_comm(pkg, None, torch, 0, local_rank, 1)
            out["ranks"]["rccl_ranks"] = c1.info()[1]
            out["ranks"]["rccl_version"] = pkg.Comm.version()
            c1.close()
        except Exception as e:
            out["ranks"]["rccl_error"] = repr(e)[:200]
    if (world > 1 or args.shard_points) and not args.headline_only:
        try:
            comm = make_comm(pkg, dist, torch, rank, local_rank, world)
            ok = 1.0
        except Exception as e:
            comm, ok = None, 0.0
            print("bench.py: rank %d could not create the RCCL communicator: %r" % (rank, e), file=sys.stderr)
        (n_ok,), _ = distmod.aggregate(dist, [ok], 0.0)  # all ranks or none
        if rank == 0 and comm is not None:
            out["ranks"]["rccl_ranks"] = comm.info()[1]  # ncclCommCount of the library's own communicator
            out["ranks"]["rccl_version"] = pkg.Comm.version()
            out["ranks"]["rccl_allreduce_bytes"] = {"sharded_points_per_gn_iteration": 256, "pose_graph_per_linearisation": None}
        if int(round(n_ok)) != world:
            comm = None
            if rank == 0:
                out["sharded_points"] = {"error": "RCCL communicator not available on every rank (%d of %d)" % (int(round(n_ok)), world)}
    if comm is not None:
        try:
            shres = sharded_points_leg(pkg, synth, distmod, dist, rank, world, ctx, comm, opts, np, args)
        except Exception as e:  # never let the secondary leg take the headline line down
            shres = {"error": repr(e)}
        if rank == 0:
            out["sharded_points"] = shres
    if not args.no_joint_stereo:
        try:
            jres = joint_stereo_leg(pkg, synth, distmod, dist, rank, world, ctx, comm, opts, np, args,
                                    not args.no_cpu_baseline)
        except Exception as e:
            jres = {"error": repr(e)}
        if rank == 0:
            out["joint_lidar_stereo"] = jres
    if not args.no_pose_graph:
        try:
            pgres = pose_graph_leg(pkg, synth, distmod, dist, rank, world, local_rank, comm, np,
                                   args.pg_iters, not args.no_cpu_baseline)
        except Exception as e:
            pgres = {"error": repr(e)}
        if rank == 0:
            out["pose_graph"] = pgres
            if isinstance(out["ranks"].get("rccl_allreduce_bytes"), dict):
                out["ranks"]["rccl_allreduce_bytes"]["pose_graph_per_linearisation"] = pgres.get("allreduce_bytes_per_linearisation")
    watchdog.cancel()
    if rank == 0:
        emit(out)

    if dist is not None:
        dist.barrier()
    ctx.close()
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.destroy_process_group()
    if parity_failed:
        print("bench.py: PARITY FAILURE: " + parity_failed, file=sys.stderr)
        sys.exit(4)


COMPACT_LIMIT = 6000   # bytes: the driver keeps an 8 KB tail of stdout; the LAST stdout line must fit in it whole


def _pick(d, *keys):
    """d[k0][k1]... or None: the compact line is built from whatever legs ran."""
    for k in keys:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def _r(x, digits=6):
    """floats to `digits` significant digits (the full-precision values are in the report file)."""
    if isinstance(x, float):
        return float("%.*g" % (digits, x))
    if isinstance(x, dict):
        return {k: _r(v, digits) for k, v in x.items() if v is not None or k in ("vs_baseline", "traffic", "rccl_ranks")}
    if isinstance(x, (list, tuple)):
        return [_r(v, digits) for v in x]
    return x


def compact_line(out):
    """The line the driver parses: the contract's keys, `roofline`, `cpu_baseline` and one number per secondary leg, built from
    the full report `out` (which goes to bench_report.json and to stderr).  Guaranteed shorter than COMPACT_LIMIT: optional
    blocks are dropped, last first, if a future leg grows it."""
    roof = out.get("roofline") or {}
    cb = out.get("cpu_baseline") or {}
    cfg = out.get("config") or {}
    c = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                 "scaling", "vs_baseline", "dtype", "data", "timed_region_s", "lm_iters_per_s")}
    for k in ("dry_run", "ranks_counted", "section_clock"):  # (section_clock: experiment builds only)
        if k in out:
            c[k] = out[k]
    c["config"] = {"workload": cfg.get("workload"), "scans_per_step_per_gpu": cfg.get("scans_per_step_per_gpu"),
                   "scan_points_per_step": cfg.get("scan_points_per_step"),
                   "map_frames": _pick(cfg, "map", "frames"), "map_corner": _pick(cfg, "map", "surround_corner"),
                   "map_surf": _pick(cfg, "map", "surround_surf"), "gn_iters_per_scan": cfg.get("gn_iters_per_scan"),
                   "search": cfg.get("search"), "parallelism": cfg.get("parallelism"),
                   "pose_err_vs_ground_truth_m": _pick(cfg, "pose_err_vs_ground_truth_m", "max"), "poses_crc32": cfg.get("poses_crc32"),
                   "converged_scans": cfg.get("converged_scans")}
    c["roofline"] = {"kernel": roof.get("kernel_short") or (roof.get("kernel") or "")[:120], "bound": roof.get("bound"),
                     "achieved": roof.get("achieved"), "peak": roof.get("peak"), "unit": roof.get("unit"), "frac": roof.get("frac"),
                     "traffic": roof.get("traffic"), "avg_kernel_ms": roof.get("avg_kernel_ms"),
                     "launches_timed": roof.get("launches_timed"), "points_per_launch": roof.get("points_per_launch"),
                     "alg_flops_per_point": roof.get("alg_flops_per_point"),
                     "nominal_hbm_frac_at_1700B_per_point": _pick(roof, "nominal_hbm", "frac"),
                     "measured_hbm_frac": _pick(roof, "measured_hbm", "frac"), "valu_issue_frac": _pick(roof, "valu_issue", "frac"),
                     "valu_issue_frac_range": [_pick(roof, "valu_issue", "frac_all_fp32_class"), _pick(roof, "valu_issue", "frac_all_int3_class")],
                     "valu_cycles_per_wave_instruction": _pick(roof, "valu_issue", "cycles_per_wave_instruction", "blend_11_to_8"),
                     "wait_frac": _pick(roof, "counters", "wait_frac"),
                     "valu_insts_per_launch": _pick(roof, "valu_issue", "valu_wave_instructions_per_launch"),
                     "lanes_active": _pick(roof, "counters", "lanes_active"), "l2_hit_rate": _pick(roof, "counters", "l2_hit_rate"),
                     "counters_from": _pick(roof, "counters", "source_file")}
    if cb:
        c["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "kind", "sample", "seconds", "pose_diff_gpu_vs_cpu_m",
                                                    "pose_diff_gpu_vs_cpu_rad", "iterations_equal", "rows_equal")}
        c["cpu_baseline"]["all_cores_value"] = _pick(cb, "all_cores", "value")
        c["cpu_baseline"]["all_cores"] = _pick(cb, "all_cores", "cores")
    if out.get("parity_failed"):
        c["parity_failed"] = out["parity_failed"][:300]
    if out.get("aborted_secondary_legs"):
        c["aborted_secondary_legs"] = out["aborted_secondary_legs"]
    opt = []   # optional blocks, most important first
    se = out.get("certificate_sweep") or {}
    if se:
        opt.append(("value_searching_every_point", se.get("value_searching_every_point")))
        opt.append(("search_modes", {"kd_tree_walk_value": _pick(se, "kd_tree_walk", "value"),
                                     "kd_tree_walk_value_searching_every_point": _pick(se, "kd_tree_walk", "value_searching_every_point"),
                                     "pose_diff_m": se.get("pose_diff_between_the_two_modes_m"), "iterations_equal": se.get("iterations_equal"),
                                     "rows_equal": se.get("rows_equal")}))
    if out.get("ranks"):
        opt.append(("ranks", out["ranks"]))
    if out.get("grid_sweep"):
        opt.append(("grid_sweep", {"share_left_to_the_tree_search": _pick(out, "grid_sweep", "share_left_to_the_tree_search")}))
    v16 = out.get("vlp16_throughput") or {}
    if v16:
        opt.append(("vlp16", {"value": v16.get("value"), "ms_per_step": v16.get("ms_per_step"), "steps": v16.get("steps"),
                              "roofline_frac": _pick(v16, "roofline", "frac"), "avg_kernel_ms": _pick(v16, "roofline", "avg_kernel_ms"),
                              "error": v16.get("error")}))
    pg = out.get("pose_graph") or {}
    if pg:
        opt.append(("pose_graph", {"lm_iters_per_s": pg.get("lm_iters_per_s"), "lm_iterations": pg.get("lm_iterations"),
                                   "solver": pg.get("solver"), "solver_iterations": pg.get("solver_iterations"), "chi2_final": pg.get("chi2_final"),
                                   "keyframes": pg.get("keyframes"), "edges": pg.get("edges"), "n_gpus": pg.get("n_gpus"),
                                   "allreduce_bytes_per_linearisation": pg.get("allreduce_bytes_per_linearisation"),
                                   "roofline_frac": _pick(pg, "roofline", "frac"), "roofline_kernel": _pick(pg, "roofline", "kernel"),
                                   "cpu_lm_iters_per_s": _pick(pg, "cpu_baseline", "value"),
                                   "inexact_lm_tol_1e-3_iters_per_s": _pick(pg, "inexact_lm", "lm_iters_per_s"), "error": pg.get("error")}))
    for key in ("mapping_frame", "mapping_frame_vlp16", "mapping_frame_cubes"):
        mf = out.get(key) or {}
        if mf:
            opt.append((key, {"gpu_ms_per_frame": mf.get("gpu_ms_per_frame"), "p99_ms": mf.get("gpu_ms_p99"),
                              "worst_ms": mf.get("gpu_ms_worst_frame"), "frames": mf.get("frames"),
                              "overlapped_ms": _pick(mf, "overlapped", "gpu_ms_per_frame"),
                              "overlapped_p99_ms": _pick(mf, "overlapped", "gpu_ms_p99"),
                              "overlapped_worst_ms": _pick(mf, "overlapped", "gpu_ms_worst_frame"),
                              "pipelined_period_ms": _pick(mf, "pipelined", "ms_per_frame"),
                              "surround_to_map_ms": _pick(mf, "gpu_ms", "surround_to_map"),
                              "search_structure": "cell grids (trees deferred)" if mf.get("search_structure_build") else ("kd-trees" if mf.get("tree_build") else None),
                              "tree_build_hbm_frac": _pick(mf, "tree_build", "frac"), "tree_build_traffic": _pick(mf, "tree_build", "traffic"),
                              "cpu_ms_per_frame": mf.get("cpu_ms_per_frame"), "pose_diff_gpu_vs_cpu_m": mf.get("pose_diff_gpu_vs_cpu_m"),
                              "error": mf.get("error")}))
    ss = out.get("single_scan") or {}
    if ss:
        opt.append(("single_scan", {k: ss.get(k) for k in ("ms_per_scanmatch", "host_buffers_ms_per_scanmatch", "gn_iterations", "sweep_kernel_ms")}))
    sh = out.get("sharded_points") or {}
    if sh:
        opt.append(("sharded_points", {k: sh.get(k) for k in ("value", "ms_per_scanmatch", "n_gpus", "allreduce_bytes_per_iteration", "rccl_ranks", "error") if k in sh}))
    js = out.get("joint_lidar_stereo") or {}
    if js:
        opt.append(("joint_lidar_stereo", {k: js.get(k) for k in ("ms_per_joint_scanmatch", "joint_rows_per_s", "n_gpus", "pose_diff_gpu_vs_cpu_m", "error") if k in js}))
    ff = out.get("final_feature_map") or {}
    if ff:
        opt.append(("final_feature_map", {k: ff.get(k) for k in ("keyframes_per_s", "ms_per_keyframe", "keyframes", "matched", "added",
                                                                 "pose_err_vs_ground_truth_m", "error") if k in ff}))
    sp = out.get("sweep_pipeline") or {}
    if sp:
        opt.append(("sweep_pipeline", {k: {"ms_per_sweep": _pick(sp, k, "ms_per_sweep"), "threads_ms_per_sweep": _pick(sp, k, "node_threads", "ms_per_sweep"),
                                           "python_threads_ms_per_sweep": _pick(sp, k, "node_threads_python", "ms_per_sweep"),
                                           "cpp_one_thread_ms_per_sweep": _pick(sp, k, "node_threads", "one_thread_ms_per_sweep"),
                                           "odometry_ms": _pick(sp, k, "ms", "odometry"), "mapping_ms": _pick(sp, k, "ms", "mapping")}
                                       for k in ("vlp16", "rings64") if k in sp} or {"error": sp.get("error")}))
    for k, v in opt:
        c[k] = v
    c["report"] = "bench_report.json (full report: every leg, accountings, counter sources); also one line on stderr"
    c = _r(c)
    line = json.dumps(c, separators=(",", ":"))
    for k, _ in reversed(opt):   # never reached today (~3.5 KB); keeps the contract if a leg grows
        if len(line) <= COMPACT_LIMIT:
            break
        c.pop(k, None)
        c["dropped_for_size"] = c.get("dropped_for_size", []) + [k]
        line = json.dumps(c, separators=(",", ":"))
    assert len(line) <= COMPACT_LIMIT, len(line)
    return line


def emit(out):
    """Full report -> bench_report.json (+ gpurun_out/ when it exists, so it comes back from the GPU box) and stderr; the compact
    line -> stdout, LAST."""
    full = json.dumps(out)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_report.json"), "w") as f:
                    f.write(full + "\n")
            except OSError:
                pass
    print(full, file=sys.stderr, flush=True)
    sys.stdout.flush()
    line = compact_line(out)
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, (line + "\n").encode())  # the descriptor stdout WAS (see main): the only bytes on it


def vlp16_throughput_leg(ctx, lidar, synth, dense, span, rank, world, args, opts, distmod, dist, info, np):
    """point-residuals/s on 16-ring x 1800 scans (BASELINE configs[1]'s sensor, every return a query -- SURVEY 8d) against the
    same map: `--scans` different VLP-16 scans per step and GPU, all in flight, cold calls, barrier + max over ranks like the
    headline; a quarter of the headline's steps (a step is a quarter of its size)."""
    rng = np.random.default_rng(9191 + rank)
    scans, inits = [], []
    for k in range(args.scans):
        g = dense[int(rng.integers(-span, span)) % len(dense)].copy()
        g[3:5] += rng.uniform(-1.0, 1.0, 2)
        g[2] += rng.uniform(-0.2, 0.2)
        qc, qs = lidar.scan(g, 16, 1800, seed=1900000 + 1000 * rank + k)
        scans.append((qc, qs))
        inits.append(synth.perturb_pose(g, seed=5099 + 1000 * rank + k))
    n_pts = sum(len(c) + len(s) for c, s in scans)
    n_corner = sum(len(c) for c, _ in scans)
    ctx.scan_set_batch(scans)
    inits = np.stack(inits)
    steps = max(2, args.steps // 2)
    quiet_gc()
    for _ in range(min(2, args.warmup)):
        ctx.run_batch(inits, opts)
    distmod.barrier(dist)
    t0 = time.perf_counter()
    pt_res = iters = sweep_launches = 0
    sweep_ms = 0.0
    n_conv = 0
    for _ in range(steps):
        status, poses, sts = ctx.run_batch(inits, opts)
        pt_res += sum(s.point_residuals for s in sts)
        iters += sum(s.iterations for s in sts)
        sweep_ms += sts[0].gpu_ms_sweep
        sweep_launches += sts[0].sweep_launches
        n_conv = int(sum(1 for s in sts if s.converged))
    distmod.barrier(dist)
    elapsed = time.perf_counter() - t0
    (total_pt_res, total_iters), t = distmod.aggregate(dist, [pt_res, iters], elapsed)
    if rank != 0:
        return None
    roof = sweep_roofline(pt_res, sweep_ms, sweep_launches, float(info.n_corner + info.n_surf), grid=ctx.grid_launches() > 0)
    # the committed counter passes are of the 64-ring command: the 16-ring launches run the same kernel on a quarter of the points
    roof["counters_of"] = "the 64-ring headline command (same kernel instantiation): see roofline.counters of the headline"
    roof.pop("counters", None)
    return {"metric": "point-residuals/s", "value": total_pt_res / t, "unit": "point-residuals/s", "n_gpus": world, "steps": steps,
            "ms_per_step": 1e3 * t / steps, "timed_region_s": t, "lm_iters_per_s": total_iters / t, "dtype": "f32",
            "config": {"workload": "synthetic 16-ring x 1800 (VLP-16) scan-to-map scanMatchScan GN loops against the same %d-frame "
                                   "voxel map: %d scans per step and GPU, all in flight" % (args.map_frames, args.scans),
                       "scan_points_per_step": n_pts, "scan_corner_share": n_corner / max(1, n_pts),
                       "gn_iters_per_scan": iters / steps / args.scans, "converged_scans": n_conv},
            "roofline": roof}


def tree_build_roofline(ms, n_corner, n_surf, np):
    """Roofline object of the kd-tree build of a mapping frame (surround -> both trees; ScanMatch.cpp:75-76 rebuilds them on
    every call): SURVEY 8d prices it as M x 16 B x log2(M / 10) streamed per tree.  The build is a chain of short kernels
    (seven per level of the big nodes, then the wavefront-local phases): what bounds it is the latency of that chain, and the
    HBM fraction says how far from streaming it is.  `traffic`: the committed counter passes of tools/bench_treebuild.py
    (tools/profile_treebuild.sh), per build, with the per-kernel breakdown."""
    alg = sum(m * 16.0 * np.log2(m / 10.0) for m in (n_corner, n_surf) if m > 10)
    t_s = ms * 1e-3
    roof = {"kernel": "lv_count / lv_hflags / lv_hwrite / lv_hswap / lv_pass2 / lv_bounds / lv_final (levels), kd_build_small, kd_build_tiny",
            "bound": "latency",
            "bound_detail": "a chain of ~100 dependent short launches (5-15 us each: a kernel boundary on eight XCDs, then a few dependent "
                            "loads) for the nodes above 1 536 points, then one wavefront per subtree: no bandwidth is near a limit",
            "achieved": alg / t_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / t_s / 1e9 / HBM_PEAK_GBS,
            "alg_bytes_per_build": alg, "ms_per_build": ms, "points": [int(n_corner), int(n_surf)],
            "accounting": "sum over both trees of M x 16 B x log2(M / 10) (SURVEY 8d) / wall time of lslam_fmap_surround_to_map "
                          "(gather of the active cubes + both builds, median of the frames)",
            "traffic": None}
    prof = newest_profile("tree_pmc.csv")
    if prof:
        per = {}
        for line in open(os.path.join(ROOT, prof)):
            f = line.strip().split(",")
            if len(f) >= 6 and not line.startswith("#") and f[0] != "pass" and f[2] in ("FETCH_SIZE", "WRITE_SIZE"):
                k = per.setdefault(f[1], {"FETCH_SIZE": 0.0, "WRITE_SIZE": 0.0})
                k[f[2]] = float(f[5])
        if per:
            by_kernel = {k: (2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0 for k, v in per.items()}
            tot = sum(by_kernel.values())
            roof["traffic"] = tot
            roof["measured_hbm"] = {"bytes_per_build": tot, "achieved": tot / t_s / 1e9, "frac": tot / t_s / 1e9 / HBM_PEAK_GBS, "unit": "GB/s",
                                    "bytes_per_build_by_kernel": {k: v for k, v in sorted(by_kernel.items(), key=lambda kv: -kv[1])},
                                    "source": "%s: (2 x FETCH_SIZE + WRITE_SIZE) x 1024, summed over a build's launches; not measured in this run" % prof}
    return roof


def sweep_roofline(pt_res, sweep_ms, sweep_launches, map_points, grid=True):
    """The roofline object of one timed region of sweep launches (the 64-ring headline, the 16-ring leg).

    achieved / peak / frac are PHYSICAL: the sweep kernel is bound by vector-ALU instruction issue (the counter passes: 99 % of the
    fp32 issue slots of the 1 024 SIMDs are taken), so the line prices it on the fp32 roof -- SURVEY 8d's 1.2 kflop per
    point-residual x the points an average timed launch processed / that launch's HIP-event duration, against the 157.3 TFLOP/s
    vector fp32 peak of MI355X_MICROARCH.md.  The fraction is small because the search is divergent (43 of 64 lanes active) and
    most of its instructions are compares, selects and address arithmetic, not the counted flops; `valu_issue` says how full the
    issue port is.  SURVEY 8d's byte pricing is kept beside it as `nominal_hbm` (it exceeds 1: those bytes are bytes TOUCHED, 97 %
    of them L1 hits -- not a fraction of anything) and the counter-measured HBM-side traffic as `measured_hbm`."""
    avg_sweep_ms = sweep_ms / max(1, sweep_launches)
    t_s = avg_sweep_ms * 1e-3
    # algorithmic work of an average timed launch: scans of a chunk that have already converged are skipped by later
    # launches, so count the points actually processed
    pts_per_launch = pt_res / max(1, sweep_launches)
    flops = FLOPS_PER_POINT_RESIDUAL * pts_per_launch
    tflops = flops / t_s / 1e12 if t_s > 0 else 0.0
    survey_gbs = ALG_BYTES_PER_POINT_RESIDUAL * pts_per_launch / t_s / 1e9 if t_s > 0 else 0.0
    bounded_gbs = ALG_BYTES_PER_POINT_BOUNDED * pts_per_launch / t_s / 1e9 if t_s > 0 else 0.0
    compulsory = map_points * 16.0 + pts_per_launch * (16.0 + 36.0)
    roof = {
        "kernel": ("sweep_grid_kernel<256> (the grid sweep: 27-cell probe + proof for every point, residual chain for the proven ones; "
                   "tests/test_gpu_grid.py and test_gpu_stack_shapes.py hold it against the oracle) + cert_plan_kernel + "
                   "sweep_queue_kernel<256,true,12> (kd-tree search + residual chain of the points the probe could not prove); one timed "
                   "'launch' is one sweep = that group of dispatches (HIP events on the first and the last of them)") if grid else
                  ("sweep_kernel<256,true,false,12> (the shallow-stack batch instantiation; tests/test_gpu_stack_shapes.py holds it "
                   "against the oracle) -- from a loop's second sweep on as the certificate sweep: sweep_kernel<...,1> over every point "
                   "+ cert_plan_kernel + sweep_queue_kernel<256,true,12> over the points whose neighbours could not be carried over; "
                   "one timed 'launch' is one sweep = that group of dispatches (HIP events on the first and the last of them)"),
        "kernel_short": "sweep_grid_kernel<256> + cert_plan_kernel + sweep_queue_kernel<256,true,12>" if grid else
                        "sweep_kernel<256,true,false,12> (+ certificate pass: cert_plan_kernel, sweep_queue_kernel)",
        "bound": "valu",
        "achieved": tflops,
        "peak": FP32_PEAK_TFLOPS,
        "unit": "TFLOP/s",
        "frac": tflops / FP32_PEAK_TFLOPS,
        "accounting": "achieved = %.0f flop per point-residual (SURVEY 8d) x %.4g points an average timed launch processed / its "
                      "HIP-event duration of %.4g ms; peak = vector fp32 (MI355X_MICROARCH.md).  Neither `hbm` nor `mfma` bounds "
                      "this kernel: the counters put VALU issue at `valu_issue.frac` of its slots and HBM at `measured_hbm.frac`.  "
                      "The flops are the ALGORITHM's (a 5-NN search per point and sweep, SURVEY's count for the kd-tree walk); the grid "
                      "sweep finds the same five with fewer executed instructions, which shows as a higher fraction, not as more work"
                      % (FLOPS_PER_POINT_RESIDUAL, pts_per_launch, avg_sweep_ms),
        "alg_flops_per_point": FLOPS_PER_POINT_RESIDUAL,
        "alg_flops_per_launch": flops,
        "avg_kernel_ms": avg_sweep_ms,
        "launches_timed": sweep_launches,
        "points_per_launch": pts_per_launch,
        # SURVEY 8d's byte pricing (1.7 KB per point-residual, nanoflann's unbounded search on the surveyed map) and the same
        # with the bytes the bounded search really touches on this map: NOMINAL -- above the HBM peak because they are L1 hits
        "nominal_hbm": {"alg_bytes_per_point": ALG_BYTES_PER_POINT_RESIDUAL, "alg_bytes_per_launch": ALG_BYTES_PER_POINT_RESIDUAL * pts_per_launch,
                        "achieved": survey_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": survey_gbs / HBM_PEAK_GBS,
                        "bounded_search": {"alg_bytes_per_point": ALG_BYTES_PER_POINT_BOUNDED, "achieved": bounded_gbs,
                                           "frac": bounded_gbs / HBM_PEAK_GBS},
                        "note": "bytes touched, not bytes moved from HBM: a fraction above 1 means exactly that"},
        # SURVEY 8d asks for both accountings: the compulsory-unique lower bound of a sweep -- every map point and every
        # query read once, every output written once: (Mc+Ms) 16 B + N (16 + 36) B
        "compulsory_hbm": {"bytes_per_launch": compulsory, "achieved": compulsory / t_s / 1e9 if t_s > 0 else 0.0, "unit": "GB/s",
                           "frac": (compulsory / t_s / 1e9 if t_s > 0 else 0.0) / HBM_PEAK_GBS},
    }
    roof.update(pmc_counters(avg_sweep_ms))
    # which resource the counters name: the issue port only when the priced instructions take >= 0.8 of the SIMDs' time
    vi = (roof.get("valu_issue") or {}).get("frac")
    wf = (roof.get("counters") or {}).get("wait_frac")
    mh = (roof.get("measured_hbm") or {}).get("frac")
    if vi is not None and vi >= 0.8:
        roof["bound"] = "valu"
    elif vi is not None:
        roof["bound"] = "mixed: valu issue %.2f of the SIMDs' time, waves parked on memory %s of their life, hbm %s of peak -- no single resource saturated" % (
            vi, "%.2f" % wf if wf is not None else "n/a", "%.2f" % mh if mh is not None else "n/a")
    return roof


def gather_per_rank(distmod, dist, rank, world, x):
    """[x of rank 0, x of rank 1, ...] on every rank, through the one reduction dist.aggregate already has (a one-hot sum)."""
    v = [0.0] * world
    v[rank] = float(x)
    got, _ = distmod.aggregate(dist, v, 0.0)
    return [float(g) for g in got]


def dry_run_report(world, ranks_counted, per_rank):
    """LSLAM_BENCH_DRY_RUN: a report with the keys and string lengths of a real one (numbers are placeholders), so that the CPU
    test of the launcher also tests that the printed line stays parseable and short."""
    long = "x" * 600
    roof = {"kernel": long, "kernel_short": "sweep_kernel", "bound": "valu", "achieved": 9.4, "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": 0.06, "traffic": 4.35e9, "avg_kernel_ms": 6.0, "launches_timed": 200, "points_per_launch": 4.7e7,
            "alg_flops_per_point": FLOPS_PER_POINT_RESIDUAL, "accounting": long, "nominal_hbm": {"frac": 1.66, "note": long},
            "measured_hbm": {"frac": 0.09, "source": long}, "valu_issue": {"frac": 0.65, "frac_all_fp32_class": 0.54, "frac_all_int3_class": 0.9, "cycles_per_wave_instruction": {"blend_11_to_8": 2.49}, "valu_wave_instructions_per_launch": 3.6e9, "source": long},
            "counters": {"lanes_active": 43.0, "l2_hit_rate": 0.9, "wait_frac": 0.45, "source": long, "source_file": "profiles/r04_pmc_sweep.csv"}}
    mf = {"gpu_ms": {"surround_to_map": 1.2}, "gpu_ms_per_frame": 3.2, "gpu_ms_p99": 3.9, "gpu_ms_worst_frame": 4.0, "frames": 200,
          "overlapped": {"gpu_ms_per_frame": 2.3, "gpu_ms_p99": 2.9, "gpu_ms_worst_frame": 3.0, "schedule": long},
          "tree_build": {"frac": 0.018, "traffic": 5.9e8, "accounting": long}, "cpu_ms_per_frame": 900.0, "pose_diff_gpu_vs_cpu_m": 1e-6,
          "gpu_ms_per_frame_each": [[1.0] * 6] * 200}
    return {"dry_run": True, "ranks_counted": ranks_counted,
            "metric": "point-residuals/s", "value": sum(per_rank), "unit": "point-residuals/s", "n_gpus": world, "steps": 1, "warmup": 0,
            "ms_per_step": 60.0, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "lm_iters_per_s": 1.0e5, "timed_region_s": 1.2,
            "config": {"workload": long[:300], "scans_per_step_per_gpu": 960, "scan_points_per_step": 110000000,
                       "map": {"frames": 10000, "surround_corner": 157000, "surround_surf": 587000}, "gn_iters_per_scan": 4.3,
                       "parallelism": long[:100], "pose_err_vs_ground_truth_m": {"max": 0.01}, "converged_scans": 960},
            "roofline": roof, "ranks": {"world": world, "per_rank_value": per_rank, "rccl_ranks": None},
            "certificate_sweep": {"what": long, "value_searching_every_point": 7.0e9, "share_of_point_residuals_certified": 0.25,
                                  "pose_diff_between_the_two_modes_m": 1e-7, "iterations_equal": True, "rows_equal": True},
            "single_scan": {"ms_per_scanmatch": 0.35, "host_buffers_ms_per_scanmatch": 0.6, "gn_iterations": 4, "sweep_kernel_ms": 0.05},
            "vlp16_throughput": {"value": 5.7e9, "ms_per_step": 20.0, "steps": 10, "roofline": dict(roof)},
            "cpu_baseline": {"value": 2.0e6, "unit": "point-residuals/s", "cores": 1, "kind": "port", "sample": long[:250], "seconds": 20.0,
                             "pose_diff_gpu_vs_cpu_m": 1e-6, "pose_diff_gpu_vs_cpu_rad": 1e-7, "iterations_equal": True, "rows_equal": True,
                             "all_cores": {"value": 1.0e7, "cores": 8, "kind": long[:80]}},
            "mapping_frame": mf, "mapping_frame_vlp16": mf, "mapping_frame_cubes": mf,
            "final_feature_map": {"keyframes_per_s": 900.0, "ms_per_keyframe": 1.1, "keyframes": 300, "matched": 298, "added": 300,
                                  "pose_err_vs_ground_truth_m": 0.01, "workload": long},
            "sweep_pipeline": {"vlp16": {"ms_per_sweep": 3.0, "ms": {"odometry": 0.3, "mapping": 0.8}, "node_threads": {"ms_per_sweep": 2.0}},
                               "rings64": {"ms_per_sweep": 5.0, "ms": {"odometry": 0.4, "mapping": 0.8}, "node_threads": {"ms_per_sweep": 3.0}}},
            "sharded_points": {"value": 1.0e9, "ms_per_scanmatch": 0.4, "n_gpus": world, "allreduce_bytes_per_iteration": 256},
            "joint_lidar_stereo": {"ms_per_joint_scanmatch": 0.5, "joint_rows_per_s": 1e9, "n_gpus": world, "parity": long},
            "pose_graph": {"lm_iters_per_s": 519.0, "lm_iterations": 100, "solver_iterations": 11000, "chi2_final": 1.0, "keyframes": 5000,
                           "edges": 24999, "n_gpus": world, "allreduce_bytes_per_linearisation": 8900000,
                           "roofline": {"kernel": "pg_pcg_persistent_kernel", "frac": 0.019, "accounting": long, "bound_detail": long},
                           "cpu_baseline": {"value": 6.4, "sample": long}}}


def make_comm(pkg, dist, torch, rank, local_rank, world):
    """The library's own RCCL communicator: rank 0 makes the id, torch.distributed carries the 128 bytes."""
    import numpy as np
    uid = pkg.Comm.unique_id() if rank == 0 else np.zeros(128, np.uint8)
    if dist is not None:
        t = torch.from_numpy(uid.astype(np.int32)).cuda()
        dist.broadcast(t, src=0)
        uid = t.cpu().numpy().astype(np.uint8)
    return pkg.Comm(local_rank, uid, rank, world)


# the per-scan lslam_stats fields a caller of lslam_scanmatch_run_batch reads as results (the timings and the launch count are
# measurements of the run, not outputs of it)
DUMP_STATS = ("status", "iterations", "n_line", "n_plane", "n_rows", "degenerate", "converged", "delta_r", "delta_t", "score",
              "percent", "point_residuals", "sweeps", "score2", "percent2")


def dump_outputs(d, status, poses, sts, rank, world, np):
    """--dump-outputs: what the last timed step returned -- the refined poses (float32, as the library writes them), the
    batch's worst status and the per-scan statistics (float64; every integer field is exact in it) -- as d/<name>.npy.
    About 140 KB at the default sizes.  With several ranks every rank writes its own files, suffixed _rank<r>."""
    os.makedirs(d, exist_ok=True)
    arrays = {"poses": np.ascontiguousarray(poses, np.float32), "batch_status": np.array([int(status)], np.float64)}
    for f in DUMP_STATS:
        arrays["stats_" + f] = np.array([getattr(s, f) for s in sts], np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ("_rank%d" % rank if world > 1 else "") + ".npy"), a)


def quiet_gc():
    import gc
    gc.collect()
    gc.freeze()


def newest_profile(suffix):
    """profiles/rNN_<suffix> of the highest round that has one (the counter passes are committed per round)."""
    import glob
    c = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    return os.path.relpath(c[-1], ROOT) if c else None


def pmc_counters(avg_sweep_ms):
    """What the hardware counters say about the sweep kernel.  PMC counters cannot be collected inside the
    timed run (rocprofv3 needs its own passes, FETCH_SIZE / WRITE_SIZE separate ones), so these figures are
    read from the COMMITTED summary of the passes of this same command (tools/collect_profiles.sh ->
    profiles/rNN_pmc_sweep.csv; mean per launch over the launches with the full grid -- which is every sweep launch of the
    profiled run: converged scans' blocks exit early, the grid does not shrink) and labelled as such.
    MI355X_MICROARCH.md: FETCH_SIZE / WRITE_SIZE are in KiB and FETCH_SIZE under-reports wide reads by 2x
    on gfx950, so HBM-side traffic = (2 * FETCH + WRITE) * 1024; an L2 request is 128 B."""
    prof = newest_profile("pmc_sweep.csv")
    if not prof:
        return {"traffic": None, "valu_issue": None, "measured_hbm": None, "counters": "no committed counter profile"}
    v = {}
    src = ""
    for line in open(os.path.join(ROOT, prof)):
        if line.startswith("#"):
            src += line[1:].strip() + " "
            continue
        f = line.strip().split(",")
        if len(f) >= 4 and f[0] != "pass":
            v[f[1]] = float(f[3])
    g = v.get
    traffic = (2.0 * g("FETCH_SIZE", 0.0) + g("WRITE_SIZE", 0.0)) * 1024.0 if "FETCH_SIZE" in v else None
    c = {"source": "%s (rocprofv3 --pmc passes; %s)" % (prof, src.strip()[:200]), "source_file": prof}
    # the profiled launches' own duration in engine cycles: GRBM_GUI_ACTIVE (summed over the 8 XCDs; at 2.4 GHz it reproduces
    # the HIP-event duration of these launches), else SQ_BUSY_CYCLES (summed over the 32 shader engines)
    cyc = v["GRBM_GUI_ACTIVE"] / 8.0 if v.get("GRBM_GUI_ACTIVE", 0) > 0 else v.get("SQ_BUSY_CYCLES", 0.0) / 32.0
    t_s = cyc / 2.4e9 if cyc > 0 else avg_sweep_ms * 1e-3
    if cyc > 0:
        c["profiled_launch_ms"] = 1e3 * t_s
        c["profiled_launch_cycles"] = cyc
    measured_hbm = None
    if traffic is not None and t_s > 0:
        gbs = traffic / t_s / 1e9
        measured_hbm = {"bytes_per_launch": traffic, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                        "source": "(2 x FETCH_SIZE + WRITE_SIZE) x 1024 per launch (%s) / that launch's duration" % prof}
    if "TCC_REQ_sum" in v and t_s > 0:
        c["l2_gbs"] = v["TCC_REQ_sum"] * 128.0 / t_s / 1e9
        c["l2_frac"] = c["l2_gbs"] / L2_PEAK_GBS
        if v.get("TCC_HIT_sum", 0) + v.get("TCC_MISS_sum", 0) > 0:
            c["l2_hit_rate"] = v["TCC_HIT_sum"] / (v["TCC_HIT_sum"] + v["TCC_MISS_sum"])
    if "SQ_INSTS_VALU" in v and "SQ_THREAD_CYCLES_VALU" in v and v["SQ_INSTS_VALU"] > 0:
        c["lanes_active"] = v["SQ_THREAD_CYCLES_VALU"] / v["SQ_INSTS_VALU"]
    if "SQ_WAIT_ANY" in v and v.get("SQ_WAVE_CYCLES", 0) > 0:
        c["wait_frac"] = v["SQ_WAIT_ANY"] / v["SQ_WAVE_CYCLES"]
    valu_issue = None
    if "SQ_INSTS_VALU" in v and cyc > 0:
        # What the vector-ALU instructions of a sweep take of the SIMDs' time, priced with MEASURED costs per wave-instruction
        # (tools/ubench_valu.hip -> profiles/rNN_ubench_valu.json: independent instructions, four waves per SIMD, s_memtime):
        # the fp32 class (v_fma / v_fmac / v_mul / v_sub_f32: 1.95 shader cycles per wave64 instruction -- the guide's 2 on a
        # SIMD-32) and the class of v_med3_u32 / v_and_or_b32 / v_cndmask_b32 with an SGPR mask / fp64 (3.24).  The grid
        # probe's candidate loop -- the bulk of the kernel's instructions, csrc/lslam_grid.hpp -- is 19 instructions of which 8
        # are of the second class (five v_med3_u32, v_and_or_b32, two v_cndmask_b32): the blend below.  A half-empty wavefront
        # costs the same (measured: 32 active lanes = 64).  SQ_ACTIVE_INST_VALU (per-wave busy quad-cycles, which overlap between
        # the waves of a SIMD and exceed the SIMDs' time) is kept as a raw figure only.
        cost = valu_costs()
        insts, simd_cyc = v["SQ_INSTS_VALU"], cyc * 1024.0
        blend = (11.0 * cost["fp32"] + 8.0 * cost["int3"]) / 19.0
        frac = insts * blend / simd_cyc
        valu_issue = {"achieved": insts * blend / t_s, "peak": 1024.0 * 2.4e9, "unit": "SIMD cycles/s",
                      "frac": frac, "frac_all_fp32_class": insts * cost["fp32"] / simd_cyc, "frac_all_int3_class": insts * cost["int3"] / simd_cyc,
                      "cycles_per_wave_instruction": {"fp32_class": cost["fp32"], "med3_cndmask_fp64_class": cost["int3"], "blend_11_to_8": blend,
                                                      "source": cost["source"]},
                      "busy_quad_cycles_raw": v["SQ_ACTIVE_INST_VALU"] * 4.0 / simd_cyc if "SQ_ACTIVE_INST_VALU" in v else None,
                      "lanes_active_of_64": c.get("lanes_active"),
                      "valu_wave_instructions_per_launch": insts,
                      "note": "frac = SQ_INSTS_VALU x measured cycles per wave-instruction (11 : 8 blend of the two classes, the candidate "
                              "loop's mix) / (1 024 SIMDs x GRBM_GUI_ACTIVE / 8); the two all-one-class figures bracket it.  Below 0.8 the "
                              "issue port is not what bounds the kernel on its own: see wait_frac (waves parked on memory) beside it",
                      "source": "SQ_INSTS_VALU, GRBM_GUI_ACTIVE of %s; costs of %s" % (prof, cost["source"])}
    for k in ("TA_BUSY_avr", "TCP_TOTAL_CACHE_ACCESSES_sum", "TA_FLAT_READ_WAVEFRONTS_sum", "TCP_TCC_READ_REQ_sum", "GRBM_GUI_ACTIVE",
              "TA_TA_BUSY_sum", "SQ_INSTS_VALU_MFMA_F32", "SQ_VALU_MFMA_BUSY_CYCLES"):
        if k in v:
            c[k] = v[k]
    if "TA_BUSY_avr" in v and cyc > 0:
        c["ta_busy"] = v["TA_BUSY_avr"] / cyc  # texture-address units: vector-memory instruction issue
    return {"traffic": traffic,
            "traffic_source": "committed rocprofv3 --pmc passes of `bench.py --headline-only` (tools/collect_profiles.sh -> %s), mean per "
                              "sweep over all sweeps of the profiled run (the same population as avg_kernel_ms: a batch's later sweeps launch the "
                              "running scans' workgroups only); not measured in this run" % prof,
            "valu_issue": valu_issue, "measured_hbm": measured_hbm, "counters": c}


def valu_costs():
    """Measured SIMD cycles per wave64 vector instruction (tools/ubench_valu.hip, kept under profiles/): the fp32 class and
    the v_med3 / v_cndmask / fp64 class, at four waves per SIMD (a saturated SIMD).  Falls back to the guide's 2 cycles."""
    prof = newest_profile("ubench_valu.json")
    out = {"fp32": 2.0, "int3": 2.0, "source": "MI355X_MICROARCH.md (2 cycles per wave64 v_fma_f32); no committed microbenchmark"}
    if not prof:
        return out
    try:
        rows = json.load(open(os.path.join(ROOT, prof)))["results"]
        pick = lambda op: [r["simd_ticks_per_wave_instruction"] for r in rows if r["op"] == op and r["lanes"] == 64 and r["waves_per_simd"] == 4][0]
        out = {"fp32": max(pick("v_fma_f32"), pick("v_fmac_f32"), pick("v_mul_f32")),
               "int3": max(pick("v_med3_u32"), pick("v_and_or_b32"), pick("v_cndmask_b32 (sgpr pair)")), "source": prof}
    except Exception as e:  # a malformed file must not take the bench down
        out["source"] += " (%s unreadable: %r)" % (prof, e)
    return out


def sharded_points_leg(pkg, synth, distmod, dist, rank, world, ctx, comm, opts, np, args):
    """ONE 115 200-point scan, its points sharded contiguously over the ranks,
    the 32 fp64 normal-equation sums all-reduced every Gauss-Newton iteration by the library's own RCCL
    communicator on the library's stream (ncclAllReduce between the reducing and the solving kernel, the
    loop stays device-resident), the 6x6 solve replicated.  Strong scaling of a ~60 us sweep: reported as
    measured, next to the recommended no-collective batch mode."""
    pr = synth.make_problem(rings=args.rings, azimuth_steps=1800, seed=0)  # the same scan on every rank
    # ... and the same map: every rank must take the same decisions from the same all-reduced sums
    # (rank 0's map was replaced by the mapping-frame leg)
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    cb, ce = distmod.shard_range(len(pr["corner"]), rank, world)
    sb, se = distmod.shard_range(len(pr["surf"]), rank, world)
    ctx.scan_set(pr["corner"][cb:ce], pr["surf"][sb:se])
    ctx.set_comm(comm)
    for _ in range(3):
        ctx.run_sharded(pr["init_pose"], opts=opts)
    steps = 50
    quiet_gc()
    distmod.barrier(dist)
    t0 = time.perf_counter()
    pt = 0
    for _ in range(steps):
        status, pose, st = ctx.run_sharded(pr["init_pose"], opts=opts)
        pt += st.point_residuals
    distmod.barrier(dist)
    dt = time.perf_counter() - t0
    ctx.set_comm(None)
    (tot,), tmax = distmod.aggregate(dist, [pt], dt)
    return {"value": tot / tmax, "unit": "point-residuals/s", "ms_per_scanmatch": 1e3 * tmax / steps,
            "gn_iterations": int(st.iterations), "n_gpus": world, "scaling": "strong",
            "allreduce_bytes_per_iteration": 256, "transport": "ncclAllReduce (RCCL) on the library's stream",
            "pose_err_vs_ground_truth_m": float(np.abs(pose - pr["gt_pose"])[3:].max())}


def joint_stereo_leg(pkg, synth, distmod, dist, rank, world, ctx, comm, opts, np, args, with_cpu):
    """BASELINE configs[4]: LOAM edge/plane rows + stereo reprojection rows in ONE joint 6x6 system per
    Gauss-Newton iteration (include/lslam_c.h lslam_stereo_set; the reference has no code for the visual
    term -- parity unpinned, the oracle restates ORB-SLAM2's pose-only stereo edge).  One 64-ring scan
    and 2 000 stereo observations of map landmarks; at N>1 the scan points AND the observations are
    sharded over the ranks and the 32 sums all-reduced per iteration (the sharded-points path)."""
    pr = synth.make_problem(rings=args.rings, azimuth_steps=1800, seed=0)
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    pts = np.concatenate([pr["map_corner"], pr["map_surf"]])
    lm, ob, w = synth.make_stereo(pts, pr["gt_pose"], n=2000)
    cam = ctx.default_stereo_cam()
    for i, v in enumerate(synth.T_CAM_LIDAR.reshape(-1)):
        cam.T_cl[i] = float(v)
    cam.weight = 1e-3
    cb, ce = distmod.shard_range(len(pr["corner"]), rank, world)
    sb, se = distmod.shard_range(len(pr["surf"]), rank, world)
    o0, o1 = distmod.shard_range(len(lm), rank, world)
    ctx.scan_set(pr["corner"][cb:ce], pr["surf"][sb:se])
    if world > 1:
        ctx.set_comm(comm)

    def run():
        if world == 1:
            return ctx.run(pr["init_pose"], opts)
        return ctx.run_sharded(pr["init_pose"], opts=opts)

    def timed(steps):
        for _ in range(3):
            run()
        quiet_gc()
        distmod.barrier(dist)
        each = []
        for _ in range(steps):
            t1 = time.perf_counter()
            status, pose, st = run()
            each.append(time.perf_counter() - t1)
        distmod.barrier(dist)
        # median call (max over ranks): one call in a few dozen shows a 30-50 ms host-side stall on the
        # bench box that a mean over 10-25 calls would mostly consist of; the worst call is reported too
        _, med = distmod.aggregate(dist, [0.0], float(np.median(each)))
        _, worst = distmod.aggregate(dist, [0.0], float(max(each)))
        return 1e3 * med, 1e3 * worst, pose, st
    steps = 25
    ms_lidar, worst_lidar, pose_l, st_l = timed(steps)
    ctx.stereo_set(lm[o0:o1], ob[o0:o1], w[o0:o1], cam)
    ms_joint, worst_joint, pose_j, st_j = timed(steps)
    ctx.stereo_clear()
    if world > 1:
        ctx.set_comm(None)
    n_pts = len(pr["corner"]) + len(pr["surf"])
    res = {"ms_per_joint_scanmatch": ms_joint, "ms_per_lidar_only_scanmatch": ms_lidar,
           "statistic": "median of %d calls (max over ranks)" % steps, "ms_worst_call": [worst_lidar, worst_joint],
           "joint_rows_per_s": (st_j.iterations * (n_pts + 3 * len(lm))) / (1e-3 * ms_joint),
           "scan_points": n_pts, "stereo_observations": int(len(lm)), "stereo_weight": float(cam.weight),
           "gn_iterations": int(st_j.iterations), "gn_iterations_lidar_only": int(st_l.iterations),
           "rows_last_iteration": int(st_j.n_rows), "n_gpus": world,
           "parallelism": "scan points and observations sharded over %d GPU(s), 256 B all-reduce per iteration" % world
           if world > 1 else "one GPU, device-resident loop",
           "pose_err_vs_ground_truth_m": float(np.abs(pose_j - pr["gt_pose"])[3:].max()),
           "pose_err_lidar_only_m": float(np.abs(pose_l - pr["gt_pose"])[3:].max()),
           "parity": "unpinned: no reference code for the visual term"}
    if with_cpu and rank == 0:
        from oracle_lib import Oracle, OracleStereoCam
        o = Oracle(native=True)
        oc = OracleStereoCam()
        for f, _ in OracleStereoCam._fields_:
            setattr(oc, f, getattr(cam, f))
        t0 = time.perf_counter()
        ok, opose, ost, used = o.scanmatch_joint(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"],
                                                 lm, ob, w, oc, pr["init_pose"])
        cdt = time.perf_counter() - t0
        res["cpu_baseline"] = {"ms_per_joint_scanmatch": 1e3 * cdt, "cores": 1, "kind": "port",
                               "sample": "one joint call of the oracle (kd-trees rebuilt inside, as the reference's scanMatchScan does)",
                               "gn_iterations": int(ost.iterations), "stereo_observations_used": int(used)}
        if world == 1:
            res["pose_diff_gpu_vs_cpu_m"] = float(np.abs(pose_j - opose)[3:].max())
            res["pose_diff_gpu_vs_cpu_rad"] = float(np.abs(pose_j - opose)[:3].max())
    return res


def pose_graph_leg(pkg, synth, distmod, dist, rank, world, local_rank, comm, np, lm_iters, with_cpu):
    """BASELINE config 4: SE(3) pose-graph LM, 5 000 keyframes / 4 999 odometry + 20 000 loop
    edges, fp64, run until the solver's own stopping rule ends it (limit `lm_iters`).  Edges are sharded
    across the ranks; every linearisation all-reduces the block system [H blocks | b | chi2] with the
    library's RCCL communicator on the solver's stream, the damped solve is replicated."""
    g = synth.make_pose_graph()
    pg = pkg.PoseGraph(local_rank)
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"])
    ne = len(g["ij"])
    nbytes = 0
    b, e = distmod.shard_range(ne, rank, world)
    if world > 1:
        pg.set_comm(comm, b, e)
        nbytes = pg.system_doubles() * 8
    pg.optimize(1)  # warm-up (also builds the structures); restart from the initial estimate
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"])
    if world > 1:
        pg.set_comm(comm, b, e)
    t0 = time.perf_counter()
    pg.build()  # graph upload + block structure (g2o: initializeOptimization), outside the timed LM
    build_ms = 1e3 * (time.perf_counter() - t0)
    quiet_gc()
    distmod.barrier(dist)
    t0 = time.perf_counter()
    iters = pg.optimize(lm_iters)
    distmod.barrier(dist)
    dt = time.perf_counter() - t0
    (_,), tmax = distmod.aggregate(dist, [0.0], dt)
    st = pg.last_stats
    est = pg.poses()
    err = np.linalg.norm(est[:, :3] - g["gt"][:, :3], axis=1)
    res = {"lm_iters_per_s": iters / tmax, "lm_iterations": iters, "lm_trials": st.lm_trials,
           "solver_iterations": st.cg_iterations, "chi2_initial": st.chi2_initial, "chi2_final": st.chi2_final,
           "seconds": tmax, "keyframes": len(g["init"]), "edges": ne, "dtype": "f64", "n_gpus": world,
           "graph_build_ms": build_ms, "gpu_ms_total": st.gpu_ms_total,
           "position_err_vs_ground_truth_m": {"mean": float(err.mean()), "max": float(err.max())},
           "allreduce_bytes_per_linearisation": nbytes,
           "parallelism": "edges sharded over %d GPU(s), ncclAllReduce of the block system on the solver's stream, "
                          "replicated damped solve" % world}
    # The solver's dominant kernel is the persistent PCG kernel (one launch per damped solve).  What it must move, by
    # design: the block-CSR matrix ONCE per solve (every 6x6 fp64 block -- diagonal + both orientations of each off-diagonal
    # block -- into registers) and, per PCG iteration, the vectors other workgroups need: z and p written once and read by the
    # neighbouring aggregates (~3 readers), the restricted q / r_c (6 doubles per aggregate, read by everybody).
    pairs = {(min(int(a), int(b_)), max(int(a), int(b_))) for a, b_ in np.asarray(g["ij"]).reshape(-1, 2)}
    blocks = len(g["init"]) + 2 * len(pairs)
    n6 = len(g["init"]) * 6
    matrix_bytes = blocks * 36 * 8 + blocks * 4
    spmv_bytes = matrix_bytes + 3 * n6 * 8
    if st.cg_iterations > 0 and st.gpu_ms_total > 0:
        per_it_s = st.gpu_ms_total * 1e-3 / st.cg_iterations
        fused = st.fused_solves == st.lm_trials
        its = st.cg_iterations / max(1, st.lm_trials)
        vec_bytes_per_it = 2 * n6 * 8 * (1 + 3)  # z and p: one write, ~three remote reads each
        alg_per_solve = matrix_bytes + its * vec_bytes_per_it if fused else its * spmv_bytes
        solve_s = per_it_s * its
        res["fused_solves"] = st.fused_solves
        res["roofline"] = {"kernel": "pg_pcg_persistent_kernel" if fused else "pg_cg_prod_kernel",
                           "bound": "latency",
                           "bound_detail": ("two grid-wide exchanges per PCG iteration through the device's coherence point (~2.5 us each, "
                                            "publish -> visible) plus ~5 us of per-aggregate reductions and arithmetic; the matrix stays in "
                                            "registers for the whole solve: neither HBM nor the fp64 units are near a limit")
                           if fused else
                           ("chain of four small dependent launches per PCG iteration (6-8 us kernels + ~3 us launch-to-launch) on a 15.9 MB "
                            "system that lives in L2 / Infinity Cache"),
                           "achieved": alg_per_solve / solve_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": alg_per_solve / solve_s / 1e9 / HBM_PEAK_GBS, "traffic": None,
                           "alg_bytes_per_solve": alg_per_solve, "pcg_iterations_per_solve": its, "us_per_cg_iteration": 1e6 * per_it_s,
                           "accounting": "bytes a damped solve must move (matrix once: %d B; per PCG iteration the exchanged vectors: %d B) "
                                         "/ (solver GPU time per solve: it includes the preconditioner set-ups and the linearisations)"
                                         % (matrix_bytes, vec_bytes_per_it),
                           # round 2's accounting (a block-CSR product per iteration as if the matrix were re-read): nominal, kept for comparison
                           "nominal_spmv": {"alg_bytes_per_cg_iteration": spmv_bytes, "achieved": spmv_bytes / per_it_s / 1e9,
                                            "frac": spmv_bytes / per_it_s / 1e9 / HBM_PEAK_GBS,
                                            "note": "those bytes are register reads after the first iteration, not memory traffic"}}
        # measured memory traffic of the persistent kernel from the committed counter passes (rocprofv3 --pmc of
        # tools/bench_posegraph.py, mean per launch = per damped solve), not measured in this run
        pmc = newest_profile("pg_pmc.csv")
        if fused and pmc:
            v = {}
            for line in open(os.path.join(ROOT, pmc)):
                f = line.strip().split(",")
                if len(f) >= 4 and not line.startswith("#") and f[0] != "pass":
                    v[f[1]] = float(f[3])
            if "FETCH_SIZE" in v and "WRITE_SIZE" in v:
                per_launch = (2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0
                res["roofline"]["traffic"] = per_launch
                res["roofline"]["measured_hbm"] = {"bytes_per_solve": per_launch, "achieved": per_launch / solve_s / 1e9,
                                                   "frac": per_launch / solve_s / 1e9 / HBM_PEAK_GBS, "unit": "GB/s"}
                res["roofline"]["traffic_source"] = ("%s: (2 x FETCH_SIZE + WRITE_SIZE) x 1024 per launch of pg_pcg_persistent_kernel "
                                                     "(one damped solve); not measured in this run" % pmc)
                if v.get("SQ_WAVE_CYCLES", 0) > 0:
                    res["roofline"]["wait_frac"] = v.get("SQ_WAIT_ANY", 0.0) / v["SQ_WAVE_CYCLES"]
    pg.close()
    if world == 1:
        # Next to the default, never instead of it: the same run as an INEXACT Levenberg-Marquardt (lslam_pg_set_solve_tolerance:
        # a damped solve stops at relative residual 1e-3 instead of 1e-8).  Another trajectory of iterates -- the reference's
        # direct solver ("lm_var", solver_g2o.cpp:16) gives LM exact steps, and 1e-8 is indistinguishable from that -- the same
        # optimum: compared here with the default run's.
        pgi = pkg.PoseGraph(local_rank)
        pgi.set_graph(g["init"], g["ij"], g["meas"], g["info"])
        pgi.build()
        pgi.set_solve_tolerance(1e-3)
        t0 = time.perf_counter()
        it_i = pgi.optimize(lm_iters)
        dt_i = time.perf_counter() - t0
        sti = pgi.last_stats
        esti = pgi.poses()
        pgi.close()
        res["inexact_lm"] = {"solve_tolerance": 1e-3, "lm_iters_per_s": it_i / dt_i, "lm_iterations": it_i, "lm_trials": sti.lm_trials,
                             "solver_iterations": sti.cg_iterations, "seconds": dt_i, "chi2_final": sti.chi2_final,
                             "chi2_rel_diff_vs_default": abs(sti.chi2_final - st.chi2_final) / st.chi2_final,
                             "max_position_diff_vs_default_m": float(np.abs(esti[:, :3] - est[:, :3]).max()),
                             "note": "not the pose_graph value: the default solves every damped system to 1e-8, which is what the reference's direct solver gives LM"}
    if with_cpu and rank == 0:
        # a compiled direct solver beside it: oracle/posegraph_oracle.c -- the same LM with analytic Jacobians and an RCM-ordered
        # envelope block Cholesky, one core (what g2o + CSparse, the reference's solver, do; g2o itself is not available)
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import posegraph_oracle_c as pc
        n_it = min(PG_CPU_ITERS, iters) if iters > 0 else PG_CPU_ITERS
        cest, cst = pc.optimize(g["init"], g["ij"], g["meas"], g["info"], fixed=0, max_iters=n_it)
        # the device solver stopped after the same LM iterations: same chi2 (both solve each damped system to convergence)
        pg2 = pkg.PoseGraph(local_rank)
        pg2.set_graph(g["init"], g["ij"], g["meas"], g["info"])
        pg2.build()
        pg2.optimize(cst.iterations)
        gchi = pg2.last_stats.chi2_final
        gest = pg2.poses()
        pg2.close()
        res["cpu_baseline"] = {"value": cst.iterations / cst.t_total, "unit": "LM-iters/s", "cores": 1, "kind": "port",
                               "sample": "%d LM iterations (%d damped solves) of oracle/posegraph_oracle.c on the same graph: analytic "
                                         "Jacobians, reverse-Cuthill-McKee-ordered envelope block Cholesky (%d blocks, %.2f GFLOP per "
                                         "factorisation), one core; g2o + CSparse, the reference's solver, are not available here"
                                         % (cst.iterations, cst.trials, cst.env_blocks, cst.factor_flops / 1e9),
                               "seconds": cst.t_total,
                               "seconds_by_phase": {"order": cst.t_order, "linearize": cst.t_linearize, "factor": cst.t_factor,
                                                    "solve": cst.t_solve, "chi2": cst.t_chi2},
                               "factor_gflops": cst.factor_flops * cst.trials / cst.t_factor / 1e9 if cst.t_factor > 0 else None,
                               "chi2_after_sample": cst.chi2_final, "gpu_chi2_after_the_same_iterations": gchi,
                               "position_diff_gpu_vs_cpu_m": float(np.abs(gest[:, :3] - cest[:, :3]).max())}
    return res


def single_scan_leg(ctx, scan, init, opts, steps):
    """Latency view of the same path: ONE 115 200-point scan in flight (rank 0, after the timed region;
    the map is the same surround): wall time per scanMatchScan loop and the sweep kernel on its own."""
    qc, qs = scan
    ctx.scan_set(qc, qs)
    for _ in range(5):
        ctx.run(init, opts)
    t0 = time.perf_counter()
    pt = 0
    sw_ms = 0.0
    sw_n = 0
    for _ in range(steps):
        status, pose, st = ctx.run(init, opts)
        pt += st.point_residuals
        sw_ms += st.gpu_ms_sweep
        sw_n += st.sweep_launches
    dt = time.perf_counter() - t0
    avg = sw_ms / max(1, sw_n)
    # PCIe-inclusive: the caller hands over HOST clouds on every call (lslam_scanmatch_scan:
    # pack + Morton order + H2D, then the loop); never the headline value
    t1 = time.perf_counter()
    pt_h = 0
    for _ in range(steps):
        status, pose, st2 = ctx.scanmatch_scan(qc, qs, init, opts)
        pt_h += st2.point_residuals
    dth = time.perf_counter() - t1
    return {"value": pt / dt, "unit": "point-residuals/s", "ms_per_scanmatch": 1e3 * dt / steps,
            "host_buffers_value": pt_h / dth, "host_buffers_ms_per_scanmatch": 1e3 * dth / steps,
            "gn_iterations": st.iterations, "sweep_kernel_ms": avg, "scan_points": int(len(qc) + len(qs)),
            "sweep_us_per_full_scan": 1e3 * sw_ms * (len(qc) + len(qs)) / max(1, pt),
            # algorithmic bytes of the points actually processed / time of ALL sweep launches (the one
            # trailing launch per call that finds the loop finished costs a few microseconds)
            "roofline_frac": ALG_BYTES_PER_POINT_RESIDUAL * pt / (sw_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if sw_ms > 0 else None}


def mapping_frame_leg(pkg, synth, ctx, surround, lidar, gt, opts, np, with_cpu, rings=64, cubes=False):
    """One LaserMapping frame end to end on the device (SURVEY 8f n1/n2 around the hot path), per step:
    extractFeatures on the full-resolution sweep, VoxelGrid of the features (LaserMatcher.cpp:289-301, leaf
    1.0 = the reference default), FeatureMap::update, surround -> kd-trees, scanMatchScan,
    addFeatureCloud -- next to the oracle doing the same steps on one host core (one frame).  The map is
    the active area of the 10k-frame voxel map (both sides load the same downloaded surround)."""
    sur_c, sur_s = surround
    gt = np.asarray(gt, np.float64)
    _, _, cloud, ranges = lidar.scan(gt, rings, 1800, seed=4321, full=True)
    fm = pkg.FeatureMap(ctx, 21, 21, 11)
    fm.setup_filter_size(0.2, 0.4, 0.6)
    fm.update(gt[3:].astype(np.float32))
    fm.add_feature_cloud(sur_c, sur_s, np.eye(4, dtype=np.float32))
    # as LaserMapping sets its context up (the-cooper-mapper_amd/pipeline.py, include/lslam_pipeline.hpp): the per-frame
    # surround map gets its cell grids at once and its kd-trees only if a frame needs them (lslam_map_defer_trees)
    ctx.defer_trees(not cubes)
    R, t = synth.pose_to_Rt(gt)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    init = synth.perturb_pose(gt, seed=77, dt=0.1, dr_deg=0.5)
    gt32 = gt.astype(np.float32)
    # cubes: variant C (FeatureMap::scanMatchScan, util/FeatureMap.h:490-691) -- one kd-tree per cube of the active
    # area, kept between frames; only the cubes the previous frame's addFeatureCloud touched are rebuilt
    steps = ("extract_features", "voxel_grid", "update", "to_cubemap_incremental" if cubes else "surround_to_map",
             "scan_match", "add_feature_cloud")
    acc = {k: [] for k in steps}
    trees = []
    # >= 200 frames for the 64-ring sequential and overlapped schedules (median, p99 and worst frame: the jitter is part of
    # the result); the variants that only add a comparison run fewer
    frames = 12 if cubes else 200
    quiet_gc()
    WARM = 3  # frames before the timed ones (allocations grow to size, the map's first insert)
    for f in range(frames + WARM):
        t0 = time.perf_counter()
        feat = pkg.scan_registration.extract_features(ctx, cloud, ranges)
        t1 = time.perf_counter()
        dc, ds = pkg.voxel_grid2(ctx, feat["less_sharp"], feat["less_flat"], 1.0)  # as LaserMapping.process does (equal leaves: one pass)
        t2 = time.perf_counter()
        fm.update(gt[3:].astype(np.float32))
        t3 = time.perf_counter()
        if cubes:
            fm.to_cubemap()
            if f >= WARM:
                trees.append(fm.cubemap_stats())
        else:
            fm.surround_to_map()
        t4 = time.perf_counter()
        status, pose, st = ctx.scanmatch_scan(dc, ds, init, opts)
        t5 = time.perf_counter()
        fm.add_feature_cloud(dc, ds, T)
        t6 = time.perf_counter()
        if f == 0:
            pose_first = pose.copy()  # same map state as the oracle's single frame below
        if f >= WARM:
            for k, d in zip(steps, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                acc[k].append(d)
    # median over the frames: a single host-side stall (allocator, scheduler) in one frame would otherwise
    # dominate a 6-frame mean; the worst frame is reported next to it
    gpu = {k: 1e3 * float(np.median(v)) for k, v in acc.items()}
    per_frame = np.array([sum(v[i] for v in acc.values()) for i in range(frames)]) * 1e3
    res = {"rings": rings, "gpu_ms": gpu, "gpu_ms_per_frame": sum(gpu.values()), "frames": frames,
           "gpu_ms_statistic": "median of the timed frames",
           "gpu_ms_frame_median": float(np.median(per_frame)), "gpu_ms_p99": float(np.percentile(per_frame, 99)),
           "gpu_ms_worst_frame": float(per_frame.max()), "worst_over_median": float(per_frame.max() / np.median(per_frame)),
           "slowest_frames": [{"frame": int(i), "ms": round(float(per_frame[i]), 3),
                               "steps_ms": {k: round(1e3 * acc[k][i], 3) for k in steps}} for i in np.argsort(-per_frame)[:3]],
           "sweep_points": int(len(cloud)), "features": {k: int(len(v)) for k, v in feat.items()},
           "scan_points_after_voxel_grid": int(len(dc) + len(ds)), "map_points": fm.info()["n_corner"] + fm.info()["n_surf"],
           "scan_match_iterations": int(st.iterations),
           "pose_err_vs_ground_truth_m": float(np.abs(pose[3:] - gt[3:].astype(np.float32)).max())}
    if not cubes:
        built, after_all, _ = ctx.lazy_trees()
        if built > 0 and after_all == 0:
            # deferred trees: what surround_to_map builds per frame is the cell grids (bounding boxes, key sort, cell tables), no
            # kd-tree; priced as the bytes that must move -- every point read and written once, every cell of the tables
            # written and scanned -- over the step's wall time
            n_pts = len(sur_c) + len(sur_s)
            info_ = ctx.map_info()
            cells = ctx.grid_cells()  # (corner, surf) cells of the two tables
            # what must move: every point read and written once (2 x 16 B), every cell of the two tables written once (4 B)
            alg = 2.0 * 16.0 * n_pts + 4.0 * float(sum(cells))
            res["search_structure_build"] = {
                "what": "cell grids of the surround (lslam_map_defer_trees): no kd-tree is built unless a frame needs one",
                "ms": gpu["surround_to_map"], "points": n_pts, "cells": [int(c) for c in cells], "trees_built_after_all": int(after_all),
                "bound": "latency", "bound_detail": "segment tables, gather, one bounding-box round trip, then per type count / scan / scatter / rank (4 launches); the step's wall time includes two host waits",
                "alg_bytes": alg, "achieved": alg / (gpu["surround_to_map"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": alg / (gpu["surround_to_map"] * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                "kd_depth_reported": int(max(info_.depth_corner, info_.depth_surf))}
            # HBM-side traffic of the build's kernels from the committed counter passes (tools/profile_frame.sh: FETCH_SIZE /
            # WRITE_SIZE per kernel name and launch; two launches of each per frame, one per feature type), not measured in this run
            pmc = newest_profile("frame_pmc_by_kernel.csv")
            if pmc:
                fw = {}
                for line in open(os.path.join(ROOT, pmc)):
                    m_ = re.match(r'p\d+,"(grid_(?:bbox|count|scan|scatter|rank)_kernel)",(FETCH_SIZE|WRITE_SIZE),\d+,([0-9.e+]+),', line)
                    if m_:
                        fw[(m_.group(1), m_.group(2))] = float(m_.group(3))
                if fw:
                    tr = sum((2.0 if c == "FETCH_SIZE" else 1.0) * v for (k, c), v in fw.items()) * 1024.0 * 2.0
                    res["search_structure_build"]["traffic"] = tr
                    res["search_structure_build"]["traffic_over_alg_bytes"] = tr / alg
                    res["search_structure_build"]["traffic_source"] = "%s: sum over grid_bbox / count / scan / scatter / rank of (2 x FETCH_SIZE + WRITE_SIZE) x 1024 per launch, two launches each per frame" % pmc
        else:
            res["tree_build"] = tree_build_roofline(gpu["surround_to_map"], len(sur_c), len(sur_s), np)
        # The same frame the way the reference's nodelets run it: the registration node (feature extraction, the VoxelGrid of
        # the features) is its own thread with its own context, so its work on frame k overlaps the mapping node's
        # update + surround -> kd-trees of frame k (which depend on the map after frame k - 1 and on the pose prior only):
        # frame = max(extract + voxel, update + trees) + scan match + addFeatureCloud.
        import queue
        import threading
        ctx_reg = pkg.Context(ctx.device)
        qin, qout = queue.Queue(), queue.Queue()

        def registration():
            while True:
                job = qin.get()
                if job is None:
                    return
                f_ = pkg.scan_registration.extract_features(ctx_reg, cloud, ranges)
                qout.put(pkg.voxel_grid2(ctx_reg, f_["less_sharp"], f_["less_flat"], 1.0))
        th = threading.Thread(target=registration, daemon=True)
        # two Python threads share the interpreter lock; its default hand-over interval is 5 ms -- longer than two frames.  (A C++
        # host has no such lock; the library calls themselves run without it.)
        switch_interval = sys.getswitchinterval()
        sys.setswitchinterval(5e-5)
        th.start()
        quiet_gc()
        ov = []
        OV_WARM = 20  # the registration context's first frames allocate its staging, queues and signals (a one-off 8 ms stall within the first dozen frames)
        for f in range(frames + OV_WARM):
            t0 = time.perf_counter()
            qin.put(1)
            fm.update(gt[3:].astype(np.float32))
            fm.surround_to_map()
            dc2, ds2 = qout.get()
            status2, pose2, st2 = ctx.scanmatch_scan(dc2, ds2, init, opts)
            fm.add_feature_cloud(dc2, ds2, T)
            if f >= OV_WARM:
                ov.append(time.perf_counter() - t0)
        # ... and the two nodes free-running, as nodelets do: the registration node is already on sweep k + 1 while the mapping
        # node handles sweep k (a queue of one between them).  The number is the PERIOD of the slower node -- frames per second
        # of the pair -- not a frame's latency (that is the overlapped figure above plus nothing: a frame still passes through both)
        pl = []
        qin.put(1)
        for f in range(frames + OV_WARM):
            t0 = time.perf_counter()
            dc3, ds3 = qout.get()
            qin.put(1)
            fm.update(gt[3:].astype(np.float32))
            fm.surround_to_map()
            status3, pose3, st3 = ctx.scanmatch_scan(dc3, ds3, init, opts)
            fm.add_feature_cloud(dc3, ds3, T)
            if f >= OV_WARM:
                pl.append(time.perf_counter() - t0)
        qout.get()  # the sweep the registration node was ahead by
        qin.put(None)
        th.join()
        sys.setswitchinterval(switch_interval)
        ctx_reg.close()
        res["pipelined"] = {"ms_per_frame": 1e3 * float(np.median(pl)), "frames_per_s": 1.0 / float(np.median(pl)), "ms_p99": 1e3 * float(np.percentile(pl, 99)),
                            "ms_worst_frame": 1e3 * float(max(pl)), "frames": len(pl),
                            "schedule": "registration node one sweep ahead of the mapping node (queue of one): the period of the slower node",
                            "pose_err_vs_ground_truth_m": float(np.abs(pose3[3:] - gt[3:].astype(np.float32)).max())}
        res["overlapped"] = {"gpu_ms_per_frame": 1e3 * float(np.median(ov)), "gpu_ms_p99": 1e3 * float(np.percentile(ov, 99)),
                             "gpu_ms_worst_frame": 1e3 * float(max(ov)), "worst_over_median": float(max(ov) / np.median(ov)), "frames": len(ov), "slowest_frame_index": int(np.argmax(ov)),
                             "schedule": "registration thread (extract_features + voxel_grid, own context) beside update + "
                                         "surround_to_map; then scan_match, add_feature_cloud -- the reference's nodelet split "
                                         "(MultiScanRegistration | LaserMapping)",
                             "pose_err_vs_ground_truth_m": float(np.abs(pose2[3:] - gt[3:].astype(np.float32)).max())}
    res["deferred_trees"] = dict(zip(("maps_set_without_trees", "trees_built_after_all", "pending_now"), ctx.lazy_trees()))
    ctx.defer_trees(False)
    if cubes:
        res["cube_trees_built_reused_per_frame"] = [[int(b), int(r)] for b, r in trees]
        res["variant"] = "C: per-cube trees kept between frames (FeatureMap::scanMatchScan)"
        fm.close()
        return res
    if with_cpu:
        from oracle_lib import Oracle
        o = Oracle(native=True)
        ofm = o.feature_map(21, 21, 11)
        ofm.setup_filter_size(0.2, 0.4, 0.6)
        ofm.update(gt[3:].astype(np.float32))
        ofm.add_feature_cloud(sur_c, sur_s, np.eye(4, dtype=np.float32))
        t0 = time.perf_counter()
        ofeat = o.extract_features(cloud, ranges)
        t1 = time.perf_counter()
        odc, ods = o.voxel_grid(ofeat["less_sharp"], 1.0), o.voxel_grid(ofeat["less_flat"], 1.0)
        t2 = time.perf_counter()
        ofm.update(gt[3:].astype(np.float32))
        t3 = time.perf_counter()
        oc, os_ = ofm.get_surround_feature()
        t4 = time.perf_counter()
        ok, opose, ost = o.scanmatch_scan(oc, os_, odc, ods, init)  # kd-trees rebuilt inside (quirk Q4)
        t5 = time.perf_counter()
        ofm.add_feature_cloud(odc, ods, T)
        t6 = time.perf_counter()
        cpu = {k: 1e3 * d for k, d in zip(("extract_features", "voxel_grid", "update", "surround", "scan_match_incl_tree_build",
                                            "add_feature_cloud"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5))}
        res["cpu_ms"] = cpu
        res["cpu_ms_per_frame"] = sum(cpu.values())
        res["cpu"] = {"cores": 1, "kind": "port", "sample": "one frame of the same steps in the oracle"}
        res["pose_diff_gpu_vs_cpu_m"] = float(np.abs(opose[3:] - pose_first[3:]).max())
    fm.close()
    return res


def final_feature_map_leg(pkg, synth, synth_gpu, lidar, device, np, n_keyframes=300):
    """Graph::getFinalFeatureMap (pose_graph/graph.cpp:150-199, the end of Graph::save): the reference's own many-keyframe
    workload -- SEQUENTIAL: keyframe k is scan-matched against a map that already holds keyframes 0 .. k-1 (update ->
    surround -> VoxelGrid 0.2 / 0.3 -> scanMatchScan with the bool -> addFeatureCloud iff matched).  A bounded sample of the
    pose-graph leg's 5 000 keyframes: consecutive keyframes 0.26 m apart on the loop, VLP-16 sweeps ray cast at them, estimates
    = the truth plus what an optimised graph leaves (a few centimetres).  With the bootstrap (the reference as written never
    adds the first keyframe: the-cooper-mapper_amd/graph.py)."""
    ctx = pkg.Context(device)
    traj = synth_gpu.loop_trajectory(5000)
    rng = np.random.default_rng(77)
    kfs = []
    for k in range(n_keyframes):
        g = traj[k]
        c, s = lidar.scan(g, 16, 1800, seed=555000 + k)
        est = ctx.pose_to_isometry(g.astype(np.float32)).astype(np.float64)
        est[:3, 3] += rng.normal(0.0, 0.02, 3)
        kfs.append(pkg.KeyFrame(est, 0.26 * k, c, s, frame_id=k))
    graph = pkg.Graph(device=device, ctx=ctx)
    quiet_gc()
    t0 = time.perf_counter()
    res = graph.get_final_feature_map(ctx, cube_dims=(21, 21, 11), bootstrap=True, keyframes=kfs)
    dt = time.perf_counter() - t0
    info = res["map"].info()
    gt_err = max(float(np.linalg.norm(p[:3, 3] - traj[k][3:6])) for k, p in enumerate(res["poses"]))
    res["map"].close()
    ctx.close()
    return {"keyframes": n_keyframes, "keyframes_per_s": n_keyframes / dt, "ms_per_keyframe": 1e3 * dt / n_keyframes,
            "matched": int(sum(res["matched"])), "added": int(res["added"]), "points_per_keyframe": int(np.mean([len(k.corner_cloud) + len(k.surf_cloud) for k in kfs])),
            "map_points": int(info["n_corner"] + info["n_surf"]), "pose_err_vs_ground_truth_m": gt_err,
            "workload": "Graph::getFinalFeatureMap over %d consecutive keyframes (0.26 m apart) of the 5 000-keyframe loop, 16 x 1800 sweeps, "
                        "sequential: each keyframe matched against the map of those before it" % n_keyframes}


def sweep_pipeline_leg(pkg, synth, ctx, rings, np):
    """The whole per-sweep chain on the device, raw driver cloud in, map pose out:
    MultiScanRegistration::process -> extractFeatures -> LaserOdometry::process ->
    LaserMapping::process (the-cooper-mapper_amd/pipeline.py), milliseconds per stage.  The feature clouds go from the
    extraction kernels to the odometry node in HBM (lslam_fset), the node's last clouds stay there (lslam_odom); what
    the mapping node subscribes to leaves through a ring of page-locked buffers."""
    lo, hi = (-15.0, 15.0) if rings == 16 else (-24.9, 2.0)
    world = synth.World(half_extent=175.0)
    odo = pkg.DeviceLaserOdometry(ctx)
    mapper = pkg.LaserMapping(ctx, cube_dims=(21, 21, 11))
    sr = pkg.scan_registration
    fsets = [sr.FeatureSet(ctx) for _ in range(2)]
    acc = {"register": 0.0, "extract": 0.0, "odometry": 0.0, "mapping": 0.0}
    n = 0
    raws = []
    for k in range(28):  # consecutive sweeps of a moving sensor
        gt = (0.0, 0.0, 0.3 + 0.01 * k, 3.0 + 0.4 * k, -2.0 + 0.15 * k, synth.SENSOR_HEIGHT)
        _, _, _, cloud, _ = synth.make_scan(world, rings, 1800, gt_pose=gt, seed=300 + k, full=True)
        ring = np.floor(cloud[:, 3]).astype(np.int64)
        raws.append(cloud[np.lexsort((ring, -(cloud[:, 3] - ring)))])  # arrival order of a clockwise sweep
    per_sweep = []
    warm = 4  # the first sweeps size every buffer of the three nodes (page-locked rings, map arrays)
    for k, raw in enumerate(raws):
        quiet_gc()
        t0 = time.perf_counter()
        reg, rr = sr.multiscan_register(ctx, raw, lo, hi, rings)
        t1 = time.perf_counter()
        sr.extract_features_dev(ctx, reg, rr, fsets[k & 1])
        t2 = time.perf_counter()
        T = odo.process(fsets[k & 1])
        t3 = time.perf_counter()
        if T is not None:
            M = mapper.process(odo.last_corner, odo.last_surf, T)
        t4 = time.perf_counter()
        if k >= warm:
            for key, d in zip(acc, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                acc[key] += d
            per_sweep.append({"odometry_ms": 1e3 * (t3 - t2), "iterations": int(odo.last_stats.iterations),
                              "loop_gpu_ms": float(odo.last_stats.gpu_ms_total)})
            n += 1
    mapper.feature_map.close()
    fallbacks = int(odo.last_ostats.tree_fallbacks)
    odo.close()
    for f in fsets:
        f.close()
    ms = {k: 1e3 * v / n for k, v in acc.items()}
    its = [p["iterations"] for p in per_sweep]
    res = {"rings": rings, "points_per_sweep": int(len(raw)), "ms": ms, "ms_per_sweep": sum(ms.values()),
           "sweeps_per_s": 1e3 / sum(ms.values()), "sweeps_timed": n,
           "odometry": {"node": "device-resident (lslam_odom): hashed cell grids, five iterations per launch",
                        "iterations_per_sweep": its, "ms_by_sweep": [round(p["odometry_ms"], 4) for p in per_sweep],
                        "loop_gpu_ms_by_sweep": [round(p["loop_gpu_ms"], 4) for p in per_sweep],
                        "ms_p50": float(np.median([p["odometry_ms"] for p in per_sweep])),
                        "ms_worst": float(max(p["odometry_ms"] for p in per_sweep)), "tree_fallbacks": fallbacks},
           "travelled_m": float(np.linalg.norm(M[:3, 3]))}
    # the three nodelets on three threads: as a C++ program over the mirrors of include/ (what a maintainer's nodelets are; no
    # interpreter lock between the nodes), and as three Python threads over the ctypes binding
    try:
        res["node_threads"] = sweep_pipeline_threads_cpp(pkg, rings, np, lo, hi, raws)
    except Exception as e:
        res["node_threads"] = {"error": repr(e)[:300]}
    try:
        res["node_threads_python"] = sweep_pipeline_threads(pkg, synth, rings, np, lo, hi, raws)
    except Exception as e:
        res["node_threads_python"] = {"error": repr(e)}
    if "ms_per_sweep" not in res["node_threads"] and "ms_per_sweep" in res["node_threads_python"]:
        res["node_threads"] = dict(res["node_threads_python"], host="python threads (the C++ program did not build or run: %s)" % res["node_threads"].get("error"))
    return res


def sweep_pipeline_threads_cpp(pkg, rings, np, lo, hi, raws):
    """tools/cpp/node_threads.cpp: registration, odometry and mapping as three std::threads with a context each over the C ABI
    and the header-only mirrors -- built here with g++ against the library in the tree, fed the same raw sweeps."""
    import subprocess
    import tempfile
    tmp = tempfile.mkdtemp(prefix="lslam_nodes_")
    path = os.path.join(tmp, "sweeps.bin")
    with open(path, "wb") as f:
        f.write(np.uint32(rings).tobytes() + np.float32(lo).tobytes() + np.float32(hi).tobytes() + np.uint32(len(raws)).tobytes())
        for r in raws:
            a = np.ascontiguousarray(r[:, :4], np.float32)
            f.write(np.uint32(len(a)).tobytes())
            f.write(a.tobytes())
    exe = os.path.join(tmp, "node_threads")
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "cpp", "node_threads.cpp"),
                           "-o", exe, "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir, "-lpthread"], timeout=300)
    warm = 8
    seq = subprocess.run([exe, path, str(warm), "seq"], capture_output=True, text=True, timeout=300)  # the same calls from ONE thread
    seq_ms = None
    if seq.returncode == 0 and "SEQUENTIAL" in seq.stdout:
        w = seq.stdout.split()
        seq_ms = float(w[w.index("ms_per_sweep") + 1])
    best = None
    for _ in range(2):  # (the first run also pages the program and its buffers in)
        out = subprocess.run([exe, path, str(warm)], capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            raise RuntimeError(out.stderr[-300:])
        w = [l for l in out.stdout.splitlines() if l.startswith("NODE_THREADS")][0].split()
        v = {w[i]: float(w[i + 1]) for i in range(1, len(w) - 1, 2)}
        if best is None or v["ms_per_sweep"] < best["ms_per_sweep"]:
            best = v
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return {"threads": 3, "host": "C++ (tools/cpp/node_threads.cpp: std::thread per nodelet over include/lslam_pipeline.hpp)", "ms_per_sweep": best["ms_per_sweep"],
            "sweeps_per_s": 1e3 / best["ms_per_sweep"], "sweeps_timed": int(best["sweeps_timed"]), "travelled_m": best["travelled_m"],
            "busy_ms_per_sweep": {"registration": best["registration_busy_ms"], "odometry": best["odometry_busy_ms"], "mapping": best["mapping_busy_ms"]},
            "one_thread_ms_per_sweep": seq_ms,
            "note": "timed from the sweep the LAST node (mapping) takes up after the warm-up to the end of its last one: the period is the "
                    "slowest node's busy time; one_thread_ms_per_sweep = the same program running the three nodes from one thread"}


def sweep_pipeline_threads(pkg, synth, rings, np, lo, hi, raws):
    """The same chain the way the reference runs it: scan registration, odometry and mapping are three
    nodelets with their own threads (nodelets.xml; LaserOdometry.cpp spin(), LaserMapping.cpp:27-37),
    joined by the /laser_cloud_* and /laser_odom_to_init topics.  Three host threads with a context each
    (one call in flight per context), queues between them; ctypes releases the GIL during the calls, the
    three streams share the GPU.  Registration -> odometry carries feature sets in HBM (a pool of them goes
    round), odometry -> mapping page-locked views.  Throughput of the chain, not the latency of a sweep."""
    import queue
    import threading
    sweeps = len(raws)
    ctx_r, ctx_o, ctx_m = pkg.Context(0), pkg.Context(0), pkg.Context(0)
    odo = pkg.DeviceLaserOdometry(ctx_o, publish_buffers=8)
    mapper = pkg.LaserMapping(ctx_m, cube_dims=(21, 21, 11))
    sr = pkg.scan_registration
    q1, q2 = queue.Queue(maxsize=2), queue.Queue(maxsize=2)
    pool = queue.Queue()
    fsets = [sr.FeatureSet(ctx_r) for _ in range(5)]  # one being filled, two queued, one being consumed, one spare
    for f in fsets:
        pool.put(f)
    out, err = [], []
    warm = 8  # every feature set of the pool, every buffer of the publishing ring and the map's arrays have been sized by then
    stamps = {}

    def registration():  # MultiScanRegistration nodelet: raw sweep -> feature clouds
        try:
            for k, raw in enumerate(raws):
                reg, rr = sr.multiscan_register(ctx_r, raw, lo, hi, rings)
                f = pool.get()
                sr.extract_features_dev(ctx_r, reg, rr, f)
                q1.put(f)
        except Exception as e:
            err.append(e)
        q1.put(None)

    def odometry():  # LaserOdometry nodelet
        try:
            while True:
                f = q1.get()
                if f is None:
                    break
                T = odo.process(f)
                pool.put(f)
                if T is not None:
                    q2.put((odo.last_corner, odo.last_surf, T))
        except Exception as e:
            err.append(e)
        q2.put(None)

    def mapping():  # LaserMapping nodelet
        try:
            while True:
                item = q2.get()
                if item is None:
                    break
                if len(out) == warm - 1:  # (the clock starts where the LAST node takes up its warm-th sweep: the first sweeps size every buffer)
                    stamps["t0"] = time.perf_counter()
                out.append(mapper.process(*item))
        except Exception as e:
            err.append(e)
        stamps["t1"] = time.perf_counter()
    quiet_gc()
    th = [threading.Thread(target=f) for f in (registration, odometry, mapping)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    mapper.feature_map.close()
    odo.close()
    for f in fsets:
        f.close()
    for c in (ctx_r, ctx_o, ctx_m):
        c.close()
    if err:
        raise err[0]
    n = sweeps - warm
    dt = stamps["t1"] - stamps["t0"]
    return {"threads": 3, "ms_per_sweep": 1e3 * dt / n, "sweeps_per_s": n / dt, "sweeps_timed": n,
            "travelled_m": float(np.linalg.norm(out[-1][:3, 3]))}


def cpu_baseline(surround, scans, inits, gpu_poses, gpu_stats, n_scans, np):
    """The oracle (port of the reference's single-threaded path, -O3 -march=native
    -ffp-contract=off) on a bounded sample of the SAME workload: the first `n_scans` scans of the step
    against the same map (the surround the timed region used), full scanMatchScan calls including the
    per-call kd-tree rebuild (quirk Q4), one core -- the reference's hot path is single-threaded."""
    from oracle_lib import Oracle
    o = Oracle(native=True)
    map_c, map_s = surround
    t0 = time.perf_counter()
    pt = 0
    t_build = t_sweep = 0.0
    its = 0
    dpos, drot = 0.0, 0.0
    its_equal = rows_equal = True
    for k in range(n_scans):
        ok, pose, st = o.scanmatch_scan(map_c, map_s, scans[k][0], scans[k][1], inits[k])
        its_equal = its_equal and st.iterations == gpu_stats[k].iterations
        # match counts of the last sweep: equal up to a handful of threshold-adjacent points (the two paths' poses differ
        # in the last bits from the second iteration on: different summation order of A^T A)
        rows_equal = rows_equal and all(abs(int(a) - int(b)) <= max(2, int(1e-4 * max(a, b))) for a, b in
                                        ((st.n_rows, gpu_stats[k].n_rows), (st.n_line, gpu_stats[k].n_line), (st.n_plane, gpu_stats[k].n_plane)))
        pt += st.point_residuals
        t_build += st.t_build
        t_sweep += st.t_sweep
        its += st.iterations
        dpos = max(dpos, float(np.abs(pose[3:] - gpu_poses[k][3:]).max()))
        drot = max(drot, float(np.abs(pose[:3] - gpu_poses[k][:3]).max()))
    dt = time.perf_counter() - t0
    # the same loop with the sweep spread over all host cores (OpenMP) -- a generous
    # upper bound for a CPU, NOT what the reference does (its hot path is one thread)
    all_cores = None
    try:
        oo = Oracle(native="omp")
        oo.scanmatch_scan(map_c, map_s, scans[0][0], scans[0][1], inits[0])  # threads up
        t1 = time.perf_counter()
        ok2, pose2, st2 = oo.scanmatch_scan(map_c, map_s, scans[0][0], scans[0][1], inits[0])
        dt2 = time.perf_counter() - t1
        all_cores = {"value": st2.point_residuals / dt2, "sweep_only_value": st2.point_residuals / st2.t_sweep if st2.t_sweep > 0 else None,
                     "cores": os.cpu_count(), "kind": "port, OpenMP over the scan points -- not reference behaviour"}
    except Exception as e:
        all_cores = {"error": repr(e)}
    return {
        "all_cores": all_cores,
        "value": pt / dt,
        "unit": "point-residuals/s",
        "cores": 1,
        "kind": "port",
        "sample": "%d of the step's scans: full scanMatchScan calls against the same %d-point map (%d GN iterations "
                  "each on average), kd-tree rebuilt per call as the reference does" % (n_scans, len(map_c) + len(map_s), its // max(1, n_scans)),
        "seconds": dt,
        "sweep_only_value": pt / t_sweep if t_sweep > 0 else None,
        "tree_build_s_per_call": t_build / n_scans,
        "host_cpus": os.cpu_count(),
        "pose_diff_gpu_vs_cpu_m": dpos,
        "pose_diff_gpu_vs_cpu_rad": drot,
        "iterations_equal": bool(its_equal),
        "rows_equal": bool(rows_equal),
        "iterations": its // max(1, n_scans),
    }


if __name__ == "__main__":
    main()
