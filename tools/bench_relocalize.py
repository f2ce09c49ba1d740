#!/usr/bin/env python3
"""Global re-localisation (lslam_reloc_*) on the bench map: the surround of the 10k-frame voxel map of the 600 x 600 m world
(BASELINE configs[1], built as bench.py builds it), one seeded 64 x 1800 sweep near the end of the loop, yaw every 2 degrees x
a 100 x 100 m box of positions at 1 m around a point (0.37, -0.41) m off the ground truth, voxel 2.0 m, no initial pose.

Reports, from LaserLocalization.relocalize run --repeats times after one warm-up call (the occupancy sets are built by the
warm-up, as a node builds them once per map): the median host time of the coarse stage (scan filters, scoring, selection: one
wait) with hypotheses/s and point-probes/s, the median of the refinement, the winner's error against the ground truth, and the
same scoring by the numpy restatement (tests/relocalization_ref.py) on a 3 x 3 sub-box as the CPU figure -- whose scores must
equal the device's, or the script exits non-zero.  Prints a table, writes it to --out and ends with one JSON line."""
import argparse
import glob
import importlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DIMS = (21, 21, 11)


def next_round_file():
    rounds = [int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_*"))
              for m in [re.match(r"r(\d\d)_", os.path.basename(f))] if m]
    return os.path.join(ROOT, "profiles", "r%02d_relocalize.txt" % (max(rounds, default=0) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-frames", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yaw-step", type=float, default=2.0)
    ap.add_argument("--half-extent", type=float, default=50.0)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--voxel", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    import synth_gpu
    import localization_ref as lr
    import relocalization_ref as rr
    from oracle_lib import Oracle

    ctx = pkg.Context(0)
    world = synth.World(half_extent=300.0, wall_half=295.0, pole_pitch=2.5)
    lidar = synth_gpu.GpuLidar(world, 0)
    traj = synth_gpu.loop_trajectory(args.map_frames)
    t0 = time.perf_counter()
    fm, mapstats = synth_gpu.build_voxel_map(pkg, ctx, lidar, traj, rings=16)
    fm.update(traj[-1][3:].astype(np.float32))
    map_c, map_s = fm.get_surround_feature()
    fm.close()
    build_s = time.perf_counter() - t0
    node = pkg.LaserLocalization(ctx, *DIMS)
    node.set_map(map_c, map_s, filter=False)

    gt = synth_gpu.loop_trajectory(100000)[-40].copy()
    gt[3:5] += (0.6, -0.3)
    gt[2] += 0.1
    corner, surf = lidar.scan(gt, 64, 1800, seed=900123)
    corner, surf = np.ascontiguousarray(corner, np.float32), np.ascontiguousarray(surf, np.float32)
    rot = pkg.yaw_sweep(args.yaw_step, 2)
    centre = (gt[3] + 0.37, gt[4] - 0.41)
    pos = pkg.grid_positions(centre, args.half_extent, args.step, gt[5])
    assert node.process(corner, surf, np.eye(4, dtype=np.float32), 1_000_000_000) is None  # no pose: the sweep is dropped

    kw = dict(voxel=args.voxel)
    res = node.relocalize(corner, surf, rot, pos, **kw)  # warm-up: the occupancy sets, the scratch, the kernels' code objects
    coarse, refine = [], []
    for _ in range(args.repeats):
        res = node.relocalize(corner, surf, rot, pos, **kw)
        coarse.append(res.ms_coarse)
        refine.append(res.ms_refine)
    ms_c, ms_r = float(np.median(coarse)), float(np.median(refine))
    H, P = res.n_hypotheses - res.skipped, sum(res.n_scored)
    lines = []
    say = lambda s: (lines.append(s), print(s))
    say("map: %d frames -> surround %d corner + %d surf points (built in %.1f s); occupancy sets %d + %d voxels of %.1f m" %
        (mapstats["frames"], len(map_c), len(map_s), build_s, res.occupied_voxels[0], res.occupied_voxels[1], args.voxel))
    say("sweep: 64 x 1800, %d + %d feature points, %d + %d after the scan filters" %
        (len(corner), len(surf), res.n_points[0], res.n_points[1]))
    say("hypotheses: %d yaws x %d positions = %d (%d refused at the edge), top list %d, %d candidates refined" %
        (len(rot), len(pos), res.n_hypotheses, res.skipped, res.n_selected, len(res.candidates)))
    say("| stage | median of %d | min | max | rate |" % args.repeats)
    say("|---|---|---|---|---|")
    say("| coarse (filters + scoring + selection, one wait) | %.2f ms | %.2f | %.2f | %.3g hypotheses/s, %.3g point-probes/s |" %
        (ms_c, min(coarse), max(coarse), H / (ms_c * 1e-3), H * P / (ms_c * 1e-3)))
    say("| refinement (%d candidates, %d matches) | %.2f ms | %.2f | %.2f | |" %
        (len(res.candidates), sum(c.rounds for c in res.candidates), ms_r, min(refine), max(refine)))
    rc = 0
    if res.winner >= 0:
        w = res.candidates[res.winner]
        T = res.T
        yaw = np.arctan2(T[1, 0], T[0, 0])
        e_t = float(np.linalg.norm(w.pose[3:] - gt[3:]))
        e_y = float(abs((yaw - gt[2] + np.pi) % (2 * np.pi) - np.pi))
        hyp = pos[w.hypothesis % len(pos)]
        say("verdict: status %d accepted %d fraction %.3f; winner from hypothesis %.2f m off -> %.4f m, %.5f rad from the ground truth; runner-up %s" %
            (res.status, res.accepted, res.fraction, float(np.linalg.norm(hyp[:2] - gt[3:5])), e_t, e_y,
             "none" if res.runner_up < 0 else "candidate %d (%d rows against %d)" % (res.runner_up, res.candidates[res.runner_up].n_rows, w.n_rows)))
    else:
        e_t = e_y = float("nan")
        say("verdict: status %d, no candidate converged" % res.status)
        rc = 1
    # the CPU figure: the restatement on the 3 x 3 positions around the box's centre, every yaw
    ref = lr.RefLocalization(Oracle(), DIMS, 50.0, None)
    ref.set_map(map_c, map_s, filter=False)
    sets = rr.occupancy_sets(ref, args.voxel)
    k = int(round(args.half_extent / args.step))
    side = 2 * k + 1
    sub = np.array([(k + a) * side + (k + b) for a in (-1, 0, 1) for b in (-1, 0, 1)])
    Rs = np.stack([ctx.pose_to_isometry(np.array([r[0], r[1], r[2], 0, 0, 0], np.float32))[:3, :3] for r in rot])
    t0 = time.perf_counter()
    want, n = rr.scores(ref, corner, surf, Rs, pos[sub], args.voxel, sets=sets)
    cpu_s = time.perf_counter() - t0
    got, _, _, _ = node.reloc_scores(corner, surf, rot, pos[sub], **kw)
    same = bool(np.array_equal(got, want))
    cpu_rate = want.size * sum(n) / cpu_s
    say("numpy restatement, %d hypotheses of the 3 x 3 sub-box: %.2f s, %.3g point-probes/s on one core (scoring alone); scores equal the device's: %s" %
        (want.size, cpu_s, cpu_rate, same))
    if not same:
        rc = 1
    out = args.out or next_round_file()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print(json.dumps(dict(metric="relocalize", ms_coarse=ms_c, ms_refine=ms_r, hypotheses=int(res.n_hypotheses), points=int(P),
                          hypotheses_per_s=H / (ms_c * 1e-3), probes_per_s=H * P / (ms_c * 1e-3), cpu_probes_per_s=cpu_rate,
                          error_m=e_t, error_rad=e_y, accepted=int(res.accepted), scores_equal=same, out=os.path.relpath(out, ROOT))))
    node.close()
    ctx.close()
    sys.exit(rc)


if __name__ == "__main__":
    main()
