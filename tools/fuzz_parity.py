#!/usr/bin/env python3
"""Seeded parity fuzz on the GPU box: many random problems (worlds, ring counts, poses, map densities, voxel-filtered maps
with lattice-like coordinates) through the sweep taps and the whole scanMatchScan loop, device against oracle, the lane search through
both traversal-stack shapes (the single-scan kernel and the batch kernel sweep_kernel<256,true,false,12>).
Bit-exact: neighbour indices, distances, flags, coefficients; the loop: status / iterations / rows equal, pose within
1e-4 m / 1e-5 rad.  N_SEEDS (default 24) problems; exits non-zero on the first mismatch.

    python tools/fuzz_parity.py
"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("the-cooper-mapper_amd")
synth = importlib.import_module("the-cooper-mapper_amd.synth")
from oracle_lib import Oracle

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
o = Oracle()
ctx = pkg.Context(0)
n_seeds = int(os.environ.get("N_SEEDS", "24"))
bad = 0
for seed in range(n_seeds):
    rng = np.random.default_rng(1000 + seed)
    rings = int(rng.choice([8, 16, 32]))
    steps = int(rng.choice([300, 600, 900]))
    half = float(rng.choice([40.0, 60.0, 90.0]))
    pr = synth.make_problem(rings=rings, azimuth_steps=steps, world_half=half, seed=seed % 7)
    mc, ms = pr["map_corner"], pr["map_surf"]
    if seed % 3 == 1:  # voxel-filtered map: centroids on a near-lattice, many equal coordinates
        mc, ms = pkg.voxel_grid(ctx, np.c_[mc[:, :3], np.zeros(len(mc), np.float32)], 0.2)[:, :3], \
                 pkg.voxel_grid(ctx, np.c_[ms[:, :3], np.zeros(len(ms), np.float32)], 0.4)[:, :3]
    if seed % 3 == 2:  # coordinates rounded to 1 cm: exact distance ties
        mc, ms = np.round(mc, 2).astype(np.float32), np.round(ms, 2).astype(np.float32)
    mc = np.ascontiguousarray(mc, np.float32); ms = np.ascontiguousarray(ms, np.float32)
    init = synth.perturb_pose(pr["gt_pose"], seed=seed, dt=float(rng.uniform(0.05, 0.5)), dr_deg=float(rng.uniform(0.2, 3.0)))
    ctx.map_set(mc, ms)
    ctx.scan_set(pr["corner"], pr["surf"])
    tc, ts = o.kdtree(mc), o.kdtree(ms)
    for pose in (init, pr["gt_pose"]):
        for mode in (1 | 0x100, 1 | 0x200, 2, 3):  # lane search through the deep and the shallow (batch) stack shape, packet search, grid probe
            g = ctx.sweep(pose, jtj_mode=1, search_mode=mode)
            r = o.sweep(tc, ts, pr["corner"], pr["surf"], pose)
            for key in ("idx", "flags"):
                if not np.array_equal(g[key], r[key]):
                    bad += 1; print("seed", seed, "mode", mode, key, "differs at", np.argwhere(g[key] != r[key])[:3].tolist())
            for key in ("d2", "coeff"):
                if not np.array_equal(bits(g[key]), bits(r[key])):
                    bad += 1; print("seed", seed, "mode", mode, key, "differs at", np.argwhere(bits(g[key]) != bits(r[key]))[:3].tolist())
    ok, opose, ost = o.scanmatch_scan(mc, ms, pr["corner"], pr["surf"], init)
    poses = []
    for stack in (0x100, 0x200):  # the whole loop through both stack shapes
        opts = ctx.default_opts()
        opts.search_mode = 1 | stack
        status, pose, st = ctx.run(init, opts)
        poses.append(pose)
        # last-sweep row counts: equal up to threshold-adjacent points (the poses differ in the last bits from iteration 2 on)
        if st.iterations != ost.iterations or abs(st.n_rows - ost.n_rows) > 2 or np.abs(pose[3:] - opose[3:]).max() > 1e-4 or np.abs(pose[:3] - opose[:3]).max() > 1e-5:
            bad += 1; print("seed", seed, "stack", hex(stack), "loop differs", st.iterations, ost.iterations, st.n_rows, ost.n_rows, np.abs(pose - opose).max())
    if not np.array_equal(bits(poses[0]), bits(poses[1])):
        bad += 1; print("seed", seed, "deep and shallow stack loops differ in bits")
    # the certificate sweep (forced: a single scan would not take it), with its default thresholds and with every scan testing
    # certificates from its second sweep on however far it moved: the same neighbours, so the same loop up to summation order
    for env in ({"knn_cert": 2}, {"knn_cert": 2, "cert_try_m": 1e9, "cert_track_m": 1e9}):
        opts = ctx.default_opts()
        opts.search_mode = 1 | 0x200
        for k, v in env.items():
            setattr(opts, k, v)
        q0 = ctx.cert_stats()[2]
        status, pose, st = ctx.run(init, opts)
        ran = ctx.cert_stats()[2] - q0
        # the bound every point carries for its next certificate: never above the true sixth squared distance of the position
        # it was taken at (scipy's kd-tree on the same map)
        from scipy.spatial import cKDTree
        nqc, nqs = len(pr["corner"]), len(pr["surf"])
        cq, clb = ctx.cert_state(nqc + nqs)
        for tree_pts, sl in ((mc, slice(0, nqc)), (ms, slice(nqc, nqc + nqs))):
            if len(tree_pts) < 6 or sl.stop == sl.start:
                continue
            d6 = cKDTree(tree_pts[:, :3].astype(np.float64)).query(cq[sl].astype(np.float64), k=6)[0][:, 5] ** 2
            have = clb[sl] > 0
            if have.any() and not (clb[sl][have] <= d6[have] * (1 + 1e-5) + 1e-9).all():
                bad += 1; print("seed", seed, "certificate sweep", env, "a kept bound exceeds the true sixth distance by", float((clb[sl][have] / d6[have]).max()))
        if st.iterations != ost.iterations or abs(st.n_rows - ost.n_rows) > 2 or np.abs(pose[3:] - poses[1][3:]).max() > 5e-6 or np.abs(pose[:3] - poses[1][:3]).max() > 5e-7 or (st.iterations > 1 and ran == 0):
            bad += 1; print("seed", seed, "certificate sweep", env, "differs", st.iterations, ost.iterations, st.n_rows, ost.n_rows, np.abs(pose - poses[1]).max(), ran)
    # the grid sweep (probe + proof, tree search for the rest): the same loop up to summation order
    opts = ctx.default_opts()
    opts.search_mode = 3
    g0 = ctx.grid_launches()
    status, pose, st = ctx.run(init, opts)
    if st.iterations != ost.iterations or abs(st.n_rows - ost.n_rows) > 2 or np.abs(pose[3:] - poses[1][3:]).max() > 2e-5 or np.abs(pose[:3] - poses[1][:3]).max() > 2e-6 or ctx.grid_launches() == g0:  # (a few ulps of a coordinate of tens of metres: the two sweeps group their sums differently)
        bad += 1; print("seed", seed, "grid sweep differs", st.iterations, ost.iterations, st.n_rows, ost.n_rows, np.abs(pose - poses[1]).max())
    # ... and every sweep of that loop as the production loop runs it (the first bounded by the gate, the later ones with the
    # probe clipped to the bound carried from the sweep before and the second pass started from it: LSLAM_SWEEP_FIRST /
    # _CARRIED) against the oracle's sweep at the same pose: flags and coefficients of every point, indices and distances of
    # every point the reference looks up (d2[4] < 5), bit for bit
    pose_k = np.asarray(init, np.float32)
    for k in range(8):
        if k > 0:
            opts.max_iterations = k
            status, pose_k, st_k = ctx.run(init, opts)
            if st_k.iterations < k or st_k.converged:
                break
        g = ctx.sweep(pose_k, jtj_mode=1, search_mode=3 | (0x400 if k > 0 else 0x800))
        r = o.sweep(tc, ts, pr["corner"], pr["surf"], pose_k)
        lk = (r["flags"] & 1) != 0
        if not (np.array_equal(g["flags"], r["flags"]) and np.array_equal(bits(g["coeff"]), bits(r["coeff"]))
                and np.array_equal(g["idx"][lk], r["idx"][lk]) and np.array_equal(bits(g["d2"])[lk], bits(r["d2"])[lk])):
            bad += 1; print("seed", seed, "grid loop, sweep", k, "differs from the oracle's sweep at the same pose")
    # the same map with its kd-trees deferred (lslam_map_defer_trees: grids only, the wide probe for what the 27-cell probe cannot
    # prove): the same loop up to summation order -- the rounded maps hold exact ties, for which the call must build the trees
    # after all and still agree
    c2 = pkg.Context(0)
    try:
        c2.defer_trees(True)
        c2.map_set(mc, ms)
        c2.scan_set(pr["corner"], pr["surf"])
        status, pose, st = c2.run(init, c2.default_opts())
        sets, builds, pending = c2.lazy_trees()
        deferred = sets == 1  # (a map too small for the guard or too large for the grid is built at once)
        if st.iterations != ost.iterations or abs(st.n_rows - ost.n_rows) > 2 or np.abs(pose[3:] - poses[1][3:]).max() > 2e-5 or np.abs(pose[:3] - poses[1][:3]).max() > 2e-6 or (deferred and pending and c2.grid_launches() == 0):
            bad += 1; print("seed", seed, "deferred trees differ", st.iterations, ost.iterations, st.n_rows, ost.n_rows, np.abs(pose - poses[1]).max(), (sets, builds, pending))
    finally:
        c2.close()
    print("seed %2d rings %2d steps %3d half %3.0f map %6d+%6d scan %5d: %s" % (seed, rings, steps, half, len(mc), len(ms), len(pr["corner"]) + len(pr["surf"]), "ok" if not bad else "MISMATCH"), flush=True)
    if bad:
        sys.exit(1)
print("fuzz: %d problems, no mismatch" % n_seeds)
