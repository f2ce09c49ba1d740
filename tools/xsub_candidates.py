#!/usr/bin/env python3
"""How many candidates does the clipped 27-cell probe of knn5_grid (csrc/lslam_grid.hpp) scan when the x axis of the cell
table is cut into S sub-cells per cell?  CPU count, numpy / scipy only, no GPU.

The workload is a reduced copy of the bench's: synth.World, surface samples at half the leaf size put through a VoxelGrid
(one centroid per 0.2 m corner / 0.4 m surf voxel), one 64 x 1800 scan in Morton order (0.25 m cells, as lslam_scanprep
orders it), and LATE-sweep bounds: the carried bound of a sweep after a centimetre step is the distance to the previous
five at the new position, at most the exact fifth distance plus the step,

    rb = (d5 + step) (1 + 1e-5) + GRID_CLIP_MARGIN_MIN.

Counted with the kernel's clip rule in fp32 (cell coordinate fl(fl(v - org) * inv_cx), y and z rows clipped in cells of c, the
x-extent in sub-cells of c / S: max(S (fxc - 1), floor(u - rbc S)) .. min(S (fxc + 1) + S - 1, floor(u + rbc S))):

  * candidates per point (mean over the points inside the sqrt(5) m gate with an interior cell),
  * the maximum per 64 consecutive points -- the rounds a wavefront's candidate loop runs,
  * lane use: candidates / (64 x rounds).

Usage: tools/xsub_candidates.py [--radius M] [--step M] [--cell C] [--S 1,2,3,4]
"""
import argparse
import importlib
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
synth = importlib.import_module("the-cooper-mapper_amd.synth")

F = np.float32
GRID_CLIP_MARGIN_MIN = F(3.0e-3)


def voxel_grid(pts, leaf):
    """pcl::VoxelGrid: the centroid of every occupied voxel."""
    key = np.floor(pts / leaf).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.ravel()
    n = inv.max() + 1
    out = np.zeros((n, 3))
    np.add.at(out, inv, pts)
    return (out / np.bincount(inv, minlength=n)[:, None]).astype(F)


def morton_order(pts):
    q = np.clip(pts[:, :3] * 4.0 + 512.0, 0, 1023).astype(np.uint32)

    def spread(v):
        v = v & 0x3FF
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    return np.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2), kind="stable")


def margin_cells(c):
    return int(2.2361 / c) + 3


def count_candidates(mp, q, rb, c, S):
    """Candidates per query of the bounded probe over a table with S x-sub-cells per cell.  mp, q: float32 (n, 3); rb:
    float32 clip radius per query (inf: unclipped).  Returns (candidates, interior)."""
    c = F(c)
    inv_c = F(1.0) / c
    inv_cx = F(S) / c
    org = mp.min(0) - F(margin_cells(c)) * c
    dims = (np.floor((mp.max(0) - org) * inv_c) + 1 + margin_cells(c)).astype(np.int64)
    nx = dims[0] * S

    def coord(v, a):
        return (v[:, a] - org[a]).astype(F) * (inv_cx if a == 0 else inv_c)
    mx = np.floor(coord(mp, 0)).astype(np.int64)
    my = np.floor(coord(mp, 1)).astype(np.int64)
    mz = np.floor(coord(mp, 2)).astype(np.int64)
    skey = np.sort(mx + nx * (my + dims[1] * mz))
    ufx, uy, uz = coord(q, 0), coord(q, 1), coord(q, 2)
    fxf = np.floor(ufx)
    fxc = np.floor_divide(fxf.astype(np.int64), S)  # the coarse cell IS fine div S
    fy, fz = np.floor(uy), np.floor(uz)
    inr = (fxc >= 1) & (fxc < dims[0] - 1) & (uy >= 1) & (uy < dims[1] - 1) & (uz >= 1) & (uz < dims[2] - 1)
    rbc = (rb * inv_c).astype(F)
    rbx = (rbc * F(S)).astype(F)
    with np.errstate(invalid="ignore"):
        xlo = np.maximum(S * (fxc - 1), np.floor((ufx - rbx).astype(F)))
        xhi = np.minimum(S * (fxc + 1) + S - 1, np.floor((ufx + rbx).astype(F)))
        ylo, yhi = np.maximum(fy - 1, np.floor((uy - rbc).astype(F))), np.minimum(fy + 1, np.floor((uy + rbc).astype(F)))
        zlo, zhi = np.maximum(fz - 1, np.floor((uz - rbc).astype(F))), np.minimum(fz + 1, np.floor((uz + rbc).astype(F)))
    xlo = np.where(inr, xlo, 0).astype(np.int64)
    xhi = np.where(inr, xhi, 0).astype(np.int64)
    cand = np.zeros(len(q), np.int64)
    iy, iz = np.where(inr, fy, 1).astype(np.int64), np.where(inr, fz, 1).astype(np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            jy, jz = iy + dy, iz + dz
            use = inr & (jy >= ylo) & (jy <= yhi) & (jz >= zlo) & (jz <= zhi)
            base = nx * (jy + dims[1] * jz)
            s = np.searchsorted(skey, base + xlo)
            e = np.searchsorted(skey, base + xhi + 1)
            cand += np.where(use, np.maximum(e - s, 0), 0)
    return cand, inr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=30.0, help="map radius around the origin [m]")
    ap.add_argument("--step", type=float, default=0.01, help="pose step of a late sweep [m]")
    ap.add_argument("--cell", type=float, default=0.6)
    ap.add_argument("--S", default="1,2,3,4")
    args = ap.parse_args()
    Ss = [int(s) for s in args.S.split(",")]
    world = synth.World()
    raw_c, raw_s = synth.make_map(world, 0.1, 0.2, radius=args.radius)
    maps = {"corner": voxel_grid(raw_c[:, :3].astype(np.float64), 0.2), "surf": voxel_grid(raw_s[:, :3].astype(np.float64), 0.4)}
    gt = (0.01, -0.015, 0.3, 3.0, -2.0, synth.SENSOR_HEIGHT)
    qc, qs, gt = synth.make_scan(world, 64, 1800, gt_pose=gt)
    R, t = synth.pose_to_Rt(gt)
    tot = {S: [0, 0, 0] for S in Ss}  # candidates, rounds x 64, points -- late sweeps, both types
    print("map radius %.0f m, cell %.2f m, late-sweep step %.3f m" % (args.radius, args.cell, args.step))
    for kind, scan in (("corner", qc), ("surf", qs)):
        mp = maps[kind]
        sp = scan[morton_order(scan)][:, :3].astype(np.float64)
        q = (sp @ R.T + t).astype(F)
        d, _ = cKDTree(mp.astype(np.float64)).query(q.astype(np.float64), k=5)
        d5 = d[:, 4]
        gate = d5 * d5 < 5.0
        rb = ((d5 + args.step) * (1.0 + 1.0e-5)).astype(F) + GRID_CLIP_MARGIN_MIN
        print("%-6s map %d points, scan %d points, %d inside the gate; d5 median %.3f p90 %.3f m; rb median %.3f m"
              % (kind, len(mp), len(q), gate.sum(), np.median(d5[gate]), np.percentile(d5[gate], 90), np.median(rb[gate])))
        nw = len(q) // 64
        for label, r in (("first sweep (unclipped)", np.full(len(q), np.inf, F)), ("late sweep", rb)):
            base = None
            for S in Ss:
                cand, inr = count_candidates(mp, q, r, args.cell, S)
                sel = gate & inr
                cw = np.where(sel, cand, 0)[:nw * 64].reshape(nw, 64)
                busy = cw.max(1) > 0
                rounds = cw.max(1)[busy].mean()
                use = cw[busy].sum() / (64.0 * cw.max(1)[busy].sum())
                base = base or (cand[sel].mean(), rounds)
                print("  %-24s S=%d  candidates/point %6.2f (%+5.1f %%)  rounds/wavefront %6.2f (%+5.1f %%)  lane use %.2f"
                      % (label, S, cand[sel].mean(), 100.0 * (cand[sel].mean() / base[0] - 1.0), rounds,
                         100.0 * (rounds / base[1] - 1.0), use))
                if label == "late sweep":
                    tot[S][0] += cw[busy].sum()
                    tot[S][1] += 64 * cw.max(1)[busy].sum()
                    tot[S][2] += sel[:nw * 64].sum()
    print("late sweeps, corner + surf:")
    b = tot[Ss[0]]
    for S in Ss:
        c_, r_, n_ = tot[S]
        print("  S=%d  candidates/point %6.2f (%+5.1f %%)  lane-rounds/point %6.2f (%+5.1f %%)  lane use %.2f"
              % (S, c_ / n_, 100.0 * (c_ / b[0] - 1.0), r_ / n_, 100.0 * (r_ / b[1] - 1.0), c_ / r_))


if __name__ == "__main__":
    main()
