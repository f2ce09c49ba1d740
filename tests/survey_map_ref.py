"""Restatement of the survey-cloud feature map extractor (io_module/feature_extracter.cpp:43-130 over util/pcl_util.h:39-62,
107-182 and util/voxel_grid_partition.hpp:80-330) in numpy, with chunked brute-force searches.  PCL is not available: this
file is the yardstick tests/test_gpu_survey_map.py holds ``lslam_survey_*`` against, and it states the pipeline of
include/lslam_c.h literally -- including a *sequential*, queue-based region growing (``region_sequential``) next to the
min-ancestor fixpoint the device computes (``region_fixpoint``).

What is fixed here and not PCL's (DESIGN "Survey-cloud extractor"): block and in-block order, the neighbour test and its
``r2``, fp64 accumulation over ``p - q`` in ascending (search-grid cell, index) order, the Jacobi eigen-solve, undefined
normals leaving the pipeline, (distance, index) and (curvature, index) tie-breaks, output orders, fp64 angles."""
import functools

import numpy as np

from localization_ref import cube_index

F = np.float32
GRID_CELL_PAD = 1.0 + 1.0 / 1024.0
JACOBI_SWEEPS = 10

DEFAULTS = dict(boundary_angle=3.14159 / 2.0 * 0.9, partition_leaf=50.0, partition_min_points=1000, filter_leaf=0.05,
                filter_min_points=3, normal_radius=0.05, knn_k=60, smoothness_angle=float(F(3.0 / 180.0 * np.pi)),
                curvature_threshold=1.0, cluster_min=50, cluster_max=1000000, boundary_radius=0.1, feature_leaf=0.2,
                feature_min_points=3, cube_size=50.0, cube_dims=(21, 21, 21), cube_origin=(10, 5, 10))


def cos_threshold(angle):
    """cos of the fp32 angle, evaluated in double, rounded to fp32."""
    return F(np.cos(np.float64(F(angle))))


def radius2(r):
    return F(np.float64(F(r)) * np.float64(F(r)))


def d2_f32(a, b):
    """(m, n) fp32 squared distances: the three products summed left to right."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


# ---- partition and the filter with a minimum count -------------------------------------------------------------------------
def _guard(mn, mx, inv):
    d = ((mx - mn) * inv).astype(np.int64) + 1
    return int(d[0]) * int(d[1]) * int(d[2]) > np.iinfo(np.int32).max


def partition(cloud, leaf, min_points):
    """VoxelGridPartition::applyPartition -> (blocks in ascending cell index, input order inside; cells below the minimum)."""
    c = np.asarray(cloud, F)[:, :3]
    c = c[np.all(np.isfinite(c), axis=1)]
    if len(c) == 0:
        return [], 0
    inv = F(1.0) / F(leaf)
    mn, mx = c.min(0), c.max(0)
    if _guard(mn, mx, inv):
        return [], 0
    min_b = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(c * inv) - min_b.astype(F)).astype(F).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    cells, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    blocks = [c[order[s:s + n]] for s, n in zip(start, count) if n >= min_points]
    return blocks, int((count < min_points).sum())


def voxel_filter_min(cloud, leaf, min_points):
    """pcl::VoxelGrid with setMinimumPointsNumberPerVoxel: lslam_voxel_grid's arithmetic (fp32 sums in input order / count),
    voxels below the minimum give nothing.  (n, 3) or (n, 4) in, same width out."""
    c = np.asarray(cloud, F)
    if len(c) == 0:
        return c.copy()
    inv = F(1.0) / F(leaf)
    mn, mx = c[:, :3].min(0), c[:, :3].max(0)
    if _guard(mn, mx, inv):
        return c.copy()  # "Leaf size is too small for the input dataset": the input comes back
    base = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - base + 1
    ijk = np.floor(c[:, :3] * inv).astype(np.int64) - base
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    _, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    sums = np.zeros((len(start), c.shape[1]), F) + c[order[start]]  # from zero, as PCL: a lone -0.0f comes out as +0.0f
    for k in range(1, int(count.max())):
        m = count > k
        sums[m] = sums[m] + c[order[start[m] + k]]
    out = sums / count.astype(F)[:, None]
    return out[count >= min_points].astype(F)


# ---- normals -----------------------------------------------------------------------------------------------------------------
def grid_order(surface, cell):
    """The order the device's search grid gives a cloud: ascending (cell z, cell y, cell x, index), cells of size ``cell`` from
    the cloud's minimum, coordinates in fp64."""
    s = np.asarray(surface, F)[:, :3].astype(np.float64)
    lo, hi = s.min(0), s.max(0)
    dim = np.floor((hi - lo) / cell).astype(np.int64) + 1
    c = np.clip(np.floor((s - lo) / cell).astype(np.int64), 0, dim - 1)
    return np.lexsort((np.arange(len(s)), c[:, 0], c[:, 1], c[:, 2]))


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """One Jacobi rotation on arrays of matrices: the device's sv_rotate, operation for operation."""
    on = apq != 0.0
    safe = np.where(on, apq, 1.0)
    theta = (aqq - app) / (2.0 * safe)
    root = np.sqrt(theta * theta + 1.0)
    t = np.where(theta >= 0.0, 1.0 / (theta + root), -1.0 / (root - theta))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    rp, rq = c * arp - s * arq, s * arp + c * arq
    nvp = c[:, None] * vp - s[:, None] * vq
    nvq = s[:, None] * vp + c[:, None] * vq
    w = lambda new, old: np.where(on, new, old)
    return (w(app - h, app), w(aqq + h, aqq), w(0.0, apq), w(rp, arp), w(rq, arq),
            np.where(on[:, None], nvp, vp), np.where(on[:, None], nvq, vq))


def jacobi_smallest(a00, a01, a02, a11, a12, a22):
    """-> (l0, trace, normal (m, 3)): smallest eigenvalue (ties: the lower diagonal position) and its eigenvector."""
    m = len(a00)
    v0, v1, v2 = (np.tile(np.eye(3)[k], (m, 1)) for k in range(3))
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            a00, a11, a01, a02, a12, v0, v1 = _rotate(a00, a11, a01, a02, a12, v0, v1)
            a00, a22, a02, a01, a12, v0, v2 = _rotate(a00, a22, a02, a01, a12, v0, v2)
            a11, a22, a12, a01, a02, v1, v2 = _rotate(a11, a22, a12, a01, a02, v1, v2)
    l0, n = a00.copy(), v0.copy()
    k = a11 < l0
    l0, n = np.where(k, a11, l0), np.where(k[:, None], v1, n)
    k = a22 < l0
    l0, n = np.where(k, a22, l0), np.where(k[:, None], v2, n)
    return l0, (a00 + a11) + a22, n


def covariances(surface, queries, radius, chunk=256):
    """Per query: neighbour count and the fp64 mean-removed covariance entries over (double)p - (double)q, the neighbours
    taken in grid order."""
    r2 = radius2(radius)
    s32 = np.asarray(surface, F)[:, :3]
    s32 = s32[grid_order(s32, np.float64(F(radius)) * GRID_CELL_PAD)]
    q32 = np.asarray(queries, F)[:, :3]
    s64 = s32.astype(np.float64)
    count = np.zeros(len(q32), np.int64)
    cov = np.zeros((len(q32), 6))
    for a in range(0, len(q32), chunk):
        q = q32[a:a + chunk]
        rows, cols = np.nonzero(d2_f32(q, s32) < r2)
        cnt = np.bincount(rows, minlength=len(q))
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        slot = np.arange(len(rows)) - first[rows]
        width = int(cnt.max()) if len(rows) else 0
        pad = np.full((len(q), max(width, 1)), -1, np.int64)
        pad[rows, slot] = cols
        sums = np.zeros((len(q), 9))
        q64 = q.astype(np.float64)
        for k in range(width):
            ok = pad[:, k] >= 0
            d = np.where(ok[:, None], s64[np.maximum(pad[:, k], 0)] - q64, 0.0)
            t = np.stack([d[:, 0], d[:, 1], d[:, 2], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1],
                          d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
            sums = sums + t
        with np.errstate(all="ignore"):
            n = cnt.astype(np.float64)
            mx, my, mz = sums[:, 0] / n, sums[:, 1] / n, sums[:, 2] / n
            cov[a:a + chunk] = np.stack([sums[:, 3] / n - mx * mx, sums[:, 4] / n - mx * my, sums[:, 5] / n - mx * mz,
                                         sums[:, 6] / n - my * my, sums[:, 7] / n - my * mz, sums[:, 8] / n - mz * mz], 1)
        count[a:a + chunk] = cnt
    return count, cov


def normals(surface, queries, radius):
    """-> ((q, 4) fp32 {nx, ny, nz, curvature}, NaN rows where fewer than 3 neighbours; neighbour counts)."""
    count, cov = covariances(surface, queries, radius)
    out = np.full((len(count), 4), np.nan, F)
    ok = count >= 3
    if ok.any():
        c = cov[ok]
        l0, trace, n = jacobi_smallest(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), c[:, 3].copy(), c[:, 4].copy(), c[:, 5].copy())
        with np.errstate(all="ignore"):
            curv = np.where(trace == 0.0, 0.0, l0 / trace)
        q = np.asarray(queries, F)[ok, :3].astype(np.float64)
        along = (n[:, 0] * q[:, 0] + n[:, 1] * q[:, 1]) + n[:, 2] * q[:, 2]
        n = np.where((along > 0.0)[:, None], -n, n)
        out[ok] = np.concatenate([n, curv[:, None]], 1).astype(F)
    return out, count.astype(np.int32)


# ---- neighbour lists and region growing ------------------------------------------------------------------------------------
def knn_lists(pts, k, chunk=512):
    """(n, k) int32: each point's k nearest by (fp32 squared distance, index), itself included; -1 past the cloud's size."""
    p = np.asarray(pts, F)[:, :3]
    out = np.full((len(p), k), -1, np.int32)
    for a in range(0, len(p), chunk):
        order = np.argsort(d2_f32(p[a:a + chunk], p), axis=1, kind="stable")[:, :k]
        out[a:a + chunk, :order.shape[1]] = order
    return out


def edge_table(nrm, lists, c):
    """(n, k) bool: the edge i -> lists[i, t] exists; also |dot| (fp32) of every tested pair."""
    nrm = np.asarray(nrm, F)
    j = np.maximum(lists, 0)
    a, b = nrm[:, None, :3], nrm[j][:, :, :3]
    dot = np.abs((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])
    tested = (lists >= 0) & (lists != np.arange(len(lists))[:, None])
    return tested & (dot >= F(c)), dot, tested


def seed_order(curv):
    c = np.asarray(curv, F) + F(0.0)  # (-0 and +0 are one curvature)
    return np.lexsort((np.arange(len(c)), c))


def region_sequential(nrm, lists, c):
    """pcl::RegionGrowing::applyRegionGrowingAlgorithm / growRegion, literally: seeds in ascending (curvature, index), a queue
    per segment, a neighbour joins when it is unlabelled and its normal is within the threshold of the *current* point's, and
    (the curvature threshold 1.0 exceeds every curvature) every joined point is queued.  -> labels: each point's initial seed."""
    edge, _, _ = edge_table(nrm, lists, c)
    n = len(lists)
    label = np.full(n, -1, np.int64)
    for seed in seed_order(np.asarray(nrm, F)[:, 3]):
        if label[seed] != -1:
            continue
        label[seed] = seed
        queue = [int(seed)]
        while queue:
            i = queue.pop(0)
            for t in np.nonzero(edge[i])[0]:
                j = int(lists[i, t])
                if label[j] == -1:
                    label[j] = seed
                    queue.append(j)
    return label.astype(np.int32)


def region_fixpoint(nrm, lists, c):
    """The unique fixpoint of label[j] = min(label[j], label[i]) over the edges, labels starting as seed ranks, by synchronous
    rounds.  -> (labels as seed point indices, rounds until nothing changed)."""
    edge, _, _ = edge_table(nrm, lists, c)
    order = seed_order(np.asarray(nrm, F)[:, 3])
    label = np.empty(len(order), np.int64)
    label[order] = np.arange(len(order))
    src, slot = np.nonzero(edge)
    dst = lists[src, slot]
    rounds = 0
    while True:
        new = label.copy()
        np.minimum.at(new, dst, label[src])
        rounds += 1
        if np.array_equal(new, label):
            break
        label = new
    return order[label].astype(np.int32), rounds


def cluster_sizes(label):
    return np.bincount(label, minlength=len(label))[label]


# ---- boundary ----------------------------------------------------------------------------------------------------------------
def boundary(pts, nrm, radius, threshold, chunk=512):
    """-> (flags (n,) bool, largest angle gap (n,) fp64; 0 and False for a point without a neighbour of non-zero delta)."""
    p32 = np.asarray(pts, F)[:, :3]
    n32 = np.asarray(nrm, F)[:, :3]
    r2 = radius2(radius)
    n64 = n32.astype(np.float64)
    first = (np.abs(n32[:, 0]) > np.abs(n32[:, 2]) * F(1e-5)) | (np.abs(n32[:, 1]) > np.abs(n32[:, 2]) * F(1e-5))
    with np.errstate(all="ignore"):
        inv1 = 1.0 / np.sqrt(n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1])
        inv2 = 1.0 / np.sqrt(n64[:, 1] * n64[:, 1] + n64[:, 2] * n64[:, 2])
    zero = np.zeros(len(n64))
    v = np.where(first[:, None], np.stack([-n64[:, 1] * inv1, n64[:, 0] * inv1, zero], 1),
                 np.stack([zero, -n64[:, 2] * inv2, n64[:, 1] * inv2], 1))
    u = np.stack([n64[:, 1] * v[:, 2] - n64[:, 2] * v[:, 1], n64[:, 2] * v[:, 0] - n64[:, 0] * v[:, 2],
                  n64[:, 0] * v[:, 1] - n64[:, 1] * v[:, 0]], 1)
    gaps = np.zeros(len(p32))
    p64 = p32.astype(np.float64)
    for a in range(0, len(p32), chunk):
        q = p32[a:a + chunk]
        near = d2_f32(q, p32) < r2
        near &= np.any(q[:, None, :] != p32[None, :, :], axis=2)
        rows, cols = np.nonzero(near)
        if len(rows) == 0:
            continue
        d = p64[cols] - p64[a + rows]
        vv, uu = v[a + rows], u[a + rows]
        ang = np.arctan2((vv[:, 0] * d[:, 0] + vv[:, 1] * d[:, 1]) + vv[:, 2] * d[:, 2],
                         (uu[:, 0] * d[:, 0] + uu[:, 1] * d[:, 1]) + uu[:, 2] * d[:, 2])
        cnt = np.bincount(rows, minlength=len(q))
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        pad = np.full((len(q), int(cnt.max())), np.inf)
        pad[rows, np.arange(len(rows)) - start[rows]] = ang
        pad.sort(axis=1)
        with np.errstate(all="ignore"):
            dif = np.diff(pad, axis=1)
        dif[~np.isfinite(dif)] = 0.0
        has = cnt > 0
        last = pad[np.arange(len(q)), np.maximum(cnt - 1, 0)]
        wrap = (2.0 * np.pi - last) + pad[:, 0]
        best = np.maximum(dif.max(axis=1) if dif.shape[1] else 0.0, wrap)
        gaps[a:a + chunk] = np.where(has, best, 0.0)
    return gaps > threshold, gaps


# ---- the whole pipeline ------------------------------------------------------------------------------------------------------
def extract(cloud, **kw):
    """-> dict(corner, surf (n, 4) fp32 permuted, in block order; corner_cube, surf_cube; stats; blocks: per-block stages)."""
    P = dict(DEFAULTS, **kw)
    c = np.asarray(cloud, F)[:, :3]
    finite = np.all(np.isfinite(c), axis=1)
    st = dict(points_in=int(finite.sum()), points_nonfinite=int((~finite).sum()), blocks_kept=0, blocks_dropped=0, max_block_points=0,
              filtered_points=0, undefined_normals=0, clusters_kept=0, clusters_dropped=0, planar_points=0, boundary_points=0)
    blocks, st["blocks_dropped"] = partition(c, P["partition_leaf"], P["partition_min_points"])
    st["blocks_kept"] = len(blocks)
    cth = cos_threshold(P["smoothness_angle"])
    out = [[], []]
    stages = []
    for block in blocks:
        st["max_block_points"] = max(st["max_block_points"], len(block))
        stage = dict(block=block)
        stages.append(stage)
        filt = voxel_filter_min(block, P["filter_leaf"], P["filter_min_points"])
        st["filtered_points"] += len(filt)
        if len(filt) == 0:
            continue
        nrm_all, cnt = normals(block, filt, P["normal_radius"])
        stage.update(filtered=filt, normals_all=nrm_all, counts=cnt)
        ok = ~np.isnan(nrm_all[:, 0])
        st["undefined_normals"] += int((~ok).sum())
        pts, nrm = filt[ok], nrm_all[ok]
        if len(pts) == 0:
            continue
        lists = knn_lists(pts, P["knn_k"])
        label, rounds = region_fixpoint(nrm, lists, cth)
        size = cluster_sizes(label)
        planar = (size >= P["cluster_min"]) & (size <= P["cluster_max"])
        roots = label == np.arange(len(label))
        st["clusters_kept"] += int((roots & planar).sum())
        st["clusters_dropped"] += int((roots & ~planar).sum())
        flags, gaps = boundary(pts, nrm, P["boundary_radius"], P["boundary_angle"])
        st["planar_points"] += int(planar.sum())
        st["boundary_points"] += int(flags.sum())
        stage.update(pts=pts, normals=nrm, lists=lists, labels=label, rounds=rounds, planar=planar, flags=flags, gaps=gaps)
        for t, sel in enumerate((flags, planar)):
            f = voxel_filter_min(pts[sel], P["feature_leaf"], P["feature_min_points"])
            if len(f) == 0:
                continue
            perm = np.zeros((len(f), 4), F)
            perm[:, 0], perm[:, 1], perm[:, 2] = f[:, 1], f[:, 2], f[:, 0]
            ijk = cube_index(perm, P["cube_size"], P["cube_origin"])
            dims = np.asarray(P["cube_dims"])
            inside = np.all((ijk >= 0) & (ijk < dims), axis=1)
            idx = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]
            out[t].append((perm[inside], idx[inside]))
    res = {}
    for t, name in enumerate(("corner", "surf")):
        res[name] = np.concatenate([p for p, _ in out[t]], 0) if out[t] else np.zeros((0, 4), F)
        res[name + "_cube"] = np.concatenate([i for _, i in out[t]], 0) if out[t] else np.zeros(0, np.int64)
    st["n_corner"], st["n_surf"] = len(res["corner"]), len(res["surf"])
    res.update(stats=st, blocks=stages, params=P)
    return res


def save(res, directory):
    """saveCloudToFiles in the layout lslam_fmap_save writes: cubes in (i, j, k) loop order, corner before surf."""
    import os
    W, H, D = res["params"]["cube_dims"]
    count = 0
    with open(os.path.join(directory, "index.txt"), "w") as index:
        for i in range(W):
            for j in range(H):
                for k in range(D):
                    c = i + j * W + k * W * H
                    for t, name in enumerate(("corner", "surf")):
                        pts = res[name][res[name + "_cube"] == c]
                        if len(pts) == 0:
                            continue
                        with open(os.path.join(directory, "%d.pcd" % count), "wb") as f:
                            f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\n"
                                     "TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n"
                                     % (len(pts), len(pts))).encode())
                            f.write(np.ascontiguousarray(pts, F).tobytes())
                        index.write("%d %d %d %d %d %d\n" % (count, t, i, j, k, len(pts)))
                        count += 1


# ---- the test scene ------------------------------------------------------------------------------------------------------------
SCENE_SEED = 8  # (7 left 1.8e-6 of margin at the edge threshold: tests/test_survey_map_ref.py asks for 1e-5)
SCENE_PARAMS = dict(partition_leaf=4.0)
CORNER = (12.3, -7.1, 1.9)


def make_planes(seed=SCENE_SEED, n=100, spacing=0.02):
    """A floor and a wall of n x n points meeting at an edge: in-plane jitter +-4 mm, Gaussian noise 0.5 mm, fp32."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) * spacing
    cx, cy, cz = CORNER

    def plane():
        return g + rng.uniform(-0.004, 0.004, g.shape), rng.normal(0.0, 0.0005, len(g))
    a, na = plane()
    floor = np.stack([cx + a[:, 0], cy + a[:, 1], cz + na], 1)
    b, nb = plane()
    wall = np.stack([cx + nb, cy + b[:, 0], cz + b[:, 1]], 1)
    return np.concatenate([floor, wall], 0).astype(F)


def make_scene(seed=SCENE_SEED):
    """The two planes, a detached patch of 300 points (its partition cell stays below the block minimum) and a copy of the
    planes moved 40 m along y (a second block, and after the axis permutation a second cube)."""
    planes = make_planes(seed)
    rng = np.random.default_rng(seed + 1000)
    g = np.stack(np.meshgrid(np.arange(15), np.arange(20), indexing="ij"), -1).reshape(-1, 2) * 0.02
    patch = np.stack([CORNER[0] - 6.0 + g[:, 0], CORNER[1] + 10.0 + g[:, 1], CORNER[2] + rng.normal(0.0, 0.0005, len(g))], 1).astype(F)
    copy = (planes + np.array([0.0, 40.0, 0.0], F)).astype(F)
    return np.concatenate([planes, patch, copy], 0)


@functools.lru_cache(maxsize=None)
def scene_reference():
    """The scene and its extraction by this file, computed once per process and shared (treat as read-only)."""
    cloud = make_scene()
    return cloud, extract(cloud, **SCENE_PARAMS)
