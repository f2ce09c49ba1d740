"""The occupancy grid on the device (lslam_occ_*, csrc/lslam_occ.hip) against tests/occupancy_ref.py: counts, values and ray
counters equal in every cell -- single rays on prescribed fixed-point coordinates, the classification's thresholds, random clouds
that straddle the kernel's tile and chunk, the algebra of integrations, dropped rays, the refusals -- and the scene of a box that
is there for two keyframes of six, through the store and through Graph(occupancy=True).save."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import occupancy_ref as R

pytestmark = pytest.mark.gpu

E4 = np.zeros((0, 4), np.float32)
F32 = np.float32


def _xyz(a, b, h, up_axis):
    """(a, b, h) -> (x, y, z): up_axis 1: (a, b, h) = (z, x, y); 2: (x, y, z)."""
    return (b, h, a) if up_axis == 1 else (a, b, h)


def _pose_ab(a, b, h, up_axis):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = _xyz(a, b, h, up_axis)
    return T


def _points(abh, up_axis):
    out = np.zeros((len(abh), 4), np.float32)
    for k, (a, b, h) in enumerate(abh):
        out[k, :3] = _xyz(a, b, h, up_axis)
    return out


def _same(store, grid, what=""):
    """Counts, values and the ray counters of the store equal the reference grid's, in every cell."""
    got, want = store.occ_counts(), grid.counts()
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d cells differ" % (what, int((got != want).sum()))
    assert np.array_equal(store.occ_values(), grid.values()), what
    info = store.occ_info()
    assert (info["rays_cast"], info["rays_dropped"], info["rays_obstacle"], info["rays_ground"]) == \
        (grid.stats["cast"], grid.stats["dropped"], grid.stats["obstacle"], grid.stats["ground"]), what
    assert info["n_integrated"] == grid.n_integrated


# ---- single rays on prescribed fixed-point coordinates ------------------------------------------------------------------------
# 64 x 48 cells of 0.25 m (scale 1024 per metre, exact), origin (0, 0): a fixed-point unit is 2^-10 m, so poses and points that
# are multiples of it land A and B exactly.  C: a cell corner well inside the grid.
C0 = 20 * 256
SINGLE = {
    "octant +a+b shallow": ((C0 + 100, C0 + 60), (C0 + 1000, C0 + 360)),
    "octant +a+b steep": ((C0 + 100, C0 + 60), (C0 + 400, C0 + 960)),
    "octant -a+b steep": ((C0 + 100, C0 + 60), (C0 - 200, C0 + 960)),
    "octant -a+b shallow": ((C0 + 100, C0 + 60), (C0 - 800, C0 + 360)),
    "octant -a-b shallow": ((C0 + 100, C0 + 60), (C0 - 800, C0 - 240)),
    "octant -a-b steep": ((C0 + 100, C0 + 60), (C0 - 200, C0 - 840)),
    "octant +a-b steep": ((C0 + 100, C0 + 60), (C0 + 400, C0 - 840)),
    "octant +a-b shallow": ((C0 + 100, C0 + 60), (C0 + 1000, C0 - 240)),
    "horizontal +": ((C0 + 100, C0 + 60), (C0 + 1600, C0 + 60)),
    "horizontal -": ((C0 + 100, C0 + 60), (C0 - 1400, C0 + 60)),
    "vertical +": ((C0 + 100, C0 + 60), (C0 + 100, C0 + 1560)),
    "vertical -": ((C0 + 100, C0 + 60), (C0 + 100, C0 - 1440)),
    "diagonal ++": ((C0 + 100, C0 + 60), (C0 + 1124, C0 + 1084)),
    "diagonal -+": ((C0 + 100, C0 + 60), (C0 - 924, C0 + 1084)),
    "diagonal --": ((C0 + 100, C0 + 60), (C0 - 924, C0 - 964)),
    "diagonal +-": ((C0 + 100, C0 + 60), (C0 + 1124, C0 - 964)),
    "along a grid line in a": ((C0 + 10, C0), (C0 + 1500, C0)),
    "along a grid line in b": ((C0, C0 + 1500), (C0, C0 + 10)),
    "through lattice corners, slope 1": ((C0 - 128, C0 - 128), (C0 + 640, C0 + 640)),
    "through lattice corners, slope -1": ((C0 - 128, C0 + 128), (C0 + 640, C0 - 640)),
    "through a lattice corner, slope 2": ((C0 - 64, C0 - 128), (C0 + 448, C0 + 896)),
    "through a lattice corner, slope -1/2": ((C0 - 128, C0 + 64), (C0 + 896, C0 - 448)),
    "B on a wall from the left": ((C0 + 100, C0 + 60), (C0 + 512, C0 + 60)),
    "B on a wall from the right": ((C0 + 800, C0 + 60), (C0 + 512, C0 + 60)),
    "B on a wall from below": ((C0 + 100, C0 + 60), (C0 + 130, C0 + 512)),
    "B on a wall from above": ((C0 + 100, C0 + 900), (C0 + 130, C0 + 512)),
    "B on a lattice corner": ((C0 + 100, C0 + 60), (C0 + 512, C0 + 768)),
    "A on a lattice corner": ((C0, C0), (C0 + 700, C0 + 300)),
    "A and B in one cell": ((C0 + 100, C0 + 60), (C0 + 200, C0 + 90)),
    "zero length inside a cell": ((C0 + 100, C0 + 60), (C0 + 100, C0 + 60)),
    "zero length on a wall": ((C0, C0 + 60), (C0, C0 + 60)),
    "zero length on a corner": ((C0, C0), (C0, C0)),
    "leaving the grid in a": ((60 * 256 + 30, C0 + 60), (60 * 256 + 2500, C0 + 700)),
    "leaving the grid in b": ((C0 + 100, 45 * 256 + 9), (C0 - 300, 45 * 256 + 2000)),
    "origin outside, end inside": ((-1500, 3000), (2000, 3300)),
    "origin inside, end outside": ((2000, 3300), (-1500, 3000)),
    "both ends outside, crossing a corner": ((-1000, 2000), (3000, -1500)),
    "both ends outside, crossing the width": ((-300, C0 + 77), (64 * 256 + 500, C0 - 400)),
    "both ends outside, missing the grid": ((-1000, -200), (3000, -100)),
    "end cell is the last cell": ((62 * 256 + 5, 46 * 256 + 5), (63 * 256 + 255, 47 * 256 + 255)),
}
SINGLE_P = dict(resolution=0.25, origin=(0.0, 0.0), width=64, height=48, min_range=0.5, max_range=20.0)


@pytest.mark.parametrize("up_axis", [1, 2])
def test_single_rays_cell_for_cell(pkg, ctx, up_axis):
    """One keyframe of one point per case and class; pose and point are multiples of the fixed-point unit, and the test asserts
    through the reference that A and B landed where they were meant to."""
    p = R.params(up_axis=up_axis, **SINGLE_P)
    store = pkg.KeyframeStore(ctx, slab_points=64)
    try:
        store.occ_setup(**p)
        cases = []
        for name, (A, B) in SINGLE.items():
            for cls, h in (("obstacle", -0.8), ("ground", -1.8)):  # the fallback plane: height above the floor = h + 1.8
                T = _pose_ab(A[0] / 1024.0, A[1] / 1024.0, 1.8, up_axis)
                pt = _points([((B[0] - A[0]) / 1024.0, (B[1] - A[1]) / 1024.0, h)], up_axis)
                a, b, _ = R.ray_ends(pt, T, p)
                assert (int(a[0]), int(a[1])) == A and (int(b[0, 0]), int(b[0, 1])) == B, name
                ob, gr = R.classify(pt, R.fallback_plane(p), p)
                assert (bool(ob[0]), bool(gr[0])) == (cls == "obstacle", cls == "ground"), name
                kid = store.add(pt if len(cases) % 2 else E4, E4 if len(cases) % 2 else pt)
                cases.append((name + " / " + cls, kid, T, pt))
        kfs = {kid: ((pt, E4) if i % 2 else (E4, pt)) for i, (_, kid, _, pt) in enumerate(cases)}
        grid = R.Grid(p)
        for name, kid, T, pt in cases:
            store.occ_clear()
            grid.clear()
            store.occ_integrate([kid], [T])
            grid.integrate(kfs, [kid], [T])
            _same(store, grid, name)
        assert store.occ_info()["ray_launches"] == len(cases)
        # and all of them in one call: every chunk of eight keyframes, the last one partial or not
        store.occ_clear()
        grid.clear()
        store.occ_integrate([c[1] for c in cases], [c[2] for c in cases])
        grid.integrate(kfs, [c[1] for c in cases], [c[2] for c in cases])
        _same(store, grid, "all single rays")
    finally:
        store.close()


# ---- classification -----------------------------------------------------------------------------------------------------------
def _ulps(v):
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


@pytest.mark.parametrize("up_axis", [1, 2])
def test_classification_thresholds_gates_and_planes(pkg, ctx, up_axis):
    p = R.params(up_axis=up_axis, resolution=0.25, origin=(-8.0, -6.0), width=64, height=48, min_range=1.0, max_range=10.0,
                 sensor_height=0.0)
    # with sensor_height 0 the fallback plane gives hgt = h exactly: every threshold, and one ulp to either side
    abh, want_cls = [], []
    k = 0
    for thr, inside in ((0.3, (False, True, True)), (2.0, (True, True, False)), (0.15, (True, True, False)), (-0.15, (False, True, True))):
        for hv, ins in zip(_ulps(thr), inside):
            abh.append((2.0 + 0.3 * k, 1.0 + 0.1 * k, float(hv)))
            want_cls.append(("obstacle" if thr > 0.2 else "ground") if ins else None)
            k += 1
    thr_pts = _points(abh, up_axis)
    ob, gr = R.classify(thr_pts, R.fallback_plane(p), p)
    assert [("obstacle" if o else "ground" if g else None) for o, g in zip(ob, gr)] == want_cls
    # the range gates: on them and one ulp to either side, along a at obstacle height; the reference says which are in
    gate_abh = [(float(v), 0.0, 0.0) for r in (1.0, 10.0) for v in _ulps(r)]
    gate_pts = _points(gate_abh, up_axis)
    gate_pts[:, [1 if up_axis == 1 else 2]] = 1.0  # hgt = 1: obstacle, if the gate lets it
    gate_pts2 = gate_pts.copy()  # |p|^2 = a^2 + 1: gates at sqrt(lo^2 - 1) are not floats, so shift the gate instead
    pg = dict(p, min_range=float(np.sqrt(F32(2.0))), max_range=float(np.sqrt(F32(101.0))))
    ob, _ = R.classify(gate_pts2, R.fallback_plane(pg), pg)
    d2 = (gate_pts2[:, 0] * gate_pts2[:, 0] + gate_pts2[:, 1] * gate_pts2[:, 1]) + gate_pts2[:, 2] * gate_pts2[:, 2]
    lo, hi = F32(pg["min_range"]) * F32(pg["min_range"]), F32(pg["max_range"]) * F32(pg["max_range"])
    assert np.array_equal(ob, (d2 >= lo) & (d2 <= hi)) and ob.any() and not ob.all()
    bad = _points([(3.0, 2.0, 1.0)] * 8, up_axis)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1], bad[5, 2] = np.nan, np.nan, np.nan, np.inf, -np.inf, np.inf
    bad[6, :3] = (1e30, 1e30, 0.5)   # the squared norm overflows: outside the gate
    bad[7, :3] = (0.2, 0.2, 0.2)     # inside min_range
    rng = np.random.default_rng(11)
    rnd = np.zeros((300, 4), np.float32)
    rnd[:, :3] = rng.uniform(-7.0, 7.0, (300, 3))
    rnd[:, 1 if up_axis == 1 else 2] = rng.uniform(-0.5, 2.4, 300)
    tilted = np.array(_xyz(0.05, -0.03, 1.0, up_axis) + (1.7,), np.float64)
    tilted[:3] /= np.linalg.norm(tilted[:3])
    T = R.pose_matrix((0.02, -0.03, 0.4, 0.5, 0.3, 0.2)).astype(np.float32)
    kfs = [(thr_pts[:5], thr_pts[5:]), (gate_pts2[:2], gate_pts2[2:]), (bad[:3], bad[3:]), (rnd[:100], rnd[100:]),
           (E4, rnd[:50]), (rnd[50:120], E4), (E4, E4)]
    store = pkg.KeyframeStore(ctx, slab_points=256)
    try:
        ids = [store.add(c, s) for c, s in kfs]
        I4 = np.eye(4, dtype=np.float32)

        def run(par, use, poses, planes=None, valid=None, what=""):
            store.occ_setup(**par)
            store.occ_clear()
            grid = R.Grid(par)
            store.occ_integrate(use, poses, planes, valid)
            grid.integrate(kfs, use, poses, planes, valid)
            _same(store, grid, what)
            return grid

        g = run(p, [0], [I4], what="thresholds")
        assert (g.stats["obstacle"], g.stats["ground"]) == (4, 4)
        g = run(pg, [1], [I4], what="range gates")
        assert g.stats["obstacle"] == int(ob.sum())
        g = run(p, [2], [I4], what="non-finite, overflowing and near points")
        assert g.stats["cast"] == 0 and g.counts().sum() == 0
        p18 = dict(p, sensor_height=1.8)
        every = [T] * len(ids)
        a = run(p18, ids, every, what="fallback plane")
        planes = np.tile(tilted, (len(ids), 1))
        b = run(p18, ids, every, planes, what="a tilted plane for every keyframe")
        assert not np.array_equal(a.counts(), b.counts())
        valid = np.array([1, 0, 1, 0, 1, 0, 1], np.int32)
        planes_nan = planes.copy()
        planes_nan[valid == 0] = np.nan  # not read
        c = run(p18, ids, every, planes_nan, valid, what="plane_valid 0 falls back")
        assert not np.array_equal(c.counts(), a.counts()) and not np.array_equal(c.counts(), b.counts())
        g = run(dict(p18, ground_clears=0), ids, every, planes, what="ground_clears 0")
        assert g.stats["ground"] == 0 and g.stats["obstacle"] == b.stats["obstacle"]
        g = run(p18, [4, 5, 6], [T] * 3, what="empty corner, empty surf, both empty")
        assert g.stats["cast"] > 0
        g = run(p18, [6], [T], what="both clouds empty alone")
        assert g.stats["cast"] == 0 and store.occ_info()["n_integrated"] == 1
        run(dict(p18, min_observations=2, hit_weight=1), ids + ids[:3], every + every[:3], what="min_observations 2, hit_weight 1")
    finally:
        store.close()


# ---- shapes: tiles, chunks, slabs ------------------------------------------------------------------------------------------------
SHAPE_P = dict(resolution=0.1, origin=(-3.17, 1.33), width=160, height=120, min_range=1.0, max_range=10.0)
SHAPE_POSES = [(0.03, -0.02, 0.3, 3.0, -2.0, 1.8), (-0.05, 0.04, 1.2, 5.5, -1.0, 1.9), (0.02, 0.06, -0.7, 4.0, 1.5, 1.7),
               (0.08, -0.03, 2.6, 1.0, -3.5, 1.85), (-0.04, -0.05, -2.1, 6.0, -4.0, 1.75), (0.01, 0.02, 0.9, -2.0, 2.0, 1.8),
               (0.0, 0.0, 0.0, 9.5, 6.0, 1.8), (-0.02, 0.03, 3.0, 2.2, 7.7, 1.82), (0.05, 0.05, -1.5, 12.5, 9.0, 1.78),
               (0.0, -0.06, 2.2, 7.0, 3.0, 1.8)]


def _world_to_graph(T, up_axis):
    """A z-up world pose as the pose of a sensor whose frame -- and graph -- is y up (x, y, z)_loam = (y, z, x)_world."""
    if up_axis == 2:
        return T
    P = np.zeros((4, 4))
    P[0, 1] = P[1, 2] = P[2, 0] = P[3, 3] = 1.0
    return P @ T @ P.T


@pytest.fixture(scope="module")
def shapes(pkg):
    return shapes_data(pkg)


def shapes_data(pkg):
    """Per up axis: ten keyframes of 1, TILE - 1, TILE, TILE + 1, 3 TILE + 7 ... random points at general SE(3) poses, and the
    reference vote of each, computed once."""
    tile, chunk = pkg.occupancy.RAY_TILE, pkg.occupancy.KF_CHUNK
    assert chunk + 2 == len(SHAPE_POSES)
    sizes = [1, tile - 1, tile, tile + 1, 3 * tile + 7]
    out = {}
    for up_axis in (1, 2):
        rng = np.random.default_rng(20 + up_axis)
        p = R.params(up_axis=up_axis, **SHAPE_P)
        kfs, poses = [], []
        for k, p6 in enumerate(SHAPE_POSES):
            n = sizes[k % len(sizes)]
            abh = np.stack([rng.uniform(-9.0, 9.0, n), rng.uniform(-9.0, 9.0, n), rng.uniform(-2.2, 0.6, n)], axis=1)
            pts = _points(abh, up_axis)
            cut = n // 3
            kfs.append((pts[:cut], pts[cut:]))
            poses.append(_world_to_graph(R.pose_matrix(p6), up_axis).astype(np.float32))
        votes = [R.keyframe_vote(c, s, T, None, p) for (c, s), T in zip(kfs, poses)]
        assert sum(v[2]["obstacle"] for v in votes) > 300 and sum(v[2]["ground"] for v in votes) > 50
        out[up_axis] = dict(p=p, kfs=kfs, poses=poses, votes=votes)
    return out


def _sum_votes(sh, ids):
    g = R.Grid(sh["p"])
    for k in ids:
        hit, free, st = sh["votes"][k]
        g.n_hit += hit
        g.n_free += free
        for key in g.stats:
            g.stats[key] += st[key]
        g.n_integrated += 1
    return g


@pytest.mark.parametrize("up_axis", [1, 2])
def test_tiles_chunks_and_slabs(pkg, ctx, shapes, up_axis):
    sh = shapes[up_axis]
    chunk = pkg.occupancy.KF_CHUNK
    store = pkg.KeyframeStore(ctx, slab_points=1024)
    try:
        ids = [store.add(c, s) for c, s in sh["kfs"]]
        assert store.info()["n_slabs"] >= 3
        store.occ_setup(**sh["p"])
        assert store.occ_info()["grid_bytes"] == 0  # nothing before the grid is needed
        for n in (1, chunk - 1, chunk, chunk + 1, len(ids)):
            store.occ_clear()
            before = store.occ_info()
            store.occ_integrate(ids[:n], sh["poses"][:n])
            _same(store, _sum_votes(sh, ids[:n]), "%d keyframes" % n)
            after = store.occ_info()
            assert after["ray_launches"] - before["ray_launches"] == (n + chunk - 1) // chunk
            assert after["grid_bytes"] == 5 * 160 * 120 and after["scratch_bytes"] > 0
        lib = store.lib
        assert lib.lslam_debug_occ_integrate(store.h, 2) == 0  # the tap: the grid and the stats stay
        _same(store, _sum_votes(sh, ids), "after the tap")
        assert store.occ_info()["ray_launches"] == after["ray_launches"]
    finally:
        store.close()


# ---- algebra ------------------------------------------------------------------------------------------------------------------
def test_algebra_of_integrations(pkg, ctx, shapes):
    sh = shapes[2]
    P = sh["poses"]
    store = pkg.KeyframeStore(ctx, slab_points=1024)
    try:
        ids = [store.add(c, s) for c, s in sh["kfs"]]
        store.occ_setup(**sh["p"])
        A, B = [0, 2, 4, 6, 8], [1, 3, 4, 9]
        store.occ_integrate(A, [P[k] for k in A])
        store.occ_integrate(B, [P[k] for k in B])
        ab = store.occ_counts()
        _same(store, _sum_votes(sh, A + B), "A then B")
        store.occ_clear()
        assert store.occ_counts().sum() == 0 and (store.occ_values() == -1).all()
        info = store.occ_info()
        assert info["n_integrated"] == 0 and info["rays_cast"] == 0 and info["is_set"] and info["width"] == 160  # the parameters stay
        store.occ_integrate(B, [P[k] for k in B])
        store.occ_integrate(A, [P[k] for k in A])
        assert np.array_equal(store.occ_counts(), ab)
        store.occ_clear()
        store.occ_integrate(A + B, [P[k] for k in A + B])
        assert np.array_equal(store.occ_counts(), ab)
        # an id named twice votes twice (keyframe 4 is in A and in B); one keyframe alone, then twice in one call
        store.occ_clear()
        store.occ_integrate([4], [P[4]])
        one = store.occ_counts()
        hit, free, _ = sh["votes"][4]
        assert np.array_equal(one, (free.astype(np.uint32) | (hit.astype(np.uint32) << 16)))
        assert not (hit & free).any() and hit.any() and free.any()  # within one keyframe: one hit and no free, or one free
        store.occ_integrate([4, 4], [P[4], P[4]])
        assert np.array_equal(store.occ_counts(), 3 * one)
        # across two keyframes a cell counts both: some cell is hit by one and crossed by the other
        store.occ_clear()
        store.occ_integrate([4, 9], [P[4], P[9]])
        both = store.occ_counts()
        nf, nh = pkg.occupancy.split_counts(both)
        other_hit, other_free, _ = sh["votes"][9]
        mixed = (hit & other_free) | (other_hit & free)
        assert mixed.sum() > 5 and ((nf == 1) & (nh == 1))[mixed].all() and int(nf.max()) <= 2 and int(nh.max()) <= 2
        # the device view agrees with the downloads; the store's byte counters did not move over any of it
        pc, pv = store.occ_view()
        assert pc and pv
        n = 160 * 120
        dev_c, dev_v = np.zeros(n, np.uint32), np.zeros(n, np.int8)
        rt = C.CDLL("libamdhip64.so")  # (the library's own runtime: loaded with it)
        rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert rt.hipMemcpy(dev_c.ctypes.data, pc, 4 * n, 2) == 0 and rt.hipMemcpy(dev_v.ctypes.data, pv, n, 2) == 0
        assert np.array_equal(dev_c.reshape(120, 160), both) and np.array_equal(dev_v.reshape(120, 160), store.occ_values())
        kinfo = store.info()
        assert kinfo["cloud_bytes_downloaded"] == 0 and kinfo["cloud_bytes_uploaded"] == 16 * sum(len(c) + len(s) for c, s in sh["kfs"])
        # new parameters clear; the same parameters again do not
        store.occ_setup(**sh["p"])
        assert np.array_equal(store.occ_counts(), both)
        store.occ_setup(**dict(sh["p"], hit_weight=5))
        assert store.occ_info()["n_integrated"] == 0 and store.occ_counts().sum() == 0 and store.occ_info()["hit_weight"] == 5
        store.occ_integrate([0], [P[0]])
        # lslam_kfs_clear frees the grid; the parameters stay and the next integration starts from zero
        store.clear()
        info = store.occ_info()
        assert info["grid_bytes"] == 0 and info["scratch_bytes"] == 0 and info["is_set"] and info["n_integrated"] == 0
        assert store.lib.lslam_debug_occ_integrate(store.h, 1) == pkg.Status.ERR_INVALID
        kid = store.add(*sh["kfs"][4])
        store.occ_setup(**sh["p"])
        store.occ_integrate([kid], [P[4]])
        assert np.array_equal(store.occ_counts(), one)
    finally:
        store.close()


# ---- dropped rays -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up_axis", [1, 2])
def test_rays_beyond_the_fixed_point_range_are_dropped_and_counted(pkg, ctx, up_axis):
    """resolution 0.25: 2^30 units are 2^20 m.  An origin beyond that drops every ray of its keyframe; an origin just inside
    drops the rays whose end lies beyond; the far side of the range, negative, likewise."""
    edge = float(1 << 20)
    p = R.params(up_axis=up_axis, resolution=0.25, origin=(edge - 12.0, -4.0), width=64, height=48, max_range=10.0)
    rng = np.random.default_rng(31)
    abh = np.stack([rng.uniform(-8.0, 8.0, 400), rng.uniform(-8.0, 8.0, 400), rng.uniform(-2.0, 0.4, 400)], axis=1)
    pts = _points(abh, up_axis)
    kfs = [(pts[:150], pts[150:])]
    poses = [_pose_ab(edge - 12.0 + 6.0, 1.0, 1.8, up_axis),            # all inside
             _pose_ab(2.0 * edge - 12.0 - 3.0, 1.0, 1.8, up_axis),      # A inside the range, the rays towards +a leave it
             _pose_ab(2.0 * edge - 12.0 + 64.0, 1.0, 1.8, up_axis),     # A outside: everything dropped
             _pose_ab(-12.0 + 2.0, 1.0, 1.8, up_axis),                  # the negative end: rays towards -a leave it
             _pose_ab(edge - 12.0 + 6.0, -edge - 4.0 - 30.0, 1.8, up_axis)]  # b beyond the negative end
    store = pkg.KeyframeStore(ctx)
    try:
        kid = store.add(*kfs[0])
        store.occ_setup(**p)
        store.occ_integrate([kid], poses[:1])
        grid = R.Grid(p)
        grid.integrate(kfs, [0], poses[:1])
        assert grid.stats["dropped"] == 0 and grid.stats["cast"] > 100
        _same(store, grid, "inside")
        counts = store.occ_counts()
        for k in range(1, len(poses)):
            store.occ_integrate([kid], poses[k:k + 1])
            grid.integrate(kfs, [0], poses[k:k + 1])
            _same(store, grid, "pose %d" % k)
        assert np.array_equal(store.occ_counts(), counts)  # none of those rays touched the grid
        assert grid.stats["dropped"] > 2 * grid.stats["cast"] / 5 and grid.n_integrated == 5
    finally:
        store.close()


# ---- refusals that need a device ----------------------------------------------------------------------------------------------
def test_refusals_change_nothing(pkg, ctx, shapes):
    sh = shapes[2]
    P = sh["poses"]
    lib = pkg.load_library()
    INVALID = pkg.Status.ERR_INVALID
    store = pkg.KeyframeStore(ctx, slab_points=1024)

    def refused(fn, word):
        with pytest.raises(pkg.LslamError) as e:
            fn()
        assert e.value.code == INVALID and word in str(e.value), str(e.value)

    try:
        ids = [store.add(c, s) for c, s in sh["kfs"][:3]]
        # before setup
        for fn in (lambda: store.occ_integrate([0], P[:1]), store.occ_counts, store.occ_values, store.occ_clear, store.occ_view):
            refused(fn, "lslam_occ_setup was not called")
        assert not store.occ_info()["is_set"] and store.occ_info()["grid_bytes"] == 0
        # every parameter limit
        good = dict(sh["p"])
        bad = [("resolution", 0.009), ("resolution", float("nan")), ("width", 0), ("width", 8193), ("height", 0), ("height", 8193),
               ("up_axis", 0), ("up_axis", 3), ("min_range", 0.0), ("min_range", float("inf")), ("max_range", 0.5),
               ("max_range", float("nan")), ("max_range", 205.0), ("obstacle_min", 2.5), ("obstacle_max", float("inf")),
               ("ground_band", -0.01), ("ground_band", 0.3), ("sensor_height", float("nan")), ("ground_clears", 2),
               ("hit_weight", 0), ("hit_weight", 17), ("min_observations", 0), ("origin", (float("nan"), 0.0)),
               ("origin", (0.0, float("inf")))]
        for k, v in bad:
            refused(lambda: store.occ_setup(**dict(good, **{k: v})), "origin" if k == "origin" else
                    {"width": "width", "height": "width", "obstacle_max": "obstacle_m"}.get(k, k))
        assert lib.lslam_occ_setup(store.h, None) == INVALID and "null params" in lib.lslam_last_error().decode()
        rp = pkg.occupancy.occ_params(**good)
        rp.reserved = 1
        assert lib.lslam_occ_setup(store.h, C.byref(rp)) == INVALID and "reserved" in lib.lslam_last_error().decode()
        assert not store.occ_info()["is_set"]
        store.occ_setup(**good)
        store.occ_integrate(ids, P[:3])
        counts, values, info = store.occ_counts(), store.occ_values(), store.occ_info()
        # a refused setup leaves the parameters in force and the grid
        refused(lambda: store.occ_setup(**dict(good, hit_weight=99)), "hit_weight")
        nanpose = np.array(P[0])
        nanpose[1, 2] = np.nan
        infpose = np.array(P[0])
        infpose[2, 3] = np.inf
        lastrow = np.array(P[0])
        lastrow[3, :] = np.nan  # the fourth row is not read
        okplane = np.array([[0.0, 0.0, 1.0, 1.8]])
        refused(lambda: store.occ_integrate([3], P[:1]), "out of range")
        refused(lambda: store.occ_integrate([0, -1], P[:2]), "out of range")
        refused(lambda: store.occ_integrate([0], [nanpose]), "pose 0 is not finite")
        refused(lambda: store.occ_integrate([0, 1], [P[0], infpose]), "pose 1 is not finite")
        refused(lambda: store.occ_integrate([0], P[:1], np.array([[0.0, np.nan, 1.0, 1.8]])), "plane 0 is not finite")
        refused(lambda: store.occ_integrate([0], P[:1], np.array([[0.0, 0.0, 1.0, 1e300]])), "plane 0 is not finite")
        refused(lambda: store.occ_integrate([0], P[:1], np.array([[0.0, 0.0, 0.0, 1.8]])), "normal of zero length")
        refused(lambda: store.occ_integrate([0], P[:1], np.array([[1e-60, 0.0, 0.0, 1.8]])), "normal of zero length")  # zero in fp32
        ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        i1 = np.zeros(1, np.int32)
        T1 = np.ascontiguousarray(P[0]).reshape(16)
        assert lib.lslam_occ_integrate(store.h, 1, None, T1.ctypes.data_as(fp), None, None) == INVALID
        assert lib.lslam_occ_integrate(store.h, 1, i1.ctypes.data_as(ip), None, None, None) == INVALID
        assert lib.lslam_occ_integrate(store.h, -1, i1.ctypes.data_as(ip), T1.ctypes.data_as(fp), None, None) == INVALID
        assert lib.lslam_occ_integrate(store.h, 65536, i1.ctypes.data_as(ip), T1.ctypes.data_as(fp), None, None) == INVALID
        assert "n_ids outside 0 .. 65535" in lib.lslam_last_error().decode()
        assert lib.lslam_occ_counts(store.h, None) == INVALID and lib.lslam_occ_values(store.h, None) == INVALID
        assert lib.lslam_occ_info(store.h, None) == INVALID and lib.lslam_debug_occ_integrate(store.h, -1) == INVALID
        # the cap of 65535 keyframes per grid: 3 are in, 65533 more are one too many -- refused before anything runs
        many = np.zeros(65533, np.int32)
        manyT = np.ascontiguousarray(np.tile(np.asarray(P[0], np.float32).reshape(1, 16), (65533, 1)))
        assert lib.lslam_occ_integrate(store.h, 65533, many.ctypes.data_as(ip), manyT.ctypes.data_as(fp), None, None) == INVALID
        assert "cap of 65535" in lib.lslam_last_error().decode()
        assert np.array_equal(store.occ_counts(), counts) and np.array_equal(store.occ_values(), values)
        after = store.occ_info()
        assert {k: v for k, v in after.items() if k != "value_launches"} == {k: v for k, v in info.items() if k != "value_launches"}
        # what is allowed: no keyframes at all, a plane that is not read, a fourth pose row of anything
        store.occ_integrate([], np.zeros((0, 4, 4)))
        assert np.array_equal(store.occ_counts(), counts)
        store.occ_clear()
        store.occ_integrate([0], [lastrow], np.array([[np.nan] * 4]), [0])
        store.occ_integrate([1, 2], P[1:3], np.tile(okplane, (2, 1)))
        assert np.array_equal(store.occ_counts(), counts)  # (the given plane is the fallback's)
    finally:
        store.close()
    own = pkg.Context(0)
    st = pkg.KeyframeStore(own)
    st.add(*sh["kfs"][0])
    st.occ_setup(**sh["p"])
    own.close()
    for fn in (lambda: st.occ_setup(**sh["p"]), lambda: st.occ_integrate([0], P[:1]), st.occ_counts, st.occ_info, st.occ_clear):
        refused(fn, "its ctx was destroyed")
    st.close()


# ---- the scene: a box that is there for the first two of six keyframes --------------------------------------------------------
SCENE_BOX = (5.0, 7.0, 1.0, 3.0, 1.6)
SCENE_POSES = [(0, 0, .3, -4, -2), (0, 0, .35, -2.5, -2), (0, 0, .2, -1, -2), (0, 0, .3, 0.5, -2), (0, 0, .4, 2, -1.5), (0, 0, .25, 3.5, -2)]
SCENE_WALL = 12.0
# 0.5 m cells whose borders lie a quarter metre off the walls' faces: a face is in the middle of its cells
SCENE_P = dict(resolution=0.5, origin=(-15.25, -15.25), width=61, height=61, up_axis=2, max_range=30.0)


@pytest.fixture(scope="module")
def scene(synth):
    return scene_data(synth)


def scene_data(synth):
    world = synth.World(half_extent=60, wall_half=SCENE_WALL, pitch=1000.0)  # no buildings inside the walls ...
    world.poles = np.zeros((0, 5))                                            # ... and no poles: the masks below are the scene
    world.boxes = np.zeros((0, 5))
    with_box = copy.deepcopy(world)
    with_box.boxes = np.array([SCENE_BOX], np.float64)
    clouds, poses = [], []
    for i, (rx, ry, rz, x, y) in enumerate(SCENE_POSES):
        gt = (rx, ry, rz, x, y, synth.SENSOR_HEIGHT)
        c, s, _ = synth.make_scan(with_box if i < 2 else world, rings=16, azimuth_steps=450, gt_pose=gt, noise_sigma=0.02, seed=10 + i)
        clouds.append((c, s))
        poses.append(R.pose_matrix(gt).astype(np.float32))
    p = R.params(**SCENE_P)
    grid = R.Grid(p)
    grid.integrate(clouds, list(range(6)), poses)
    return dict(clouds=clouds, poses=poses, p=p, grid=grid)


def _cell(v):
    return int(np.floor((v + 15.25) / 0.5))


def _scene_masks():
    """Region masks from the scene's geometry, each eroded by one cell."""
    H = W = 61
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lo, hi = _cell(-SCENE_WALL), _cell(SCENE_WALL)  # the cells of the inner wall faces
    inner = (ii >= lo + 2) & (ii <= hi - 2) & (jj >= lo + 2) & (jj <= hi - 2)
    wall = (((ii == lo) | (ii == hi)) & (jj >= lo + 2) & (jj <= hi - 2)) | (((jj == lo) | (jj == hi)) & (ii >= lo + 2) & (ii <= hi - 2))
    beyond = (ii <= lo - 3) | (ii >= hi + 3) | (jj <= lo - 3) | (jj >= hi + 3)  # past the walls' half-metre thickness and one cell
    corridor = (ii >= _cell(-4.0) - 1) & (ii <= _cell(3.5) + 1) & (jj >= _cell(-3.0)) & (jj <= _cell(-1.0))
    x0, x1, y0, y1, _ = SCENE_BOX
    box = (ii >= _cell(x0)) & (ii <= _cell(x1)) & (jj >= _cell(y0)) & (jj <= _cell(y1))
    return dict(inner=inner, wall=wall, beyond=beyond, corridor=corridor, box=box)


def _assert_scene(values):
    m = _scene_masks()
    assert m["wall"].sum() > 150 and (values[m["wall"]] >= 65).all(), "wall cells"
    assert m["corridor"].sum() > 60 and (values[m["corridor"]] >= 0).all() and (values[m["corridor"]] <= 19).all(), "the driven corridor"
    assert m["box"].sum() >= 16 and (values[m["box"]] < 65).all(), "the box's cells"
    assert (values[m["box"]] > 19).sum() >= 8  # two keyframes did see it: it is in the votes, and outvoted
    assert m["beyond"].sum() > 500 and (values[m["beyond"]] == -1).all(), "beyond the walls"
    free_inside = m["inner"] & ~m["box"]
    assert (values[free_inside] <= 19).all() and (values[free_inside] >= 0).all()


def test_scene_walls_corridor_box_and_beyond(pkg, ctx, scene):
    _assert_scene(scene["grid"].values())  # of the reference itself
    store = pkg.KeyframeStore(ctx)
    try:
        ids = [store.add(c, s) for c, s in scene["clouds"]]
        store.occ_setup(**scene["p"])
        store.occ_integrate(ids, scene["poses"])
        _same(store, scene["grid"], "scene")
        _assert_scene(store.occ_values())
    finally:
        store.close()


def _scene_graph(pkg, ctx, scene, occupancy):
    g = pkg.Graph(ctx=ctx, resident=True, occupancy=occupancy)
    for T, (c, s) in zip(scene["poses"], scene["clouds"]):
        assert g.add_frame(T.astype(np.float64), c, s) is not None
    g.optimize()
    assert len(g.keyframes) == len(scene["poses"])
    return g


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            path = os.path.join(d, f)
            out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out


def test_graph_save_writes_the_map_only_when_asked(pkg, ctx, scene, tmp_path):
    with pytest.raises(ValueError, match="occupancy needs resident=True"):
        pkg.Graph(ctx=ctx, occupancy=True)
    trees = {}
    for name, option in (("off", None), ("on", dict(up_axis=2, resolution=0.5, max_range=30.0))):
        g = _scene_graph(pkg, ctx, scene, option)
        try:
            if option is None:
                with pytest.raises(ValueError, match="without occupancy"):
                    g.occupancy_grid()
            out = g.save(str(tmp_path / name), bootstrap=True)
            assert ("occupancy" in out) == (option is not None)
            if option is not None:
                grid = out["occupancy"]
                p = grid["params"]
                # the bounds were fitted to the optimised poses +- max_range
                est = [np.asarray(kf.estimate, np.float64) for kf in g.keyframes]
                origin, w, h, _ = R.fit_bounds(est, R.params(**option))
                assert (p.width, p.height) == (w, h) and (p.origin[0], p.origin[1]) == origin and 134 <= w <= 137 and 120 <= h <= 123
                assert grid["stats"]["n_integrated"] == 6 and grid["stats"]["rays_obstacle"] > 5000 and 0 <= grid["floors_found"] <= 6
                print("floors found: %d of 6" % grid["floors_found"])
                img, meta = pkg.occupancy.load_map(str(tmp_path / name / "map"))
                assert img.shape == (h, w) and np.array_equal(img, R.trinary(grid["values"]))
                assert (img == 0).sum() > 150 and (img == 254).sum() > 1500 and (img == 205).sum() > 5000
                assert meta["image"] == "map.pgm" and float(meta["resolution"]) == 0.5
                assert meta["origin"] == "[%.17g, %.17g, 0.0]" % origin
                assert (meta["negate"], meta["occupied_thresh"], meta["free_thresh"]) == ("0", "0.65", "0.196")
                odom = g.occupancy_grid(poses="odom", floor=False)
                _, ow, oh, _ = R.fit_bounds([np.asarray(kf.odom, np.float64) for kf in g.keyframes], R.params(**option))
                assert odom["floors_found"] == 0 and odom["values"].shape == (oh, ow)
        finally:
            g.store.close()
        trees[name] = _tree(str(tmp_path / name))
    extra = sorted(set(trees["on"]) - set(trees["off"]))
    assert extra == ["map.pgm", "map.yaml"]
    assert all(trees["on"][k] == v for k, v in trees["off"].items())
