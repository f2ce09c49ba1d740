"""Placed inputs for the localisation node's neighbour search (loc_probe_kernel / loc_tree_kernel, csrc/lslam_loc.hip): a
deterministic WALL MAP and QUERY SETS, numpy only, and the reference both are held to.

The node: a 9 x 9 x 5 cube array of 10 m cubes at the default origin (4, 4, 2), valid distance 20 m (grid_reach 2 < the array),
the map set unfiltered so that every cube keeps its points in input order.  World cube (i, j, k) is centred at 10 (i, j, k);
its walls are at 10 i +- 5.  Both types get the same structures (another seed for the random parts):

  lattice      an exact 0.25 m lattice block x 3.5 .. 6.5, y -6.5 .. -3.5, z -0.75 .. 0.75: it straddles the wall x = +5 (planes at
               4.75, 5.0, 5.25) and the wall y = -5; every coordinate a multiple of 0.25.  Queries on lattice points, edge midpoints,
               face centres and body centres tie 2-, 4- and 8-fold (and 6-fold).
  walls        single points at 5, nextafter(5, 0), nextafter(5, inf) on the positive and the negative wall of every axis, with six
               neighbours on either side, so that both cubes have trees.
  thin         cubes of exactly 4, 5, 6, 10 and 11 points (a cube gets a tree from 5 points on).
  duplicate    one point stored three times.
  cloud        300 jittered points in a slab of cube (2, 0, 0): the generic case, dense enough for the cell grid's proof.
  uncovered    a populated cube farther from the first query's cube than grid_reach: (4, 0, 0).
  corner cube  array index (0, 0, 0) = world (-4, -4, -2), populated, and the three cubes with ONE array index 0
               ((-4, 0, 0), (0, -4, 0), (0, 0, -2)): where a coordinate that is not a number must NOT land.

The reference: the cube from the fixed ``localization_ref.cube_index``; the five from ``oracle.kdtree(cube points).knn(q, 5)`` --
the nanoflann restatement decides which of several tied points is returned."""
import numpy as np

import localization_ref as lr

F = np.float32

DIMS = (9, 9, 5)
CUBE = 10.0
ORIGIN = (4, 4, 2)
VALID = 20.0
REACH = 2           # ceil(VALID / CUBE)
HALF = F(5.0)       # a wall of the cubes around the origin
THIN = {4: (-2, 1, 0), 5: (-2, 2, 0), 6: (-1, 2, 0), 10: (0, 2, 0), 11: (1, 2, 0)}  # points -> world cube
CLOUD_CUBE = (2, 0, 0)
UNCOVERED_CUBE = (4, 0, 0)
EMPTY_CUBE = (-2, -2, 0)
DUP_POINT = (-10.0, -10.0, 0.5)
ZERO_INDEX_CUBES = ((-4, -4, -2), (-4, 0, 0), (0, -4, 0), (0, 0, -2))
LATTICE_LO, LATTICE_N = (3.5, -6.5, -0.75), (13, 13, 7)

cube_index = lr.cube_index


def cube_index_old(p, cube_size, origin):
    """The expression localization_ref carried before: the half added in float32 -- kept to show what it got wrong."""
    q = np.asarray(p, F)[..., :3] / F(cube_size)
    r = np.where(q >= 0, np.floor(q + F(0.5)), np.ceil(q - F(0.5))).astype(F)
    return (r + np.asarray(origin, F)).astype(np.int64)


def wall_values(sign):
    """The wall sign * 5 with its two float32 neighbours, and theirs: five consecutive floats, ascending in magnitude."""
    h = HALF
    p, n = np.nextafter(h, F(0)), np.nextafter(h, F(np.inf))
    return (np.array([np.nextafter(p, F(0)), p, h, n, np.nextafter(n, F(np.inf))], F) * F(sign)).astype(F)


def _centre(cube):
    return np.asarray(cube, np.float64) * CUBE


def lattice_points():
    ax = [LATTICE_LO[a] + 0.25 * np.arange(LATTICE_N[a]) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    return g.astype(F)


def _wall_points():
    """Per axis and sign: the three wall values, the other two coordinates 2.0, and six neighbours on either side."""
    out = []
    for a in range(3):
        for sign in (1.0, -1.0):
            for v in wall_values(sign)[1:4]:
                p = np.full(3, 2.0, F)
                p[a] = v
                out.append(p)
            for side in (-1.0, 1.0):
                for m in range(6):
                    p = np.array([2.0 + 0.13 * m, 2.0 - 0.11 * m, 2.0 + 0.07 * (m % 3)], np.float64)
                    p[a] = sign * 5.0 + side * (0.3 + 0.1 * m)
                    out.append(p.astype(F))
    return np.asarray(out, F)


def make_map(t):
    """The wall map of type t (0 corner, 1 surf) -> (n, 4) float32, the intensity the point's number."""
    rng = np.random.default_rng(4100 + t)
    parts = [lattice_points(), _wall_points()]
    for n, cube in sorted(THIN.items()):
        parts.append((_centre(cube) + rng.uniform(-3.0, 3.0, (n, 3))).astype(F))
    dup = np.asarray(DUP_POINT, F)
    parts.append(np.concatenate([np.tile(dup, (3, 1)), (dup + rng.uniform(-1.5, 1.5, (8, 3))).astype(F)], 0))
    lo, hi = _centre(CLOUD_CUBE) + (-2.0, -2.0, -0.25), _centre(CLOUD_CUBE) + (2.0, 2.0, 0.25)
    parts.append(rng.uniform(lo, hi, (300, 3)).astype(F))
    parts.append((_centre(UNCOVERED_CUBE) + rng.uniform(-3.0, 3.0, (12, 3))).astype(F))
    for cube in ZERO_INDEX_CUBES:
        parts.append((_centre(cube) + rng.uniform(-3.0, 3.0, (8, 3))).astype(F))
    xyz = np.concatenate(parts, 0).astype(F)
    return np.concatenate([xyz, np.arange(len(xyz), dtype=F)[:, None]], 1)


def make_queries(t):
    """The queries of type t in the map frame -> (xyz (n, 3) float32, kind (n,) of str).  The first query is a lattice point of
    cube (0, 0, 0) -- a node's grids are placed around it -- and the rest are dealt out in a fixed shuffle, so that every
    workgroup of 256 gets every kind."""
    rng = np.random.default_rng(5200 + t)
    q, kind = [], []

    def add(name, pts):
        pts = np.asarray(pts, F).reshape(-1, 3)
        q.append(pts)
        kind.extend([name] * len(pts))
    lat = lattice_points()
    pick = lat[rng.choice(len(lat), 60, replace=False)]
    add("lattice point", pick)
    for name, axes in (("edge midpoint", 1), ("face centre", 2), ("body centre", 3)):
        base = lat[rng.choice(len(lat), 60, replace=False)].copy()
        for i in range(len(base)):
            for a in rng.permutation(3)[:axes]:
                base[i, a] += F(0.125)
        add("lattice " + name, base)
    add("duplicate", [DUP_POINT])
    for a in range(3):
        for sign in (1.0, -1.0):
            for v in wall_values(sign):
                p = np.full(3, 2.0, F)
                p[a] = v
                add("wall value", p)
    # within 0.1 m of the walls the lattice straddles: some of the global five lie in the cube across
    for a, w in ((0, 5.0), (1, -5.0)):
        p = np.stack([rng.uniform(3.6, 6.4, 40), rng.uniform(-6.4, -3.6, 40), rng.uniform(-0.7, 0.7, 40)], 1)
        p[:, a] = w + rng.choice([-1.0, 1.0], 40) * rng.uniform(0.01, 0.1, 40)
        add("near a wall", p)
    for n, cube in sorted(THIN.items()):
        add("thin %d" % n, _centre(cube) + rng.uniform(-4.0, 4.0, (4, 3)))
    lo, hi = _centre(CLOUD_CUBE) + (-1.8, -1.8, -0.2), _centre(CLOUD_CUBE) + (1.8, 1.8, 0.2)
    add("cloud", rng.uniform(lo, hi, (150, 3)))
    add("empty cube", _centre(EMPTY_CUBE) + rng.uniform(-4.0, 4.0, (2, 3)))
    add("uncovered cube", _centre(UNCOVERED_CUBE) + rng.uniform(-4.0, 4.0, (6, 3)))
    for cube in ZERO_INDEX_CUBES:
        add("index 0 cube", _centre(cube) + rng.uniform(-3.0, 3.0, (2, 3)))
    for a in range(3):
        for i in (-1, DIMS[a]):  # array index -1 and W
            p = np.full(3, 1.0, F)
            p[a] = (i - ORIGIN[a]) * CUBE
            add("outside the array", p)
    add("1e30", [(1e30, 1.0, 1.0), (1e30, -1e30, 1e30)])
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = np.full(3, 1.0, F)
            p[a] = bad
            add("not finite", p)
        add("not finite", np.full(3, bad, F))
    q, kind = np.concatenate(q, 0).astype(F), np.asarray(kind)
    first = int(np.flatnonzero((kind == "lattice point") & np.all(cube_index(q, CUBE, ORIGIN) == np.asarray(ORIGIN), axis=1))[0])
    order = np.concatenate([[first], rng.permutation(np.delete(np.arange(len(q)), first))])
    return q[order], kind[order]


def dist2(q, pts):
    """L2_Simple in float32: the squares accumulated x, then y, then z."""
    dx, dy, dz = (q[0] - pts[:, 0]).astype(F), (q[1] - pts[:, 1]).astype(F), (q[2] - pts[:, 2]).astype(F)
    return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)


def bin_cubes(cloud, dims=DIMS, cube=CUBE, origin=ORIGIN):
    """Array cell -> its points in input order (pushCornerPoint / pushSurfPoint), by the fixed cube_index."""
    cloud = np.ascontiguousarray(cloud, F)
    ijk = cube_index(cloud, cube, origin)
    ok = np.all((ijk >= 0) & (ijk < np.asarray(dims)), axis=1)
    idx = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]
    return {int(c): cloud[ok & (idx == c)] for c in np.unique(idx[ok])}


def cell_of(q, dims=DIMS, cube=CUBE, origin=ORIGIN):
    """Array cell of every query, -1 outside the array (and for a coordinate that is not finite)."""
    ijk = cube_index(q, cube, origin)
    ok = np.all((ijk >= 0) & (ijk < np.asarray(dims)), axis=1)
    return np.where(ok, ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1], -1)


class Reference:
    """Per query: has its cube a tree; nanoflann's five there (the oracle); the in-cube and the global brute force in float32."""

    def __init__(self, oracle, cloud, q, dims=DIMS, cube=CUBE, origin=ORIGIN, cubes=None, cells=None):
        q = np.ascontiguousarray(q, F)
        self.cubes = bin_cubes(cloud, dims, cube, origin) if cubes is None else cubes
        self.cell = cell_of(q, dims, cube, origin) if cells is None else cells
        nq = len(q)
        self.ok = np.zeros(nq, bool)
        self.xyz, self.d2 = np.zeros((nq, 5, 3), F), np.zeros((nq, 5), F)
        self.brute_d2 = np.zeros((nq, 5), F)
        self.tie = np.zeros(nq, bool)      # an exact tie among the six nearest in the cube
        self.border = np.zeros(nq, bool)   # the global five are not the in-cube five
        trees = {}
        everything = np.concatenate(list(self.cubes.values()), 0) if self.cubes else np.zeros((0, 4), F)
        for i in range(nq):
            pts = self.cubes.get(int(self.cell[i])) if self.cell[i] >= 0 else None
            if pts is None or len(pts) < 5:
                continue
            c = int(self.cell[i])
            if c not in trees:
                trees[c] = oracle.kdtree(pts)
            idx, d = trees[c].knn(q[i:i + 1], 5)
            self.ok[i] = True
            self.xyz[i], self.d2[i] = pts[idx[0], :3], d[0]
            b = np.sort(dist2(q[i], pts), kind="stable")
            self.brute_d2[i] = b[:5]
            self.tie[i] = bool(np.any(np.diff(b[:6]) == 0))
            g = np.sort(dist2(q[i], everything), kind="stable")[:5]
            self.border[i] = not np.array_equal(g.view(np.uint32), b[:5].view(np.uint32))


class Case:
    """The wall map and its queries, both types, with their references."""

    def __init__(self, oracle):
        self.map = [make_map(0), make_map(1)]
        qk = [make_queries(0), make_queries(1)]
        self.q = [qk[0][0], qk[1][0]]
        self.kind = [qk[0][1], qk[1][1]]
        self.ref = [Reference(oracle, self.map[t], self.q[t]) for t in range(2)]


# ---- a map whose corner type gets no cell grid: 400 points over a 170 m box in ONE 200 m cube (more cells than 4 096 a point) ----
NOGRID_DIMS, NOGRID_CUBE, NOGRID_ORIGIN = (9, 9, 5), 200.0, (4, 4, 2)


def make_nogrid_case(oracle):
    rng = np.random.default_rng(6300)
    corner = rng.uniform(-85.0, 85.0, (400, 3)).astype(F)
    surf = rng.uniform((-2.0, -2.0, -0.25), (2.0, 2.0, 0.25), (300, 3)).astype(F)
    clouds = [np.concatenate([c, np.arange(len(c), dtype=F)[:, None]], 1) for c in (corner, surf)]
    qc = np.concatenate([corner[:150] + rng.normal(0, 0.5, (150, 3)), rng.uniform(-99.0, 99.0, (100, 3)), rng.uniform(101.0, 120.0, (7, 3))], 0)
    qs = np.concatenate([np.zeros((1, 3)), rng.uniform((-1.8, -1.8, -0.2), (1.8, 1.8, 0.2), (150, 3))], 0)
    qc[0] = (0.5, 0.5, 0.5)
    q = [qc.astype(F), qs.astype(F)]
    ref = [Reference(oracle, clouds[t], q[t], NOGRID_DIMS, NOGRID_CUBE, NOGRID_ORIGIN) for t in range(2)]
    return clouds, q, ref


# ---- the gate (d2[4] < 5.0) and GRID_FAR through the loop: a scene that holds still --------------------------------------------
# Map and scan lie in cube (0, 0, 0).  Surf map: the planes x = 4.5, y = 4.5, z = 4.5 on a 0.5 m lattice over [-1.0, 4.5]; corner
# map: three lines on the same lattice.  The scan's points lie IN those planes at the identity pose: every residual is zero (to
# the plane fit's rounding) and the pose stays; three perpendicular planes give the normal matrix full rank by themselves.  The
# scan has NO corner points: for a point exactly on its line the reference's corner coefficient divides 0 by 0 (a012 = 0) and
# ``oracle.scanmatch_cubes`` returns a pose that is not a number -- checked on the CPU -- so the lines stay in the map unqueried.
# Around the centre (1.5, 1.5) of every plane a hole is cut that leaves four points at squared distance 1 and two at exactly 5 --
# offsets (+1, +-2), on the + side of the first in-plane axis -- so that the scan point at the centre has d2[4] = 5.0 (the plane
# z = 4.5), 5 - 2^-21 when moved by +2^-22 (x = 4.5) and 5 + 2^-21 when moved by -2^-22 (y = 4.5): one float below and one above
# the gate.  The other scan points of a plane sit on a 0.6 m raster off the lattice; those are kept whose five nearest lie in
# their own plane with a fifth squared distance below 1.5.  (The box starts at -1.0 so that the planes do not fall on a wall of
# the grid's 0.6 m cells: points in them can then be proven by the grid.)  Four more surf points lie in the plane z = 4.5 beyond
# the map's bounding box: by sqrt(5) -+ 0.04 m, and by more than the grid's margin of 3 m (GRID_FAR).
GATE_SCAN_LEAF = 0.4
GATE_AXES = ((2, 0, 1), (0, 1, 2), (1, 0, 2))  # per plane: its normal axis, its first and its second in-plane axis
GATE_SHIFT = (0.0, 2.0 ** -22, -(2.0 ** -22))  # per plane: where its gate point sits along the first in-plane axis
GATE_D2 = (5.0, 5.0 - 2.0 ** -21, 5.0 + 2.0 ** -21)


def make_gate_scene():
    """-> dict(map_corner, map_surf, corner (empty), surf (n, 4) float32; gate: indices of the three gate points in surf; far: of the four
    far points; generic: of the rest)."""
    lat = -1.0 + 0.5 * np.arange(12)
    keep = {(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (1.0, 2.0), (1.0, -2.0)}
    ms, scan, gate, far = [], [], [], []
    for k, (n, a, b) in enumerate(GATE_AXES):
        for u in lat:
            for v in lat:
                if k > 0 and (u == 4.5 or v == 4.5):
                    continue  # the planes' common edges belong to the first plane... and to nobody: no point is stored twice
                du, dv = u - 1.5, v - 1.5
                if du * du + dv * dv <= 5.0 and (du, dv) not in keep:
                    continue
                p = np.zeros(3)
                p[n], p[a], p[b] = 4.5, u, v
                ms.append(p)
    ms = np.asarray(ms, F)
    for k, (n, a, b) in enumerate(GATE_AXES):
        g = np.zeros(3, F)
        g[n], g[a], g[b] = 4.5, F(1.5) + F(GATE_SHIFT[k]), 1.5
        gate.append(len(scan))
        scan.append(g)
        for i in range(8):
            for j in range(8):
                p = np.zeros(3, F)
                p[n], p[a], p[b] = 4.5, -0.93 + 0.6 * i, -0.87 + 0.6 * j
                d = dist2(p, ms)
                five = np.argsort(d, kind="stable")[:5]
                # a generic point: its five nearest lie in its own plane, well inside the gate (not in the hole, not at an edge)
                if np.all(ms[five, n] == F(4.5)) and d[five[4]] < 1.5:
                    scan.append(p)
    lo = -1.0
    for x, y in ((lo - 2.2, 1.57), (lo - 2.28, 2.77), (lo - 3.2, 0.37), (lo - 3.4, 3.17)):
        far.append(len(scan))
        scan.append(np.array([x, y, 4.5], F))
    mc = []
    for fixed, a in ((((0, 1.0), (1, 1.0)), 2), (((1, -2.0), (2, 2.0)), 0), (((0, -2.0), (2, -2.0)), 1)):
        for s in -3.0 + 0.5 * np.arange(11):
            p = np.zeros(3)
            for ax, val in fixed:
                p[ax] = val
            p[a] = s
            mc.append(p)

    def cloud(pts):
        pts = np.asarray(pts, F).reshape(-1, 3)
        return np.concatenate([pts, np.arange(len(pts), dtype=F)[:, None]], 1)
    surf = cloud(scan)
    generic = [i for i in range(len(surf)) if i not in gate and i not in far]
    return dict(map_corner=cloud(mc), map_surf=cloud(ms), corner=np.zeros((0, 4), F), surf=surf, gate=gate, far=far, generic=generic)


def gate_reference(oracle, scene):
    """The restatement of the node the gate scene runs on."""
    ref = lr.RefLocalization(oracle, DIMS, CUBE, ORIGIN, filter_corner=GATE_SCAN_LEAF, filter_surf=GATE_SCAN_LEAF)
    ref.set_map(scene["map_corner"], scene["map_surf"], filter=False)
    return ref
