"""Scene builders for the voxel filter's edge cases (numpy only, no GPU): tests/test_voxel_cases.py holds them against the
oracle alone, tests/test_gpu_voxel_edges.py runs them through every entry of the device's one filter pipeline
(fm_key_kernel, sort or merge, scan, fm_centroid_kernel in csrc/lslam_fmap.hip) and the survey's voxel_grid_min.

  run_shapes(leaf, tail)   voxels with prescribed member counts at prescribed places of the sorted order: where a voxel's run
                           starts and ends relative to the 64-lane wavefront and the 256-entry workgroup decides which part of
                           fm_centroid_kernel sums it (neighbours' registers, or the continuation loop over chunks of 64)
  signed_zero_cloud()      voxels whose members are -0.0f in one field: pcl::VoxelGrid sums from a zero vector, and
                           0.0f + -0.0f = +0.0f
  wall_cloud(leaf)         coordinates on and next to voxel walls fl(k * leaf): the voxel index is floor(fl(v * fl(1 / leaf))),
                           which differs from floor(fl(v / leaf)) and from the real quotient there
  guard_clouds()           one cell either side of applyFilter's "leaf too small" guard (more voxels than INT_MAX: the input
                           comes back as it is)
  cube_scene()             the same ingredients for the cube map (FeatureMap): cube faces, cubes outside the active area,
                           points outside the grid, long runs, alternating and uniform stretches of cubes

All coordinates stay far below 2^24 * leaf in magnitude: the oracle subtracts min_b from the floor in float
(fmap_oracle.c:91-93), the device in int, and the two agree only while floor(v / leaf) is an integer a float holds exactly.
Every point is finite: the oracle restates PCL for dense clouds and include/lslam_c.h promises nothing for NaN or Inf."""
import numpy as np

F = np.float32
SEED = 4  # the order-sensitivity condition of tests/test_voxel_cases.py holds for this seed (0 voxels exempt)
NEG_ZERO, POS_ZERO = 0x80000000, 0x00000000
LEAVES = (0.2, 0.4, 0.5, 0.05)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def negzero():
    return F(-0.0)


def voxel_index(v, leaf):
    """floor(fl(v * fl(1 / leaf))) as pcl::VoxelGrid, the oracle and fm_key_kernel form it (fp32 throughout) -> int64."""
    inv = F(1.0) / F(leaf)
    return np.floor(np.asarray(v, F) * inv).astype(np.int64)


def xyzi32(cloud):
    """The 32-byte pcl::PointXYZI layout of an (n, 4) cloud: x y z pad intensity pad pad pad."""
    c = np.ascontiguousarray(cloud, F)
    out = np.zeros((len(c), 8), F)
    out[:, :3] = c[:, :3]
    out[:, 3] = 1.0
    out[:, 4] = c[:, 3]
    return out


# ---- run shapes ------------------------------------------------------------------------------------------------------------
LONG_RUNS = ((65, 17), (128, 40), (129, 63), (192, 1), (193, 33))  # (members, lane of the head)
LAST_RUN = 70


def run_shapes(leaf, tail=0, seed=SEED):
    """-> dict: cloud (n, 4) in a shuffled input order, labels (n,) the voxel number of every input point, counts / starts per
    voxel in sorted order (what fm_centroid_kernel sees: voxels ascending, members in input order), items {name: (start,
    count)}, n.  tail: n % 64 (0 or 1); the last voxel's run ends exactly at n.  Voxels lie side by side along x, one cell in
    y and z."""
    rng = np.random.default_rng(seed)
    counts, items = [], {}
    pos = 0

    def put(c, name=None):
        nonlocal pos
        if name:
            items[name] = (pos, c)
        counts.append(c)
        pos += c

    def pad_to(lane, mod=64):  # single-member voxels up to the wanted place
        while pos % mod != lane:
            put(1)

    put(64, "run64_at_lane0")          # lanes 0..63 of the first wavefront; the continuation finds nothing
    put(1, "head_at_lane0_behind_run64")
    pad_to(63)
    put(1, "single_at_lane63")
    pad_to(63)
    put(3, "run3_at_lane63")           # a head at lane 63: every member comes from memory
    for cnt, lane in LONG_RUNS:
        put(1)
        pad_to(lane)
        put(cnt, "run%d" % cnt)
    put(1)
    pad_to(200, 256)
    put(300, "run300_across_a_workgroup")
    put(1)
    pad_to(5)
    put(1100, "run1100_over_workgroups")
    put(1)
    pad_to((tail - LAST_RUN) % 64)
    put(LAST_RUN, "last_run")
    n = pos
    assert n % 64 == tail and n <= 12000
    counts = np.array(counts, np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    nvox = len(counts)
    v0 = -(nvox // 3)  # voxel indices on both sides of zero
    labels = rng.permutation(np.repeat(np.arange(nvox), counts))
    cloud = np.zeros((n, 4), F)
    lf = float(F(leaf))
    cloud[:, 0] = ((v0 + labels) + rng.uniform(0.1, 0.9, n)) * lf  # full random mantissas inside the voxel
    cloud[:, 1] = rng.uniform(0.1, 0.9, n) * lf
    cloud[:, 2] = -rng.uniform(0.1, 0.9, n) * lf
    cloud[:, 3] = 10.0 ** rng.uniform(-3.0, 3.0, n)
    assert np.array_equal(voxel_index(cloud[:, 0], leaf), v0 + labels)
    assert (voxel_index(cloud[:, 1], leaf) == 0).all() and (voxel_index(cloud[:, 2], leaf) == -1).all()
    return dict(cloud=cloud, labels=labels, counts=counts, starts=starts, items=items, n=n)


def sorted_by_voxel(shape):
    """The cloud in the order the sort produces (voxels ascending, members in input order)."""
    return shape["cloud"][np.argsort(shape["labels"], kind="stable")]


# ---- signed zeros ------------------------------------------------------------------------------------------------------------
def signed_zero_cloud(seed=SEED):
    """-> (cloud (n, 4), cases, all_zero).  A case: dict(kind, field, rows (input rows of the voxel's members), tag_axis, tag
    (lo, hi): the voxel's output is the one row whose tag_axis coordinate lies in [lo, hi]), all_negative (every member is
    -0.0f in `field`: the oracle's output field is +0.0f), expect_bits (of the output field, None where it is an ordinary
    number).  all_zero: the input row that is -0.0f in all four fields, alone in the voxel at the origin.
    Valid for leaves from 0.05 to 1.0: voxels are 2 m apart, members of one voxel within 0.01 m of each other and 0.27 m
    from the nearest wall."""
    rng = np.random.default_rng(seed)
    rows, cases = [], []

    def voxel(kind, field, values):
        g = len(cases)
        tag = 2.0 * g + 2.27
        idx = []
        for v in values:
            p = np.array([tag, 4.27, 6.27, 1.5], np.float64) + rng.uniform(0.0, 0.009, 4)
            tag_axis = 0
            if field == 0:  # x is the zero: the tag goes to y
                p[1] = tag + rng.uniform(0.0, 0.009)
                tag_axis = 1
            p = p.astype(F)
            p[field] = v
            idx.append(len(rows))
            rows.append(p)
        neg = all(bits(F(v)) == NEG_ZERO for v in values)
        zero = all(F(v) == 0 for v in values)
        cases.append(dict(kind=kind, field=field, rows=idx, tag_axis=tag_axis, tag=(tag - 0.001, tag + 0.01), all_negative=neg,
                          expect_bits=POS_ZERO if zero else None))

    nz, pz = negzero(), F(0.0)
    for f in range(4):
        voxel("single", f, [nz])
    for f in range(4):
        voxel("several", f, [nz, nz, nz])
    for f in range(4):
        voxel("pair", f, [nz, nz])
    for f in range(4):
        voxel("mixed", f, [nz, pz, nz])
        voxel("mixed", f, [pz, nz])
    for f in range(4):
        voxel("with_nonzero", f, [nz, F(0.01)])  # no sign issue: the sum is the other member
        voxel("with_nonzero", f, [F(0.01), nz])
    # every field at once, and the point that keeps every axis' minimum below zero (-0.0f falls into voxel 0 of min_b < 0)
    all_zero = len(rows)
    rows.append(np.array([nz, nz, nz, nz], F))
    rows.append(np.array([-3.1, -3.1, -3.1, 2.0], F))
    cloud = np.stack(rows).astype(F)
    assert (cloud[:, :3].min(0) < 0).all()
    return cloud, cases, all_zero


def find_output(out, case):
    """The row of a filter result that is the case's voxel."""
    lo, hi = case["tag"]
    c = out[:, case["tag_axis"]]
    hit = np.nonzero((c >= lo) & (c <= hi))[0]
    assert len(hit) == 1, (case, hit)
    return out[hit[0]]


# ---- voxel walls ---------------------------------------------------------------------------------------------------------------
WALL_K = 96  # walls k * leaf for k in [-WALL_K, WALL_K]


def wall_values(leaf):
    """fl(k * leaf), formed as an fp32 product of the fp32 leaf and as the decimal product rounded once, with two fp32
    neighbours on each side."""
    ks = np.arange(-WALL_K, WALL_K + 1)
    base = np.concatenate([ks.astype(F) * F(leaf), (ks * float(leaf)).astype(F)])
    vals, up, dn = [base], base, base
    for _ in range(2):
        up = np.nextafter(up, F(np.inf))
        dn = np.nextafter(dn, F(-np.inf))
        vals += [up, dn]
    return np.unique(np.concatenate(vals)).astype(F)


def wall_cloud(leaf, seed=SEED):
    """-> (cloud (n, 4), axis (n,)): axis a in 0..2 -- the point sits on a wall of that axis and inside a voxel on the other
    two; 3 -- all three coordinates sit on walls."""
    rng = np.random.default_rng(seed)
    vals = wall_values(leaf)
    inside = F(1.37 * float(F(leaf)))
    parts, axes = [], []
    for a in range(3):
        p = np.full((len(vals), 4), inside, F)
        p[:, a] = vals
        parts.append(p)
        axes.append(np.full(len(vals), a))
    m = 400
    p = np.zeros((m, 4), F)
    for a in range(3):
        p[:, a] = vals[rng.integers(0, len(vals), m)]
    parts.append(p)
    axes.append(np.full(m, 3))
    cloud = np.concatenate(parts)
    axis = np.concatenate(axes)
    cloud[:, 3] = rng.uniform(0.0, 64.0, len(cloud))
    order = rng.permutation(len(cloud))
    return cloud[order], axis[order]


def wall_discriminators(cloud, axis, leaf):
    """Per axis: how many of the scene's wall coordinates a wrong index formula would put elsewhere -> (division[3], exact[3]).
    division: floor(fl(v * inv)) != floor(fl(v / leaf)); exact: fl(v * inv) is an integer k although v < k * leaf in real
    arithmetic (fp64 holds both sides exactly enough: a product of two fp32 values is exact in fp64)."""
    l32 = F(leaf)
    inv = F(1.0) / l32
    division, exact = [], []
    for a in range(3):
        v = cloud[(axis == a) | (axis == 3), a]
        prod = v * inv
        quot = v / l32
        division.append(int((np.floor(prod) != np.floor(quot)).sum()))
        k = np.floor(prod)
        exact.append(int(((prod == k) & (v.astype(np.float64) < k.astype(np.float64) * float(l32))).sum()))
    return division, exact


# ---- the "leaf too small" guard ------------------------------------------------------------------------------------------------
GUARD_LEAF = 1.0


def guard_clouds():
    """Three points at leaf 1.0 -> list of dict(name, cloud, filtered).  Extents (2047.5, 1023.5, 1023.5) make 2048 * 1024 * 1024
    = 2^31 voxels, one more than INT_MAX: the input comes back as it is, its -0.0f intensity included.  (2046.5, ...) makes
    2047 * 2^20 <= INT_MAX: filtered -- two of the points share a voxel, the far one has the highest index and comes last
    although it went in first, and its -0.0f intensity becomes +0.0f.  The long axis on x, y and z."""
    out = []
    for long_axis in range(3):
        for long_extent, filtered in ((2047.5, False), (2046.5, True)):
            ext = [1023.5, 1023.5, 1023.5]
            ext[long_axis] = long_extent
            cloud = np.array([ext + [-0.0], [0.0, 0.0, 0.0, 1.0], [0.25, 0.25, 0.25, 3.0]], F)
            assert bits(cloud)[0, 3] == NEG_ZERO
            out.append(dict(name="%s_%s" % ("xyz"[long_axis], "filtered" if filtered else "passed"), cloud=cloud, filtered=filtered))
    return out


# ---- the cube map --------------------------------------------------------------------------------------------------------------
CUBE_DIMS = (5, 5, 5)
CUBE_SIZE = 10.0
CUBE_VALID = 12.0
CUBE_WIDE_VALID = 45.0
CUBE_LEAVES = (0.4, 0.8, 1.5)  # corner, surf, map


def cube_scene(seed=SEED):
    """A 5 x 5 x 5 grid of 10 m cubes, valid distance 12 m, sensor at the world's origin.  update() puts the sensor's cube at
    index 1 of every axis (the reference clamps it to [3, size - 4]), so the grid then covers cube centres -10 .. 30 and the
    active area is the 27 cubes with centres in {-10, 0, 10}^3; cubes with a centre at 20 or 30 hold points and stay unfiltered.

    -> dict: T (identity whose zeros are -0.0f, so that a -0.0f coordinate survives pcl::transformPointCloud's
    ((r0 x + r1 y) + r2 z) + t next to positive coordinates), pos, old = (corner, surf) pushed before the first update(),
    adds = [(corner, surf), (corner, surf)] the second without an update() before it, marks: where the planted voxels come out.

    corner clouds: consecutive points alternating between four cubes (one of them outside the active area); 320 consecutive
    points of one cube, 150 of them in one 0.4 m voxel; points on cube faces x / 10 = +-0.5, +-1.5 on every axis (roundf rounds
    half away from zero; -1.5 leaves the grid); points outside the grid; -0.0f coordinates and intensities in filtered cubes
    and in a cube that stays unfiltered.  surf clouds: only cubes of the active area, the highest one's highest voxel with 140
    members, and points outside the grid -- dropped keys directly behind a long run."""
    rng = np.random.default_rng(seed)
    nz = negzero()
    T = np.eye(4, dtype=F)
    T[T == 0] = nz

    def xyzi(p, w=None):
        out = np.zeros((len(p), 4), F)
        out[:, :3] = p
        out[:, 3] = rng.uniform(0.0, 16.0, len(p)) if w is None else w
        return out

    def in_cube(centre, n, half=4.9):
        return np.asarray(centre, np.float64) + rng.uniform(-half, half, (n, 3))

    # before the first update(): the grid covers centres -20 .. 20; what lies in [-15, 25) survives the shift
    old_corner = xyzi(rng.uniform(-14.0, 24.0, (400, 3)))
    old_surf = xyzi(rng.uniform(-14.0, 14.0, (400, 3)))
    bits(old_corner)[::50, 3] = NEG_ZERO

    centres = [(0, 0, 0), (10, 0, 0), (0, 10, 0), (20, 0, 0)]
    alt = np.zeros((600, 3))
    for i in range(len(alt)):
        alt[i] = in_cube(centres[i % 4], 1)[0]
    uniform = in_cube((10, 10, 0), 320)
    uniform[100:250] = np.array([8.0, 8.0, 1.2]) + rng.uniform(0.04, 0.36, (150, 3))  # one voxel of leaf 0.4
    faces = []
    for a in range(3):
        for f in (0.5, -0.5, 1.5, -1.5):
            for _ in range(3):
                p = rng.uniform(1.0, 4.0, 3)
                p[a] = f * CUBE_SIZE
                faces.append(p)
    faces = np.array(faces)
    outside = np.array([[47.0, 1.0, 1.0], [1.0, -31.0, 2.0], [2.0, 3.0, 55.0], [-16.0, 1.0, 1.0]])
    # -0.0f in filtered cubes: x of three members in cube (0, 10, 10); the intensity of three members in cube (10, 0, 10)
    zx = np.array([0.0, 9.3, 11.7]) + np.concatenate([np.zeros((3, 1)), rng.uniform(0.0, 0.05, (3, 2))], 1)
    zx = xyzi(zx, 2.5)
    zx[:, 0] = nz
    zw = xyzi(np.array([12.1, 2.1, 12.1]) + rng.uniform(0.0, 0.05, (3, 3)), nz)
    # ... and in cube (0, 20, 0), which stays outside the active area: x and intensity
    zu = xyzi(np.array([[0.0, 21.3, 1.7], [3.0, 22.0, 2.0]]), nz)
    zu[0, 0] = nz
    corner_a = np.concatenate([xyzi(alt), xyzi(uniform), xyzi(faces), zx, xyzi(outside), zw, zu])
    assert bits(corner_a)[:, 0].tolist().count(NEG_ZERO) == 4

    top = in_cube((10, 10, 10), 300)
    top[:, 2] = np.minimum(top[:, 2], 14.3)  # below the highest voxel layer of leaf 0.8 ([14.4, 15.2))
    run = np.array([14.5, 14.5, 14.5]) + rng.uniform(0.0, 0.1, (140, 3))
    mid = np.concatenate([in_cube((0, 0, 0), 300), in_cube((-10, 10, 0), 200)])
    surf_a = np.concatenate([xyzi(mid[:250]), xyzi(outside[:2]), xyzi(top), xyzi(run[:70]), xyzi(mid[250:]), xyzi(run[70:]),
                             xyzi(outside[2:])])

    more = np.array([8.0, 8.0, 1.2]) + rng.uniform(0.04, 0.36, (130, 3))
    spread = rng.uniform(-14.0, 24.0, (800, 3))
    corner_b = np.concatenate([xyzi(spread[:400]), xyzi(more), xyzi(spread[400:]), xyzi(outside)])
    bits(corner_b)[::37, 3] = NEG_ZERO
    surf_b = np.concatenate([xyzi(rng.uniform(-14.0, 14.0, (500, 3))), xyzi(np.array([14.5, 14.5, 14.5]) + rng.uniform(0.0, 0.1, (135, 3))),
                             xyzi(outside)])
    marks = dict(
        filtered_x=dict(box=((-0.01, 0.01), (9.2, 9.6), (11.6, 12.0)), field=0),       # +0.0f x from three -0.0f members
        filtered_w=dict(box=((12.0, 12.4), (2.0, 2.4), (12.0, 12.4)), field=3),        # +0.0f intensity
        unfiltered=dict(box=((-0.01, 0.01), (21.2, 21.4), (1.6, 1.8)), fields=(0, 3)))  # -0.0f x and intensity, as they went in
    return dict(T=T, pos=np.zeros(3, F), old=(old_corner, old_surf), adds=[(corner_a, surf_a), (corner_b, surf_b)], marks=marks)


def find_in_box(cloud, box):
    m = np.ones(len(cloud), bool)
    for a, (lo, hi) in enumerate(box):
        m &= (cloud[:, a] >= lo) & (cloud[:, a] <= hi)
    return cloud[m]


def setup_cube_map(m, valid=CUBE_VALID):
    m.setup_world_cube_size(CUBE_SIZE)
    m.setup_lidar_valid_distance(valid)
    m.setup_filter_size(*CUBE_LEAVES)


def cube_steps(scene):
    """The sequence both maps go through -> list of (name, function of a map).  The last step widens the valid distance: the
    cubes that stayed unfiltered enter the surround as they are, which is the only place their points can be seen raw."""
    T, pos = scene["T"], scene["pos"]
    steps = [("add before update", lambda m: m.add_feature_cloud(scene["old"][0], scene["old"][1], T)),
             ("update", lambda m: m.update(pos)),
             ("add", lambda m: m.add_feature_cloud(scene["adds"][0][0], scene["adds"][0][1], T)),
             ("add again without update", lambda m: m.add_feature_cloud(scene["adds"][1][0], scene["adds"][1][1], T))]

    def widen(m):
        m.setup_lidar_valid_distance(CUBE_WIDE_VALID)
        m.update(pos)
    return steps, ("update with a wider valid distance", widen)
