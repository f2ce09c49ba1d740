"""The scenes of tests/voxel_cases.py against the oracle alone (no GPU): the layouts hold what they promise, the values make
the order of a voxel's sum visible, and oracle/fmap_oracle.c is a specification on them -- +0.0f out of -0.0f members, the
multiply-by-the-inverse voxel index on the walls, the guard one cell either side of INT_MAX, raw points in cubes outside the
active area.  tests/test_gpu_voxel_edges.py runs the same scenes on the device."""
import numpy as np
import pytest

import voxel_cases as V
from voxel_cases import F, NEG_ZERO, POS_ZERO, bits


# ---- run shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("leaf", [0.4, 0.05])
def test_run_shapes_layout(leaf, tail):
    s = V.run_shapes(leaf, tail)
    it, counts, starts, n = s["items"], s["counts"], s["starts"], s["n"]
    assert n == counts.sum() == len(s["cloud"]) <= 12000 and n % 64 == tail
    # what the sort produces really has this layout
    lab = np.sort(s["labels"], kind="stable")
    assert np.array_equal(np.nonzero(np.diff(lab, prepend=-1))[0], starts)
    # heads at lane 63, with one member and with more
    assert it["single_at_lane63"][0] % 64 == 63 and it["single_at_lane63"][1] == 1
    assert it["run3_at_lane63"][0] % 64 == 63 and it["run3_at_lane63"][1] >= 2
    # exactly one wavefront from lane 0, the next head at lane 0
    assert it["run64_at_lane0"] == (0, 64) and it["head_at_lane0_behind_run64"][0] == 64
    assert 64 in starts
    # long runs from lanes other than 0; the continuation's full chunks (L == 64)
    twice = 0
    for cnt, lane in V.LONG_RUNS:
        start, c = it["run%d" % cnt]
        assert c == cnt and start % 64 == lane and lane != 0
        in_wave = 64 - lane  # the head and the members behind it in its wavefront
        assert cnt > in_wave
        twice += (cnt - in_wave) // 64 >= 2
    assert {c for c, _ in V.LONG_RUNS} == {65, 128, 129, 192, 193} and twice >= 1
    assert sum(lane not in (0, 63) for _, lane in V.LONG_RUNS) >= 4
    start, c = it["run300_across_a_workgroup"]
    assert c >= 257 and start % 256 != 0 and start // 256 != (start + c - 1) // 256
    start, c = it["run1100_over_workgroups"]
    assert c >= 1000 and (start + c - 1) // 256 - start // 256 >= 4
    start, c = it["last_run"]
    assert start + c == n and c > 64 - start % 64  # ends at n, and ends in the continuation
    # single-member voxels between the long runs
    big = np.nonzero(counts >= 64)[0]
    assert len(big) >= 9
    for a, b in zip(big[:-1], big[1:]):
        assert (counts[a + 1:b] == 1).any(), (a, b)


def _seq(a):
    s = np.zeros(a.shape[1], F)  # from zero, as the oracle
    for p in a:
        s = s + p
    return s


def _tree(a):
    if len(a) == 1:
        return a[0].copy()
    return _tree(a[:len(a) // 2]) + _tree(a[len(a) // 2:])


ORDER_SENSITIVE_VOXELS = {0: 10, 1: 10}  # voxels with >= 3 members per tail


@pytest.mark.parametrize("tail", [0, 1])
def test_run_shapes_sums_depend_on_the_order(tail):
    """A condition on the scene: in EVERY voxel with three or more members the fp32 sum in input order differs, in at least one
    field, from the sum in reversed order and from the pairwise (tree) sum -- a kernel that adds a run's members in another
    order cannot give the oracle's bits.  No voxel is exempt (voxel_cases.SEED was picked for that)."""
    for leaf in V.LEAVES:
        s = V.run_shapes(leaf, tail)
        c = V.sorted_by_voxel(s)
        checked = 0
        for start, cnt in zip(s["starts"], s["counts"]):
            if cnt < 3:
                continue
            m = c[start:start + cnt]
            fwd = _seq(m)
            assert (bits(fwd) != bits(_seq(m[::-1]))).any(), (leaf, start, cnt, "reversed")
            assert (bits(fwd) != bits(_tree(m))).any(), (leaf, start, cnt, "pairwise")
            checked += 1
        assert checked == ORDER_SENSITIVE_VOXELS[tail]


@pytest.mark.parametrize("leaf", V.LEAVES)
def test_run_shapes_oracle_counts(oracle, leaf):
    s = V.run_shapes(leaf, 1)
    out = oracle.voxel_grid(s["cloud"], leaf)
    assert len(out) == len(s["counts"])
    c = V.sorted_by_voxel(s)
    for name in ("run3_at_lane63", "run193", "last_run"):
        start, cnt = s["items"][name]
        k = int(np.searchsorted(s["starts"], start))
        assert np.array_equal(bits(out[k]), bits(_seq(c[start:start + cnt]) / F(cnt))), name


# ---- signed zeros ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", V.LEAVES + (1.0,))
def test_signed_zero_cloud_oracle_gives_positive_zero(oracle, leaf):
    cloud, cases, all_zero = V.signed_zero_cloud()
    assert {c["kind"] for c in cases} == {"single", "several", "pair", "mixed", "with_nonzero"}
    for kind in ("single", "several", "mixed", "with_nonzero"):
        assert {c["field"] for c in cases if c["kind"] == kind} == {0, 1, 2, 3}
    assert (voxel_min_index(cloud, leaf) < 0).all()
    out = oracle.voxel_grid(cloud, leaf)
    assert len(out) == len(cases) + 2
    n_neg = 0
    for c in cases:
        members = cloud[c["rows"]]
        assert len(np.unique(V.voxel_index(members[:, :3], leaf), axis=0)) == 1  # one voxel at this leaf
        row = V.find_output(out, c)
        f = c["field"]
        if c["all_negative"]:
            assert (bits(members)[:, f] == NEG_ZERO).all() and bits(row)[f] == POS_ZERO, c
            n_neg += 1
        elif c["expect_bits"] is not None:
            assert bits(row)[f] == c["expect_bits"], c
        else:
            assert row[f] == F(0.01) / F(2.0), c  # the nonzero member decides, in either order
    assert n_neg == 12
    zero_row = out[(out[:, :3] == 0).all(1)]
    assert len(zero_row) == 1 and (bits(zero_row) == POS_ZERO).all() and (bits(cloud[all_zero]) == NEG_ZERO).all()


def voxel_min_index(cloud, leaf):
    return V.voxel_index(cloud[:, :3].min(0), leaf)


# ---- voxel walls ---------------------------------------------------------------------------------------------------------------
# measured from the builder (per axis x, y, z): points where floor(fl(v * inv)) != floor(fl(v / leaf)), and points where
# fl(v * inv) is an integer k while v < k * leaf
WALL_MIN = {0.2: dict(division=(39, 37, 34), exact=(162, 148, 151)), 0.4: dict(division=(39, 37, 34), exact=(162, 148, 151))}


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_wall_cloud_discriminates(leaf):
    cloud, axis = V.wall_cloud(leaf)
    division, exact = V.wall_discriminators(cloud, axis, leaf)
    print("wall discriminators leaf", leaf, "division", division, "exact", exact)
    for a in range(3):
        assert division[a] >= WALL_MIN[leaf]["division"][a] > 0, (leaf, a, division)
        assert exact[a] >= WALL_MIN[leaf]["exact"][a] > 0, (leaf, a, exact)


@pytest.mark.parametrize("leaf", V.LEAVES)
def test_wall_cloud_oracle_uses_the_inverse_product(oracle, leaf):
    """The oracle's grouping is the one floor(fl(v * inv)) gives: as many outputs as distinct index triples, in ascending
    (z, y, x) order -- and on this scene that is not what a division gives (leaves 0.2 and 0.4)."""
    cloud, axis = V.wall_cloud(leaf)
    assert set(axis.tolist()) == {0, 1, 2, 3} and np.isfinite(cloud).all()
    assert np.abs(cloud[:, :3]).max() < 2.0 ** 24 * leaf / 1024
    out = oracle.voxel_grid(cloud, leaf)
    ijk = V.voxel_index(cloud[:, :3], leaf)
    uniq = np.unique(ijk[:, ::-1], axis=0)[:, ::-1]  # ascending in (z, y, x)
    assert len(out) == len(uniq)
    # a single-member voxel comes out as the point itself (0 + x, x / 1), at its place in the order
    first = {tuple(u): k for k, u in enumerate(uniq)}
    keys, cnt = np.unique(ijk, axis=0, return_counts=True)
    singles = {tuple(k) for k, c in zip(keys, cnt) if c == 1}
    seen = 0
    for p, v in zip(cloud, ijk):
        if tuple(v) in singles and (p != 0).all():
            assert np.array_equal(bits(out[first[tuple(v)]]), bits(p))
            seen += 1
    assert seen > 100
    if leaf in (0.2, 0.4):
        other = np.floor(cloud[:, :3] / F(leaf)).astype(np.int64)
        assert len(np.unique(other, axis=0)) != len(uniq) or (other != ijk).any()


# ---- the guard ---------------------------------------------------------------------------------------------------------------
def test_guard_clouds_oracle(oracle):
    clouds = V.guard_clouds()
    assert len(clouds) == 6 and sum(g["filtered"] for g in clouds) == 3
    for g in clouds:
        c = g["cloud"]
        ext = (c[:, :3].max(0) - c[:, :3].min(0)).astype(np.int64) + 1
        vol = int(ext[0]) * int(ext[1]) * int(ext[2])
        out = oracle.voxel_grid(c, V.GUARD_LEAF)
        if g["filtered"]:
            assert vol == 2047 << 20 and vol <= 2 ** 31 - 1
            assert len(out) == 2 and np.array_equal(out[0], np.array([0.125, 0.125, 0.125, 2.0], F)), g["name"]
            assert np.array_equal(bits(out[1, :3]), bits(c[0, :3])) and bits(out)[1, 3] == POS_ZERO
        else:
            assert vol == 2 ** 31
            assert out.shape == (3, 4) and np.array_equal(bits(out), bits(c)) and bits(out)[0, 3] == NEG_ZERO, g["name"]


# ---- the cube map ------------------------------------------------------------------------------------------------------------
def test_cube_scene_oracle(oracle):
    scene = V.cube_scene()
    marks = scene["marks"]
    ofm = oracle.feature_map(*V.CUBE_DIMS)
    V.setup_cube_map(ofm)
    steps, widen = V.cube_steps(scene)
    for name, step in steps:
        step(ofm)
    info = ofm.info()
    assert list(info["origin"]) == [1, 1, 1] and len(info["valid"]) == 27
    oc, os_ = ofm.get_surround_feature()
    # filtered voxels whose members were all -0.0f in one field come out as +0.0f
    for key in ("filtered_x", "filtered_w"):
        row = V.find_in_box(oc, marks[key]["box"])
        assert len(row) == 1 and bits(row)[0, marks[key]["field"]] == POS_ZERO, (key, row)
    assert len(V.find_in_box(oc, marks["unfiltered"]["box"])) == 0  # its cube is not part of the surround
    # consecutive points of the new cloud alternate between four cubes; 320 stay in one; a voxel takes 150 of them
    corner = scene["adds"][0][0]
    cube = np.round(corner[:600, :3] / F(V.CUBE_SIZE)).astype(int)
    assert len(np.unique(cube[:4], axis=0)) == 4 and (cube[:-4] == cube[4:]).all()
    assert len(np.unique(np.round(corner[600:920, :3] / F(V.CUBE_SIZE)).astype(int), axis=0)) == 1
    assert len(np.unique(V.voxel_index(corner[700:850, :3], 0.4), axis=0)) == 1
    q = corner[:, :3] / F(V.CUBE_SIZE)
    for a in range(3):
        assert {0.5, -0.5, 1.5, -1.5} <= set(q[:, a].tolist())
    # the surf cloud's last key is a long run, dropped points behind it
    run = V.find_in_box(os_, ((14.4, 15.2), (14.4, 15.2), (14.4, 15.2)))
    assert len(run) == 1 and os_[:, 2].max() == run[0, 2]
    # cubes outside the active area hold points; widened, they show them raw: -0.0f as it went in
    full_before = ofm.get_full_map()
    widen[1](ofm)
    info2 = ofm.info()
    assert len(info2["valid"]) > 27
    wc, _ = ofm.get_surround_feature()
    assert len(wc) > len(oc)
    raw = V.find_in_box(wc, marks["unfiltered"]["box"])
    assert len(raw) == 1 and all(bits(raw)[0, f] == NEG_ZERO for f in marks["unfiltered"]["fields"]), raw
    assert (bits(wc)[:, 3] == NEG_ZERO).sum() >= 2
    assert len(full_before) > 0 and (bits(full_before) != NEG_ZERO).all()  # the map filter sums everything from zero
