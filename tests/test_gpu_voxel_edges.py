"""The voxel filter's one kernel chain (fm_key_kernel, sort or fm_merge_kernel, scan, fm_centroid_kernel) and the survey's
sv_voxel_kernel against oracle/fmap_oracle.c on the scenes of tests/voxel_cases.py, through every entry that reaches them:
lslam_voxel_grid, lslam_voxel_grid2 in either position, the 32-byte PointXYZI stride, lslam_voxel_grid_min(1), the local map's
device-resident window and the cube map.  Every comparison is bit for bit (uint32 views, equal shapes); a mismatch names
the first differing row with its bit patterns.

What the scenes are for: runs placed against the 64-lane wavefront and the 256-entry workgroup (the continuation loop of
fm_centroid_kernel), -0.0f members (PCL sums from a zero vector: +0.0f out), coordinates on voxel walls (the index is
floor(fl(v * fl(1 / leaf)))), the "leaf too small" guard one cell either side of INT_MAX, cube faces and cubes outside the
active area.  tests/test_voxel_cases.py shows on the CPU that the scenes hold these and that the oracle decides them.

Out of scope: non-finite points.  The oracle restates PCL for dense clouds and include/lslam_c.h promises nothing for them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_cases as V
from local_map_ref import transform_cloud
from voxel_cases import F, NEG_ZERO, POS_ZERO, bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFILTER, KEY_ORDERED = 1, 2  # include/lslam_c.h LSLAM_LMAP_*


def assert_bits(got, ref, tag):
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    assert got.shape == ref.shape, (tag, "shape", got.shape, ref.shape)
    g, r = bits(got), bits(ref)
    if not np.array_equal(g, r):
        row = int(np.nonzero((g != r).any(1))[0][0])
        bad = int((g != r).any(1).sum())
        raise AssertionError("%s: %d of %d rows differ; first row %d: got %s (%s), oracle %s (%s)" % (
            tag, bad, len(g), row, ["%08x" % v for v in g[row]], got[row].tolist(), ["%08x" % v for v in r[row]], ref[row].tolist()))


def _scenes():
    out = {}
    for leaf, tail in ((0.4, 0), (0.4, 1), (0.05, 1), (0.2, 0)):
        out["runs_leaf%g_tail%d" % (leaf, tail)] = (V.run_shapes(leaf, tail)["cloud"], leaf)
    zero = V.signed_zero_cloud()[0]
    for leaf in (0.2, 0.5, 1.0):
        out["signed_zero_leaf%g" % leaf] = (zero, leaf)
    for leaf in V.LEAVES:
        out["walls_leaf%g" % leaf] = (V.wall_cloud(leaf)[0], leaf)
    for g in V.guard_clouds():
        out["guard_" + g["name"]] = (g["cloud"], V.GUARD_LEAF)
    return out


SCENES = _scenes()
_REF = {}


@pytest.fixture(scope="module")
def beside():
    """An unrelated cloud for the other position of lslam_voxel_grid2 (own extent, own min_b)."""
    rng = np.random.default_rng(31)
    c = (rng.uniform(-6, 6, (3000, 4)) + np.array([40.0, -25.0, 3.0, 0.0])).astype(F)
    c[:, 3] = rng.uniform(0, 64, len(c))
    return c


def reference(oracle, name):
    """oracle.voxel_grid of a scene, computed once and handed out read-only."""
    if name not in _REF:
        cloud, leaf = SCENES[name]
        ref = oracle.voxel_grid(cloud, leaf)
        ref.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


# ---- 1. every host entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_entries_match_oracle(pkg, ctx, oracle, beside, name):
    cloud, leaf = SCENES[name]
    ref = reference(oracle, name)
    if name.startswith("guard_") and name.endswith("passed"):
        assert_bits(ref, cloud, (name, "the oracle hands the input back"))
    one = pkg.voxel_grid(ctx, cloud, leaf)
    assert_bits(one, ref, (name, "voxel_grid"))
    side_ref = oracle.voxel_grid(beside, leaf)
    ga, gb = pkg.voxel_grid2(ctx, cloud, beside, leaf)
    assert_bits(ga, ref, (name, "voxel_grid2, position a"))
    assert_bits(gb, side_ref, (name, "voxel_grid2, the cloud beside it"))
    ga, gb = pkg.voxel_grid2(ctx, beside, cloud, leaf)
    assert_bits(gb, ref, (name, "voxel_grid2, position b"))
    assert_bits(ga, side_ref, (name, "voxel_grid2, the cloud beside it"))
    assert_bits(pkg.voxel_grid(ctx, V.xyzi32(cloud), leaf), ref, (name, "voxel_grid, 32-byte stride"))
    ga, gb = pkg.voxel_grid2(ctx, V.xyzi32(cloud), V.xyzi32(beside), leaf)
    assert_bits(ga, ref, (name, "voxel_grid2, 32-byte stride"))
    vmin = pkg.survey_map.voxel_grid_min(ctx, cloud, leaf, 1)
    assert_bits(vmin, ref, (name, "voxel_grid_min(1)"))
    assert_bits(vmin, one, (name, "voxel_grid_min(1) against voxel_grid"))


def test_signed_zero_outputs(pkg, ctx):
    """The planted voxels one by one, so that a failure names the voxel: every field whose members are all -0.0f comes out as
    +0.0f (bit pattern 0), a -0.0f next to a nonzero member changes nothing."""
    cloud, cases, all_zero = V.signed_zero_cloud()
    for leaf in (0.2, 1.0):
        out = pkg.voxel_grid(ctx, cloud, leaf)
        for c in cases:
            got = bits(V.find_output(out, c))[c["field"]]
            if c["expect_bits"] is not None:
                assert got == c["expect_bits"], (leaf, c["kind"], "field", c["field"], "members",
                                                 ["%08x" % v for v in bits(cloud[c["rows"]])[:, c["field"]]], "got %08x" % got)
            else:
                assert got == bits(F(0.01) / F(2.0)), (leaf, c, "%08x" % got)
        row = out[(out[:, :3] == 0).all(1)]
        assert len(row) == 1 and (bits(row) == POS_ZERO).all(), (leaf, ["%08x" % v for v in bits(row).ravel()])


# ---- 2. other input orders -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["reversed", "sorted"])
@pytest.mark.parametrize("leaf,tail", [(0.4, 0), (0.05, 1)])
def test_run_shapes_in_other_input_orders(pkg, ctx, oracle, order, leaf, tail):
    """Reversed, the members of every voxel are summed the other way round; sorted by voxel already, idx is the identity."""
    s = V.run_shapes(leaf, tail)
    cloud = s["cloud"][::-1].copy() if order == "reversed" else V.sorted_by_voxel(s)
    ref = oracle.voxel_grid(cloud, leaf)
    assert len(ref) == len(s["counts"])
    assert_bits(pkg.voxel_grid(ctx, cloud, leaf), ref, (order, leaf, tail))
    assert_bits(pkg.survey_map.voxel_grid_min(ctx, cloud, leaf, 1), ref, (order, leaf, tail, "voxel_grid_min(1)"))


# ---- 3. the device-resident form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,on_device", [(REFILTER, False), (KEY_ORDERED, False), (KEY_ORDERED, True)])
def test_device_resident_window(pkg, ctx, oracle, mode, on_device):
    """The local map's surround is lslam_voxel_grid over the window where it lies in HBM (include/lslam_c.h,
    lslam_lmap_get_surround): a frame whose surface cloud is run_shapes and whose corner cloud is signed_zero_cloud, then a
    second frame with the two swapped (the key-ordered window merges it in).  The frames' pose is the identity with -0.0f for
    its zeros, under which -0.0f coordinates next to positive ones survive pcl::transformPointCloud."""
    leaf = 0.4
    T = np.eye(4, dtype=F)
    T[T == 0] = V.negzero()
    shapes = [V.run_shapes(leaf, 1)["cloud"], V.run_shapes(leaf, 0, seed=V.SEED + 1)["cloud"]]
    zero = V.signed_zero_cloud()[0]
    moved = transform_cloud(T, zero)
    assert (bits(moved)[:, :3] == NEG_ZERO).sum() >= 30 and np.array_equal(bits(moved)[:, 3], bits(zero)[:, 3])
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 14, max_frames=8, mode=mode, filter_corner=leaf, filter_surf=leaf)
    frames = [(zero, shapes[0]), (shapes[1], zero)]
    win_c, win_s = np.zeros((0, 4), F), np.zeros((0, 4), F)
    for k, (c, s) in enumerate(frames):
        if on_device:
            import torch
            dev = torch.device("cuda", 0)
            lm.add_data_frame(torch.from_numpy(c).to(dev), torch.from_numpy(s).to(dev), T)
        else:
            lm.add_data_frame(c, s, T)
        win_c = np.concatenate([win_c, transform_cloud(T, c)])
        win_s = np.concatenate([win_s, transform_cloud(T, s)])
        gc, gs = lm.get_surround_feature()
        assert_bits(gc, oracle.voxel_grid(win_c, leaf), ("corner window", mode, on_device, k))
        assert_bits(gs, oracle.voxel_grid(win_s, leaf), ("surf window", mode, on_device, k))
    assert lm.info()["n_frames"] == 2
    lm.close()


# ---- 4. the cube map ---------------------------------------------------------------------------------------------------------
def _compare_maps(fm, ofm, tag):
    gi, oi = fm.info(), ofm.info()
    assert list(gi["origin"]) == list(oi["origin"]), tag
    assert np.array_equal(gi["valid"], oi["valid"]), tag
    gc, gs = fm.get_surround_feature()
    oc, os_ = ofm.get_surround_feature()
    assert_bits(gc, oc, (tag, "surround corner"))
    assert_bits(gs, os_, (tag, "surround surf"))
    assert_bits(fm.get_full_map(), ofm.get_full_map(), (tag, "full map"))
    return gc, gs


def test_cube_map_matches_oracle(pkg, ctx, oracle):
    """cube_scene() through FeatureMap and the oracle's: info, valid list, both surround clouds and the full map after every
    step -- add before update(), update(), add (the points pushed before are not in key order: everything is sorted), add again
    without update() (merged), and at last an update() with a wider valid distance, which shows the cubes that stayed
    unfiltered as they are."""
    scene = V.cube_scene()
    fm = pkg.FeatureMap(ctx, *V.CUBE_DIMS)
    ofm = oracle.feature_map(*V.CUBE_DIMS)
    for m in (fm, ofm):
        V.setup_cube_map(m)
    steps, widen = V.cube_steps(scene)
    for name, step in steps:
        step(fm)
        step(ofm)
        gc, gs = _compare_maps(fm, ofm, name)
    assert len(fm.info()["valid"]) == 27 and len(gc) > 500 and len(gs) > 300
    merged, resorted = fm.rebuild_stats()
    assert merged > 0 and resorted > 0, (merged, resorted)
    for key in ("filtered_x", "filtered_w"):
        row = V.find_in_box(gc, scene["marks"][key]["box"])
        assert len(row) == 1 and bits(row)[0, scene["marks"][key]["field"]] == POS_ZERO, (key, ["%08x" % v for v in bits(row).ravel()])
    widen[1](fm)
    widen[1](ofm)
    gc, gs = _compare_maps(fm, ofm, widen[0])
    raw = V.find_in_box(gc, scene["marks"]["unfiltered"]["box"])
    assert len(raw) == 1 and all(bits(raw)[0, f] == NEG_ZERO for f in scene["marks"]["unfiltered"]["fields"]), raw
    # the widened area is filtered by the next add: the raw -0.0f values become +0.0f there too
    empty = np.zeros((0, 4), F)
    fm.add_feature_cloud(empty, empty, scene["T"])
    ofm.add_feature_cloud(empty, empty, scene["T"])
    gc, gs = _compare_maps(fm, ofm, "empty add over the wider area")
    assert (bits(gc) != NEG_ZERO).all()
    fm.close()


# ---- the per-ring filter of the feature extractor (fx_ring_voxel_kernel: the same sums, in LDS) ---------------------------------
@pytest.mark.parametrize("leaf,want", [(0.2, POS_ZERO), (1.0e-4, NEG_ZERO)])
def test_ring_voxel_filter_signed_zero(pkg, ctx, oracle, synth, leaf, want):
    """A sweep whose intensities are all -0.0f: the less-flat list's VoxelGrid gives +0.0f in every voxel, and at a leaf that
    trips the guard the ring comes back unfiltered with -0.0f as it went in."""
    world = synth.World(half_extent=60.0, wall_half=55.0)
    _, _, _, cloud, ranges = synth.make_scan(world, 16, 900, full=True)
    cloud = cloud.copy()
    cloud[:, 3] = V.negzero()
    p, q = pkg.scan_registration.default_params(ctx), oracle.reg_params()
    for obj in (p, q):
        obj.less_flat_filter_size = leaf
    got = pkg.scan_registration.extract_features(ctx, cloud, ranges, p, taps=True)
    ref = oracle.extract_features(cloud, ranges, q)
    assert len(ref["less_flat"]) > 1000 and (bits(ref["less_flat"])[:, 3] == want).all()
    assert_bits(got["less_flat"], ref["less_flat"], ("less_flat", leaf))


# ---- 5. the same under the process-wide switches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["LSLAM_FMAP_MEASURED_EXTENTS", "LSLAM_SMALL_SORT"])
def test_entries_and_cube_map_under_a_switch(switch):
    """Both switches are read once per process: the host entries and the cube map again in one child pytest each --
    LSLAM_FMAP_MEASURED_EXTENTS=1 takes every rebuild's extents from the points (fm_minmax_kernel: alternating and uniform
    stretches of cubes), LSLAM_SMALL_SORT=1 sorts frame-sized inputs with lslam_sort.hip."""
    env = dict(os.environ)
    env[switch] = "1"
    me = os.path.join(ROOT, "tests", "test_gpu_voxel_edges.py")
    out = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", me,
                          "-k", "test_entries_match_oracle or test_cube_map_matches_oracle"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "%d passed" % (len(SCENES) + 1) in out.stdout, out.stdout[-500:]
