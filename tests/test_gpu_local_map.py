"""The sliding-window local mapper on the device (lslam_lmap_*, LocalFeatureMap, LaserMappingLocal) against the reference chain
restated with oracle calls and numpy (tests/local_map_ref.py): container contents bit for bit, the eviction rule with its
off-by-one, the two ways of producing the surround held against each other, the "leaf too small" guard, the node's poses, the
composed path a user had before, capacity and misuse."""
import os
import subprocess

import numpy as np
import pytest

from local_map_ref import RefLaserMappingLocal, RefLocalFeatureMap, transform_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_TOL = 1e-4  # the project's bar for a chain's poses (tests/test_gpu_pipeline.py)
REFILTER, KEY_ORDERED, ALWAYS_RESORT = 1, 2, 4  # include/lslam_c.h LSLAM_LMAP_*
MODES = [REFILTER, KEY_ORDERED, ALWAYS_RESORT]
TOO_FEW_REF, NOT_CONVERGED, TOO_FEW_MATCHES = 1, 2, 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def iso(oracle, pose):
    R, t = oracle.pose_to_Rt(np.asarray(pose, np.float32))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    return T


def gt_of(synth, k, x_extra=0.0):
    return (0.0, 0.0, 0.3 + 0.01 * (k % 20), 3.0 + 0.4 * k + x_extra, -2.0 + 0.15 * (k % 20), synth.SENSOR_HEIGHT)


@pytest.fixture(scope="module")
def frames(oracle, synth, small_problem):
    """Downsampled corner / surf features of 14 sweeps of the drive through small_problem's world, with their poses."""
    world = small_problem["world"]
    out = []
    for k in range(14):
        c, s, gtp = synth.make_scan(world, 16, 900, gt_pose=gt_of(synth, k), seed=300 + k)
        out.append((oracle.voxel_grid(c, 1.0), oracle.voxel_grid(s, 1.0), iso(oracle, gtp)))
    return out


def shifted(T, dx):
    T = T.copy()
    T[0, 3] += np.float32(dx)
    return T


def assert_same(lm, ref, where):
    """Everything the container shows against the helper: frames, accum (the exact double), surround (counts and bits)."""
    i = lm.info()
    assert i["n_frames"] == len(ref.queue), (where, i, len(ref.queue))
    assert i["accum_distance"] == ref.accum, (where, i["accum_distance"], ref.accum)
    assert i["frames_evicted"] == ref.evicted, (where, i["frames_evicted"], ref.evicted)
    got = lm.get_frames()
    assert len(got) == len(ref.queue)
    for k, (g, r) in enumerate(zip(got, ref.queue)):
        assert g[2] == r[2], (where, k, g[2], r[2])
        assert g[0].shape == r[0].shape and np.array_equal(bits(g[0]), bits(r[0])), (where, k, "corner")
        assert g[1].shape == r[1].shape and np.array_equal(bits(g[1]), bits(r[1])), (where, k, "surf")
    assert i["n_corner"] == sum(len(f[0]) for f in ref.queue) and i["n_surf"] == sum(len(f[1]) for f in ref.queue)
    gc, gs = lm.get_surround_feature()
    rc, rs = ref.get_surround_feature()
    assert gc.shape == rc.shape and gs.shape == rs.shape, (where, gc.shape, rc.shape, gs.shape, rs.shape)
    assert np.array_equal(bits(gc), bits(rc)), (where, "surround corner")
    assert np.array_equal(bits(gs), bits(rs)), (where, "surround surf")
    return gc, gs


@pytest.mark.parametrize("mode", MODES)
def test_container_parity(pkg, ctx, oracle, frames, mode):
    """Twelve frames at known poses, leaves 0.2 / 0.4, nothing evicted: after every add the device container equals the helper."""
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=mode)
    ref = RefLocalFeatureMap(oracle)
    assert_same(lm, ref, "empty")
    for k in range(12):
        c, s, T = frames[k]
        lm.add_data_frame(c, s, T)
        ref.add_data_frame(c, s, T)
        gc, gs = assert_same(lm, ref, k)
    assert lm.info()["n_frames"] == 12 and len(gc) > 500 and len(gs) > 1500
    merged, resorted, refiltered = lm.stats()
    if mode == REFILTER:
        assert (merged, resorted) == (0, 0) and refiltered == 24
    elif mode == KEY_ORDERED:
        assert merged == 22 and resorted == 2 and refiltered == 0  # the first frame of each type is sorted as a whole
    else:
        assert merged == 0 and resorted == 24
    lm.close()


@pytest.mark.parametrize("mode", MODES)
def test_eviction_short_window(pkg, ctx, oracle, frames, mode):
    """queue_distance 2.0 m over a 0.43 m-per-sweep drive: frames leave on most sweeps, two at a time (the n + 1 rule)."""
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=mode, queue_distance=2.0)
    ref = RefLocalFeatureMap(oracle, queue_distance=2.0)
    sizes = []
    for k in range(14):
        c, s, T = frames[k]
        lm.add_data_frame(c, s, T)
        ref.add_data_frame(c, s, T)
        assert_same(lm, ref, k)
        sizes.append(len(ref.queue))
    assert ref.evicted >= 6 and max(sizes) <= 6
    assert any(a - b == 1 for a, b in zip(sizes, sizes[1:]))  # push one, erase two
    lm.close()


@pytest.mark.parametrize("mode", MODES)
def test_eviction_of_the_whole_queue(pkg, ctx, oracle, frames, mode):
    """A 31 m step: every frame falls behind, the erase of n + 1 takes the new frame with them, the next surround is empty --
    the empty map, on which a match reports TOO_FEW_REF -- and the window fills again from the sweep after."""
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=mode)
    ref = RefLocalFeatureMap(oracle)
    for k in range(5):
        c, s, T = frames[k]
        lm.add_data_frame(c, s, T)
        ref.add_data_frame(c, s, T)
        assert_same(lm, ref, k)
    assert lm.surround_to_map_counts()[0] > 0
    c, s, T = frames[5]
    lm.add_data_frame(c, s, shifted(T, 31.0))
    ref.add_data_frame(c, s, shifted(T, 31.0))
    assert ref.queue == [] and ref.evicted == 6
    assert_same(lm, ref, "after the step")
    assert lm.surround_to_map_counts() == (0, 0)
    status, pose, st = ctx.scanmatch_scan(c, s, np.zeros(6, np.float32))
    assert int(status) == TOO_FEW_REF
    for k in range(6, 9):
        c, s, T = frames[k]
        lm.add_data_frame(c, s, shifted(T, 31.0))
        ref.add_data_frame(c, s, shifted(T, 31.0))
        assert_same(lm, ref, k)
    assert lm.info()["n_frames"] == 3
    lm.close()


def test_modes_agree_on_equal_keys_and_a_widened_extent(pkg, ctx, oracle, frames):
    """The re-filter and the key-ordered window side by side (and the helper beside both) over a sequence with a frame whose
    points repeat an earlier frame's exactly -- equal keys: arrival order must decide the sums -- and a frame with a far
    outlier that widens the extent (another min_b, a wider key), with frames leaving in between."""
    a = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=REFILTER, queue_distance=3.0)
    b = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=KEY_ORDERED, queue_distance=3.0)
    ref = RefLocalFeatureMap(oracle, queue_distance=3.0)
    seq = []
    for k in range(4):
        seq.append(frames[k])
    seq.append(frames[1])                      # the same points at the same pose again
    seq.append(frames[4])
    c, s, T = frames[5]
    c, s = c.copy(), s.copy()
    c[7, :3] = (150.0, -90.0, 40.0)            # far outliers: the window's extent (and min_b) jumps
    s[11, :3] = (-120.0, 170.0, -30.0)
    seq.append((c, s, T))
    seq += [frames[k] for k in range(6, 12)]   # ... and shrinks back when that frame leaves
    seq.append((frames[12][0], np.zeros((0, 4), np.float32), frames[12][2]))  # a frame without surf points
    seq.append(frames[13])
    for n, (c, s, T) in enumerate(seq):
        for m in (a, b):
            m.add_data_frame(c, s, T)
        ref.add_data_frame(c, s, T)
        ac, as_ = assert_same(a, ref, ("refilter", n))
        bc, bs = assert_same(b, ref, ("key-ordered", n))
        assert np.array_equal(bits(ac), bits(bc)) and np.array_equal(bits(as_), bits(bs)), n
    assert ref.evicted > 0
    merged, resorted, refiltered = b.stats()
    assert merged > 20 and refiltered == 0, (merged, resorted, refiltered)
    a.close()
    b.close()


@pytest.mark.parametrize("mode", [REFILTER, KEY_ORDERED])
def test_leaf_too_small_guard(pkg, ctx, oracle, frames, mode):
    """A window 330 m wide on every axis: (330 / 0.2)^3 voxels exceed INT_MAX at the corner leaf, so pcl::VoxelGrid (and
    Oracle.voxel_grid) hands the corner cloud back unfiltered, in input order; the surf leaf 0.4 still filters."""
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=mode)
    ref = RefLocalFeatureMap(oracle)
    far = np.array([[-165.0, -165.0, -165.0, 1.0], [165.0, 165.0, 165.0, 2.0], [165.0, -165.0, 165.0, 3.0], [0.5, 0.25, 0.125, 4.0],
                    [0.5, 0.25, 0.125, 5.0]], np.float32)
    I = np.eye(4, dtype=np.float32)
    for n, (c, s, T) in enumerate((frames[0], (far, far, I), frames[1])):
        lm.add_data_frame(c, s, T)
        ref.add_data_frame(c, s, T)
        gc, gs = assert_same(lm, ref, n)
    cc, cs = ref.concatenated()
    assert len(gc) == len(cc) and np.array_equal(bits(gc), bits(cc))   # unfiltered: the concatenation itself
    assert len(gs) < len(cs)                                           # filtered
    lm.close()


def drifting_drive(oracle, synth, world, ks):
    """(corner, surf, odometry pose) per sweep: ground truth with a small deterministic drift on top."""
    for n, k in enumerate(ks):
        c, s, gtp = synth.make_scan(world, 16, 900, gt_pose=gt_of(synth, k), seed=300 + k)
        odom = (iso(oracle, gtp) @ iso(oracle, [0, 0, 0.002 * n, 0.03 * n, -0.02 * n, 0])).astype(np.float32)
        yield n, c, s, odom


@pytest.mark.parametrize("ks", [tuple(range(8)), (0, 1, 2, 3, 2, 1, 0)], ids=["smooth", "out-and-back"])
@pytest.mark.parametrize("mode", [REFILTER, KEY_ORDERED])
def test_node_parity(pkg, ctx, oracle, synth, small_problem, ks, mode):
    """LaserMappingLocal.process against the helper chain.  Both chains are fed the device's previous pose, so that each sweep's
    stages are compared on identical input: the surround handed to the match bit for bit, the new map pose to CHAIN_TOL.
    Condition (asserted of the HELPER, so that a device that skips matches cannot pass by agreeing with an idle reference):
    on every sweep with a non-empty window the helper's match returns neither TOO_FEW_REF nor TOO_FEW_MATCHES and stops by
    its step threshold before max_iterations (10).  With use_score = 0 a good match's status is NOT_CONVERGED (2)."""
    node = pkg.LaserMappingLocal(ctx, max_points=1 << 17, max_frames=64, mode=mode)
    ref = RefLaserMappingLocal(oracle, ctx)
    worst, matched = 0.0, 0
    for n, c, s, odom in drifting_drive(oracle, synth, small_problem["world"], ks):
        new_ref, cds, sds = ref.match(c, s, odom)
        gc, gs = node.feature_map.get_surround_feature()
        assert np.array_equal(bits(gc), bits(ref.last_surround[0])) and np.array_equal(bits(gs), bits(ref.last_surround[1])), n
        M = node.process(c, s, odom)
        if n == 0:
            assert ref.last_stats is None and len(gc) == 0 and len(gs) == 0
            assert np.array_equal(bits(M), bits(odom))  # nothing to match against: the merged pose stands
        else:
            st = ref.last_stats
            assert st is not None and st.status not in (TOO_FEW_REF, TOO_FEW_MATCHES), (n, st.status)
            assert st.converged == 1 and st.iterations < 10, (n, st.converged, st.iterations)
            assert st.status == NOT_CONVERGED
            assert int(node.last_stats.status) == NOT_CONVERGED and node.last_stats.iterations == st.iterations, n
            matched += 1
        d = float(np.abs(M - new_ref).max())
        print("sweep %d: |device - helper| = %.3g, helper iterations %s" % (n, d, ref.last_stats.iterations if ref.last_stats else "-"))
        assert d <= CHAIN_TOL, (n, d)
        worst = max(worst, d)
        ref.commit(M, cds, sds, odom)
        assert node.feature_map.info()["accum_distance"] == ref.fm.accum
    assert matched == len(ks) - 1
    got = node.feature_map.get_frames()
    assert len(got) == len(ref.fm.queue) == len(ks)
    for g, r in zip(got, ref.fm.queue):
        assert np.array_equal(bits(g[0]), bits(r[0])) and np.array_equal(bits(g[1]), bits(r[1])) and g[2] == r[2]
    print("node worst |device - helper| = %.3g (bar %.0e)" % (worst, CHAIN_TOL))
    node.feature_map.close()


class _DeviceFilters:
    """Oracle.voxel_grid's place in RefLocalFeatureMap, taken by the device's lslam_voxel_grid."""

    def __init__(self, pkg, ctx):
        self.pkg, self.ctx = pkg, ctx

    def voxel_grid(self, cloud, leaf):
        return self.pkg.voxel_grid(self.ctx, cloud, leaf)


class ComposedLocalMapping:
    """What a user could compose from the public pieces before the container existed: frames kept on the host, np.concatenate,
    voxel_grid twice, map_set, scanmatch_scan."""

    def __init__(self, pkg, ctx):
        self.pkg, self.ctx = pkg, ctx
        self.fm = RefLocalFeatureMap(_DeviceFilters(pkg, ctx))
        self.opts = ctx.default_opts()
        self.opts.delta_t_abort = self.opts.delta_r_abort = 0.1
        self.opts.use_score = 0
        self.odom_last = np.eye(4, dtype=np.float32)
        self.mapped_last = np.eye(4, dtype=np.float32)

    def process(self, corner_last, surf_last, odom_new):
        out = np.zeros(16, np.float32)
        import ctypes as C
        fp = lambda x: np.ascontiguousarray(x, np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
        a, b, c = (np.ascontiguousarray(m, np.float32).reshape(16) for m in (self.odom_last, odom_new, self.mapped_last))
        self.ctx.lib.lslam_transform_associate(fp(a), fp(b), fp(c), out.ctypes.data_as(C.POINTER(C.c_float)))
        new = out.reshape(4, 4).copy()
        cds, sds = self.pkg.voxel_grid2(self.ctx, corner_last, surf_last, 1.0)
        mc, ms = self.fm.get_surround_feature()
        self.ctx.map_set(mc, ms)
        if len(mc) or len(ms):
            status, pose, st = self.ctx.scanmatch_scan(cds, sds, self.ctx.isometry_to_pose(new), self.opts)
            if int(status) != TOO_FEW_REF:
                new = self.ctx.pose_to_isometry(pose)
        self.mapped_last, self.odom_last = new.copy(), np.array(odom_new, np.float32)
        self.fm.add_data_frame(cds, sds, new)
        return new


@pytest.mark.parametrize("mode", [REFILTER, KEY_ORDERED])
def test_node_equals_the_composed_path(pkg, ctx, oracle, synth, small_problem, mode):
    """On the smooth drive the node's poses are bit for bit those of the composed path on the same context, deferred trees on
    for both."""
    node = pkg.LaserMappingLocal(ctx, max_points=1 << 17, max_frames=64, mode=mode)   # (switches deferred trees on)
    composed = ComposedLocalMapping(pkg, ctx)
    for n, c, s, odom in drifting_drive(oracle, synth, small_problem["world"], tuple(range(8))):
        M = node.process(c, s, odom)
        Mc = composed.process(c, s, odom)
        assert np.array_equal(bits(M), bits(Mc)), (n, np.abs(M - Mc).max())
    assert node.feature_map.info()["accum_distance"] == composed.fm.accum
    node.feature_map.close()


def test_device_pointer_entry(pkg, ctx, oracle, frames):
    """Frames handed over as device tensors give the container the host entry gives."""
    import torch
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32)
    ref = RefLocalFeatureMap(oracle)
    for k in range(4):
        c, s, T = frames[k]
        dc, ds = torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda()
        torch.cuda.synchronize()
        lm.add_data_frame(dc, ds, T)
        ref.add_data_frame(c, s, T)
        assert_same(lm, ref, k)
    lm.close()


def test_capacity_and_misuse(pkg, ctx, oracle, frames):
    LslamError = pkg.LslamError
    c0, s0, T0 = frames[0]
    # max_frames
    lm = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=3)
    ref = RefLocalFeatureMap(oracle)
    for k in range(3):
        lm.add_data_frame(*frames[k])
        ref.add_data_frame(*frames[k])
    with pytest.raises(LslamError) as e:
        lm.add_data_frame(*frames[3])
    assert e.value.code == pkg.Status.ERR_INVALID and "max_frames" in str(e.value)
    assert_same(lm, ref, "after the refused frame")
    # the filter-size setter is refused after the first frame ...
    with pytest.raises(LslamError) as e:
        lm.setup_filter_size(0.3, 0.5)
    assert "fixed" in str(e.value)
    assert_same(lm, ref, "after the refused setter")
    # ... and clear returns the container to its initial state: accum 0, first-frame rule armed, leaves may be set
    lm.clear()
    ref.clear()
    assert_same(lm, ref, "cleared")
    assert lm.info() == dict(n_frames=0, accum_distance=0.0, n_corner=0, n_surf=0, frames_evicted=0)
    assert lm.surround_to_map_counts() == (0, 0)
    lm.setup_filter_size(0.3, 0.5)
    ref = RefLocalFeatureMap(oracle, leaf_corner=np.float32(0.3), leaf_surf=0.5)
    for k in (4, 5):
        lm.add_data_frame(*frames[k])
        ref.add_data_frame(*frames[k])
        assert_same(lm, ref, ("other leaves", k))
    assert lm.info()["accum_distance"] == ref.accum > 0.3  # the first frame after clear() did not add its distance from frame 2
    lm.close()
    # max_points
    lm = pkg.LocalFeatureMap(ctx, max_points=len(s0) + 10, max_frames=8)
    ref = RefLocalFeatureMap(oracle)
    lm.add_data_frame(c0, s0, T0)
    ref.add_data_frame(c0, s0, T0)
    with pytest.raises(LslamError) as e:
        lm.add_data_frame(*frames[1])
    assert "max_points_per_type" in str(e.value) and "surf" in str(e.value)
    assert_same(lm, ref, "after the refused points")
    # bad arguments
    with pytest.raises(LslamError):
        lm.setup_queue_distance(0.0)
    import ctypes as C
    T = np.eye(4, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    assert lm.lib.lslam_lmap_add_data_frame(lm.h, None, 5, None, 0, 16, T.ctypes.data_as(fp)) == pkg.Status.ERR_INVALID
    assert lm.lib.lslam_lmap_add_data_frame(lm.h, c0.ctypes.data_as(C.c_void_p), 5, None, 0, 12, T.ctypes.data_as(fp)) == pkg.Status.ERR_INVALID
    assert_same(lm, ref, "after bad arguments")
    lm.close()
    h = C.c_void_p()
    assert ctx.lib.lslam_lmap_create(ctx.h, 0, 0, REFILTER | KEY_ORDERED, C.byref(h)) == pkg.Status.ERR_INVALID
    assert ctx.lib.lslam_lmap_create(ctx.h, (1 << 24) + 1, 0, 0, C.byref(h)) == pkg.Status.ERR_INVALID


def test_ordered_array_full_of_evicted_entries(pkg, ctx, oracle, frames):
    """Adds without a surround in between: the key-ordered array fills with entries of frames that have left (they are only
    compacted at a surround), cannot take the next frame, and is rebuilt from the ring at the next surround -- same bits."""
    n_surf = max(len(f[1]) for f in frames)
    lm = pkg.LocalFeatureMap(ctx, max_points=3 * n_surf + 100, max_frames=8, mode=KEY_ORDERED, queue_distance=1.0)
    ref = RefLocalFeatureMap(oracle, queue_distance=1.0)
    lm.add_data_frame(*frames[0])
    ref.add_data_frame(*frames[0])
    assert_same(lm, ref, 0)
    for k in range(1, 8):
        lm.add_data_frame(*frames[k])
        ref.add_data_frame(*frames[k])
    assert len(ref.queue) == 2 and ref.evicted == 6  # the window never emptied: frames left two at a time
    assert_same(lm, ref, "after seven adds")
    merged, resorted, refiltered = lm.stats()
    # the first frame of each type was sorted as a whole.  The surf array overflowed at the fourth frame and was rebuilt from
    # the ring; the corner array (a few hundred points per frame) had room all along, but its ordered prefix -- frame 0 -- had
    # left, so after the compaction everything in it was new: a sort of everything as well
    assert (merged, resorted, refiltered) == (0, 4, 0)
    lm.add_data_frame(*frames[8])
    ref.add_data_frame(*frames[8])
    assert_same(lm, ref, "merging again")
    assert lm.stats() == (2, 4, 0)
    lm.close()


def test_two_containers_on_two_contexts(pkg, ctx, oracle, frames):
    """Interleaved adds on two contexts: each container equals its own helper."""
    ctx2 = pkg.Context(0)
    a = pkg.LocalFeatureMap(ctx, max_points=1 << 16, max_frames=32, mode=KEY_ORDERED, queue_distance=2.0)
    b = pkg.LocalFeatureMap(ctx2, max_points=1 << 16, max_frames=32, mode=KEY_ORDERED)
    ra, rb = RefLocalFeatureMap(oracle, queue_distance=2.0), RefLocalFeatureMap(oracle)
    for k in range(8):
        a.add_data_frame(*frames[k])
        b.add_data_frame(*frames[13 - k])
        ra.add_data_frame(*frames[k])
        rb.add_data_frame(*frames[13 - k])
        assert_same(a, ra, ("a", k))
        assert_same(b, rb, ("b", k))
    a.close()
    b.close()
    ctx2.close()


def test_destroy_releases_device_memory(pkg, ctx, frames):
    """Create, use and destroy twenty times: the device's free memory is back within the size of one container (scratch that
    is not released with its container would add up)."""
    import torch

    def cycle():
        lm = pkg.LocalFeatureMap(ctx, max_points=1 << 20, max_frames=64, mode=KEY_ORDERED, queue_distance=1.0)
        for k in range(4):
            lm.add_data_frame(*frames[k])
            lm.surround_to_map_counts()
        used = free0 - torch.cuda.mem_get_info()[0]
        lm.close()
        return used
    free0 = torch.cuda.mem_get_info()[0]
    cycle()  # (what the context keeps -- its filter scratch grows with the first container -- is taken here)
    free0 = torch.cuda.mem_get_info()[0]
    one = cycle()
    assert one > (1 << 20) * 16 * 4  # a container of 2^20 points per type is hundreds of megabytes
    for _ in range(20):
        cycle()
    lost = free0 - torch.cuda.mem_get_info()[0]
    print("one container %.1f MiB, lost after 20 cycles %.1f MiB" % (one / 2 ** 20, lost / 2 ** 20))
    assert lost < one


def test_cpp_mirror_equals_python_node(pkg, oracle, synth, small_problem, tmp_path):
    """include/lslam_pipeline.hpp's LaserMappingLocal driven from C++ gives the Python node's poses (same ABI calls: same bits)."""
    sweeps = list(drifting_drive(oracle, synth, small_problem["world"], tuple(range(6))))
    path = tmp_path / "local_sweeps.bin"
    with open(path, "wb") as fo:
        for n, c, s, odom in sweeps:
            for a in (c, s):
                a = np.ascontiguousarray(a, np.float32)
                fo.write(np.uint32(len(a)).tobytes())
                fo.write(a.tobytes())
            fo.write(np.ascontiguousarray(odom, np.float32).tobytes())
    ctx = pkg.Context(0)
    node = pkg.LaserMappingLocal(ctx, max_points=1 << 18, max_frames=64)
    ref = []
    for n, c, s, odom in sweeps:
        M = node.process(c, s, odom)
        gc, gs = node.feature_map.get_surround_feature()
        ref.append((M, len(gc), len(gs)))
    node.feature_map.close()
    ctx.close()
    exe = tmp_path / "local_mapping_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "local_mapping_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [l.split() for l in out.stdout.splitlines() if l.startswith("POSE ")]
    assert len(got) == len(ref) == 6
    for w, (M, nc, ns) in zip(got, ref):
        v = np.array([float.fromhex(x) for x in w[2:14]], np.float32).reshape(3, 4)
        assert np.array_equal(bits(v), bits(M[:3])), w[1]
        assert (int(w[14]), int(w[15])) == (nc, ns)
