"""The registration node for organised clouds resident on the device (include/lslam_c.h lslam_oreg_*; csrc/lslam_features.hip)
held, BIT FOR BIT, against the CPU restatement (tests/organised_registration_ref.py: cloud and ranges) and against the
oracle-pinned extraction on the restatement's cloud and ranges (the four lists).  Nothing in this node is approximate: every
comparison is of uint32 views, but for the two /imu_trans rows that are a rotated zero vector (0 and -0 are both right)."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import organised_registration_ref as O

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000 * 10 ** 9
TILE = 1024  # OR_TILE, csrc/lslam_features.hip: cells per workgroup (256 threads)
_SCANS = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scan(synth, world, rings, steps, k=0):
    """The organised image of one synthetic sweep (made once per shape and pose, shared, never written)."""
    key = (rings, steps, k)
    if key not in _SCANS:
        gt = (0.0, 0.0, 0.3 + 0.01 * k, 3.0 + 0.4 * k, -2.0 + 0.15 * k, synth.SENSOR_HEIGHT)
        cloud = synth.make_scan(world, rings, steps, gt_pose=gt, seed=300 + k, full=True)[3]
        xyz, ring = O.image_from_scan(cloud, rings, steps)
        xyz.setflags(write=False)
        ring.setflags(write=False)
        _SCANS[key] = (xyz, ring)
    return _SCANS[key]


def _want(pkg, ctx, xyz, ring, params=None, **kw):
    """The restatement's cloud and ranges, and the pinned extraction's lists on them."""
    sr = pkg.scan_registration
    out = O.process(xyz, ring, **kw)
    lists = {k: np.zeros((0, 4), np.float32) for k in sr.LISTS}
    if len(out["cloud"]):  # (the extraction entry point refuses the {0, 0} range of an empty cloud; the node gives empty lists)
        fs = sr.FeatureSet(ctx)
        sr.extract_features_dev(ctx, out["cloud"], out["ranges"], fs, params=params)
        lists = {k: fs.download(k) for k in sr.LISTS}
        fs.close()
    out["lists"] = lists
    return out


def _assert_node(pkg, ctx, node, xyz, ring, params=None, form="packed", stamp=T0, tag="", **kw):
    sr = pkg.scan_registration
    want = _want(pkg, ctx, xyz, ring, params, **kw)
    fs = sr.FeatureSet(ctx)
    if form == "packed":
        got = node.process(xyz, stamp, fs, ring=ring)
    else:
        got = node.process(O.as_point_xyzit(xyz, ring, fill=0xAB), stamp, fs)
    assert got == fs.counts() == {k: len(want["lists"][k]) for k in sr.LISTS}, tag
    for k in sr.LISTS:
        assert np.array_equal(bits(fs.download(k)), bits(want["lists"][k])), (tag, k)
    cloud, ranges = node.cloud()
    assert cloud.shape == want["cloud"].shape and np.array_equal(bits(cloud), bits(want["cloud"])), tag
    assert np.array_equal(ranges, want["ranges"]), tag
    st = node.last_stats
    assert st.n_points == len(want["cloud"]) and st.n_cells == ring.size and st.launches == 6, tag
    fs.close()
    return got, want


@pytest.mark.parametrize("rings,steps", [(16, 900), (64, 1800)])
def test_node_equals_the_restatement_and_the_pinned_extraction(pkg, ctx, synth, small_problem, rings, steps):
    node = pkg.OrganisedScanRegistration(ctx)
    xyz, ring = _scan(synth, small_problem["world"], rings, steps)
    counts, want = _assert_node(pkg, ctx, node, xyz, ring)
    assert min(counts.values()) > 0 and 0 < len(want["cloud"]) < ring.size and np.all(node.imu_trans == 0)
    assert node.last_stats.sweeps == 1 and node.last_stats.imu_states == 0
    up = 128 + 16 * ((2 * rings * 4 + 15) // 16) + 16 * ((rings * 4 + 15) // 16) + 16 * ((steps * 4 + 15) // 16) + 16 * rings * steps
    assert node.last_stats.bytes_up == up and node.last_stats.bytes_down == (32 + 2 * rings) * 4
    if rings == 16:  # a second sweep through the warm node, as the reference's 32-byte points
        xyz2, ring2 = _scan(synth, small_problem["world"], rings, steps, k=1)
        _assert_node(pkg, ctx, node, xyz2, ring2, form="xyzit")
        assert node.last_stats.sweeps == 2
    node.close()


def test_non_default_parameters(pkg, ctx, synth, small_problem):
    sr = pkg.scan_registration
    xyz, ring = _scan(synth, small_problem["world"], 16, 900)
    p = sr.default_params(ctx)
    p.n_feature_regions, p.curvature_region, p.max_corner_sharp, p.max_surface_flat = 4, 4, 3, 5
    p.less_flat_filter_size, p.surface_curvature_threshold = 0.3, 0.05
    node = pkg.OrganisedScanRegistration(ctx, scan_period=0.05, blind_radius=6.0, params=p)
    counts, want = _assert_node(pkg, ctx, node, xyz, ring, params=p, scan_period=0.05, blind_radius=6.0)
    base = O.process(xyz, ring)
    assert min(counts.values()) > 0 and len(want["cloud"]) < len(base["cloud"])  # the wider blind radius drops points
    node.close()


def test_the_ring_is_the_points_field_not_the_row(pkg, ctx, synth, small_problem):
    xyz, ring = _scan(synth, small_problem["world"], 16, 900)
    node = pkg.OrganisedScanRegistration(ctx)
    for table in (ring[::-1], ring + np.uint16(1000)):
        _, want = _assert_node(pkg, ctx, node, xyz, np.ascontiguousarray(table))
        rows = np.repeat(np.arange(16), want["keep"].sum(1))
        assert np.any(np.floor(want["cloud"][:, 3]).astype(int) != rows)  # a kernel that wrote the row would differ
    node.close()


def _points(h, w, keep, seed=0):
    """An image whose cells are valid where `keep` (distinct points 5 m or more away) and NaN / inf / too near elsewhere."""
    rng = np.random.default_rng(seed)
    xyz = (5.0 + rng.uniform(0, 30, (h, w, 3))).astype(np.float32)
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [0.5, 0.5, 0.5], [0, 0, 0]], np.float32)
    xyz[~keep] = bad[rng.integers(0, len(bad), (~keep).sum())]
    ring = rng.integers(0, 2000, (h, 1)).astype(np.uint16).repeat(w, 1)
    return xyz, ring


PATTERNS = {
    "all": lambda n: np.ones(n, bool),
    "none": lambda n: np.zeros(n, bool),
    "alternating": lambda n: np.arange(n) % 2 == 0,
    "last": lambda n: np.arange(n) == n - 1,
    "first": lambda n: np.arange(n) == 0,
}


def test_compaction_corners_small(pkg, ctx):
    """Tiles that span rows, rows that end inside a wavefront, a ragged last tile: widths 1, 63, 64, 65 and 100 (no divisor of
    the tile) with 3 to 5 rows, under every validity pattern."""
    node = pkg.OrganisedScanRegistration(ctx)
    for k, w in enumerate((1, 63, 64, 65, 100)):
        h = 3 + k % 3
        assert TILE % w or w in (1, 64)
        for name, pattern in PATTERNS.items():
            keep = pattern(h * w).reshape(h, w)
            xyz, ring = _points(h, w, keep, seed=k)
            _, want = _assert_node(pkg, ctx, node, xyz, ring, tag="%d x %d %s" % (h, w, name))
            assert np.array_equal(want["keep"], keep)
    node.close()


def test_compaction_rows_and_tiles(pkg, ctx):
    node = pkg.OrganisedScanRegistration(ctx)
    rng = np.random.default_rng(5)
    # one row longer than a tile (and a tile boundary inside every row)
    keep = rng.random((3, 1500)) < 0.6
    _assert_node(pkg, ctx, node, *_points(3, 1500, keep, 1), tag="3 x 1500")
    # 20 rows of 100 in two tiles (the second ragged), each tile spanning many rows
    keep = rng.random((20, 100)) < 0.5
    _assert_node(pkg, ctx, node, *_points(20, 100, keep, 2), tag="20 x 100")
    # empty rows at the front, in the middle and at the end: {0, 0} / {size, size - 1}
    keep = rng.random((7, 70)) < 0.7
    keep[[0, 1, 3, 6]] = False
    _, want = _assert_node(pkg, ctx, node, *_points(7, 70, keep, 3), tag="empty rows")
    r = want["ranges"]
    assert r[0].tolist() == [0, 0] and r[1].tolist() == [0, 0] and r[3, 0] == r[3, 1] + 1 and r[6].tolist() == [len(want["cloud"]), len(want["cloud"]) - 1]
    # a sweep that keeps nothing succeeds with empty lists
    counts, want = _assert_node(pkg, ctx, node, *_points(4, 300, np.zeros((4, 300), bool), 4), tag="nothing kept")
    assert set(counts.values()) == {0} and want["ranges"].tolist() == [[0, 0]] * 4 and node.cloud()[0].shape == (0, 4)
    node.close()


def test_more_tiles_than_a_workgroup_has_threads(pkg, ctx):
    """128 x 2560 cells, mostly NaN: 320 tiles, so the sum of the tiles before a workgroup's own takes two trips of its 256
    threads; kept cells in every part of the image, some tiles empty."""
    h, w = 128, 2560
    assert h * w // TILE > 256
    rng = np.random.default_rng(6)
    keep = rng.random((h, w)) < 0.03
    keep[:, 700:900] |= rng.random((h, 200)) < 0.5
    keep[40:44] = False
    keep[127, -1] = True
    node = pkg.OrganisedScanRegistration(ctx)
    _, want = _assert_node(pkg, ctx, node, *_points(h, w, keep, 7), tag="128 x 2560")
    assert 10000 < len(want["cloud"]) < h * w // 10
    node.close()


def test_the_extractions_row_limit(pkg, ctx):
    sr = pkg.scan_registration
    node = pkg.OrganisedScanRegistration(ctx)
    fs = sr.FeatureSet(ctx)
    rng = np.random.default_rng(8)
    # width 3000 with at most 2560 kept per row: fine
    keep = rng.random((3, 3000)) < 0.5
    assert keep.sum(1).max() <= 2560
    _assert_node(pkg, ctx, node, *_points(3, 3000, keep, 1), tag="3 x 3000")
    # a row that keeps exactly 2560 passes
    keep = np.zeros((3, 2600), bool)
    keep[0, ::3] = True
    keep[1, 17:17 + 2560] = True
    keep[2, -5:] = True
    assert keep[1].sum() == 2560
    xyz, ring = _points(3, 2600, keep, 2)
    _, want = _assert_node(pkg, ctx, node, xyz, ring, tag="2560 in a row")
    # 2561: refused behind the wait, nothing to hand out; the next sweep succeeds
    keep[1, 16] = True
    xyz1, ring1 = _points(3, 2600, keep, 2)
    with pytest.raises(pkg.LslamError, match="lslam_oreg_process.*2560"):
        node.process(xyz1, T0, fs, ring=ring1)
    assert fs.counts() == dict.fromkeys(sr.LISTS, 0)
    with pytest.raises(pkg.LslamError, match="lslam_oreg_cloud"):
        node.cloud()
    _assert_node(pkg, ctx, node, xyz, ring, tag="after the refusal")
    fs.close()
    node.close()


def test_both_input_forms_give_the_same_bits(pkg, ctx, synth, small_problem):
    sr = pkg.scan_registration
    xyz, ring = _scan(synth, small_problem["world"], 16, 900)
    node = pkg.OrganisedScanRegistration(ctx)
    fs = sr.FeatureSet(ctx)
    results = []
    packed = sr.pack_organised(xyz, ring)
    dirty = packed.copy()
    dirty.view(np.uint32)[..., 3] |= np.uint32(0xBEEF0000)  # garbage in the upper half of the fourth word
    forms = [lambda: node.process(xyz, T0, fs, ring=ring), lambda: node.process(packed, T0, fs), lambda: node.process(dirty, T0, fs),
             lambda: node.process(O.as_point_xyzit(xyz, ring, fill=0), T0, fs),
             lambda: node.process(O.as_point_xyzit(xyz, ring, fill=0xFF), T0, fs)]
    for call in forms:
        counts = call()
        cloud, ranges = node.cloud()
        results.append((counts, cloud, ranges, [fs.download(k) for k in sr.LISTS]))
    assert results[0][1].shape[0] > 0 and np.array_equal(bits(results[0][1]), bits(O.process(xyz, ring)["cloud"]))
    for other in results[1:]:
        assert other[0] == results[0][0] and np.array_equal(bits(other[1]), bits(results[0][1])) and np.array_equal(other[2], results[0][2])
        for a, b in zip(other[3], results[0][3]):
            assert np.array_equal(bits(a), bits(b))
    fs.close()
    node.close()


def test_refusals_leave_the_node_as_before(pkg, ctx, synth, small_problem):
    sr = pkg.scan_registration
    capi = __import__("importlib").import_module("the-cooper-mapper_amd.capi")
    lib = ctx.lib
    xyz, ring = _scan(synth, small_problem["world"], 16, 900)
    node = pkg.OrganisedScanRegistration(ctx)
    fs = sr.FeatureSet(ctx)
    with pytest.raises(pkg.LslamError, match="lslam_oreg_cloud"):
        node.cloud()  # nothing registered yet
    good = node.process(xyz, T0, fs, ring=ring)
    cloud0, ranges0 = node.cloud()
    sweeps = node.last_stats.sweeps
    cells = sr.pack_organised(xyz, ring)
    p = cells.ctypes.data_as(C.c_void_p)
    bad = dict(null_cloud=(None, 16, 900, 16, 12), no_rows=(p, 0, 900, 16, 12), no_columns=(p, 16, 0, 16, 12),
               too_many_rows=(p, 4097, 1, 16, 12), too_many_cells=(p, 4096, 262144, 16, 12), short_stride=(p, 16, 900, 8, 2),
               odd_stride=(p, 16, 900, 14, 12), ring_outside=(p, 16, 900, 16, 15))
    for name, (ptr, h, w, stride, off) in bad.items():
        fs2 = sr.FeatureSet(ctx)
        sr.extract_features_dev(ctx, cloud0, ranges0, fs2)
        assert min(fs2.counts().values()) > 0
        counts = (C.c_size_t * 4)(7, 7, 7, 7)
        trans = np.full(12, 7.0, np.float32)
        stats = capi.LslamOregStats()
        stats.sweeps = 7
        rc = lib.lslam_oreg_process(node.h, ptr, h, w, stride, off, T0, fs2.h, counts, trans.ctypes.data_as(capi.c_float_p), C.byref(stats))
        assert rc == pkg.Status.ERR_INVALID and lib.lslam_last_error().decode().startswith("lslam_oreg_process:"), name
        assert list(counts) == [0] * 4 and np.all(trans == 0) and stats.sweeps == 0, name
        assert fs2.counts() == dict.fromkeys(sr.LISTS, 0), name  # out reads empty
        fs2.close()
    # no feature set
    rc = lib.lslam_oreg_process(node.h, p, 16, 900, 16, 12, T0, None, None, None, None)
    assert rc == pkg.Status.ERR_INVALID and lib.lslam_last_error().decode().startswith("lslam_oreg_process:")
    # a stamp that goes back (or stays) is refused, and the history is as it was
    node.handle_imu_message(T0, (0, 0, 0.1), (0, 0, 9.81))
    for stamp in (T0, T0 - 1):
        with pytest.raises(pkg.LslamError, match="lslam_oreg_imu_push"):
            node.handle_imu_message(stamp, (0, 0, 0), (0, 0, 9.81))
    assert node.imu_info()[0] == 1
    node.imu_clear()
    assert not node.has_imu_data()
    # the node is exactly as before: the last sweep's cloud included, and the next sweep is the same sweep
    cloud1, ranges1 = node.cloud()
    assert np.array_equal(bits(cloud1), bits(cloud0)) and np.array_equal(ranges1, ranges0)
    assert node.process(xyz, T0, fs, ring=ring) == good and node.last_stats.sweeps == sweeps + 1
    # bad constructor arguments
    for kw in (dict(scan_period=0.0), dict(blind_radius=-1.0), dict(blind_radius=float("nan")), dict(blind_radius=float("inf")),
               dict(imu_history_size=0), dict(imu_history_size=513)):
        with pytest.raises(pkg.LslamError, match="lslam_oreg_create"):
            pkg.OrganisedScanRegistration(ctx, **kw)
    fs.close()
    node.close()


def _motion(t):
    roll = 0.05 * math.sin(2 * math.pi * 3.0 * t)
    pitch = 0.04 * math.cos(2 * math.pi * 2.0 * t)
    yaw = 0.4 + 0.8 * t + 0.05 * math.sin(2 * math.pi * 2.0 * t)
    la = (2.5 - math.sin(pitch) * 9.81, 0.7 + math.sin(roll) * math.cos(pitch) * 9.81, math.cos(roll) * math.cos(pitch) * 9.81)
    return roll, pitch, yaw, la


@pytest.mark.parametrize("span", [(-0.05, 0.16), (-0.4, -0.2)])
def test_an_imu_changes_imu_trans_only(pkg, ctx, synth, small_problem, span):
    from test_gpu_odom import _raw as sweep
    sr = pkg.scan_registration
    xyz, ring = _scan(synth, small_problem["world"], 16, 900)
    node, multi, ref = pkg.OrganisedScanRegistration(ctx), pkg.MultiScanRegistration(ctx), O.Registration()
    fs = sr.FeatureSet(ctx)
    plain = node.process(xyz, T0, fs, ring=ring)
    cloud0, ranges0 = node.cloud()
    lists0 = [fs.download(k) for k in sr.LISTS]
    hz = 100
    for k in range(int(math.floor(span[0] * hz)), int(math.ceil(span[1] * hz)) + 1):
        roll, pitch, yaw, la = _motion(k / hz)
        stamp = T0 + k * (10 ** 9 // hz)
        node.handle_imu_message(stamp, (roll, pitch, yaw), la)
        multi.handle_imu_message(stamp, (roll, pitch, yaw), la)
        ref.history.push(stamp, roll, pitch, yaw, la)
    assert node.imu_info()[0] == len(ref.history) == multi.imu_info()[0]
    assert np.array_equal(node.imu_info()[1], multi.imu_info()[1]) and np.array_equal(node.imu_info()[2], multi.imu_info()[2])
    # no de-skew: cloud, ranges and lists are the bits they were without an IMU
    assert node.process(xyz, T0, fs, ring=ring) == plain and node.last_stats.imu_states == len(ref.history)
    cloud, ranges = node.cloud()
    assert np.array_equal(bits(cloud), bits(cloud0)) and np.array_equal(ranges, ranges0)
    for k, a in zip(sr.LISTS, lists0):
        assert np.array_equal(bits(fs.download(k)), bits(a)), k
    # /imu_trans: the start state as the multi-scan node reports it, nothing of the sweep, the rotated -start.velocity
    multi.process(sweep(synth, small_problem["world"], 0), T0, fs)
    want = ref.process(xyz, ring, T0)["imu_trans"]
    t = node.imu_trans
    assert np.array_equal(bits(t[0]), bits(multi.imu_trans[0])) and np.array_equal(bits(t[0]), bits(want[0])) and np.any(t[0] != 0)
    assert np.all(t[1] == 0) and np.all(t[2] == 0)  # as numbers: a rotated zero vector may come out as -0
    assert np.array_equal(bits(t[3]), bits(want[3])) and np.linalg.norm(t[3]) > 1e-3
    for o in (node, multi, fs):
        o.close()


def test_chain_into_the_odometry_node(pkg, ctx, synth, small_problem):
    """Three sweeps through OrganisedScanRegistration.handle_cloud_message -> DeviceLaserOdometry.process: the transforms of the
    composed path (restatement -> lslam_extract_features_dev -> the same odometry), bit for bit."""
    sr = pkg.scan_registration
    node = pkg.OrganisedScanRegistration(ctx)
    od_a, od_b = pkg.DeviceLaserOdometry(ctx), pkg.DeviceLaserOdometry(ctx)
    fa, fb = sr.FeatureSet(ctx), sr.FeatureSet(ctx)
    matched = 0
    for k in range(5):  # SYSTEM_DELAY drops the first two clouds of a session: three sweeps are compared
        xyz, ring = _scan(synth, small_problem["world"], 16, 900, k)
        got = node.handle_cloud_message(xyz, T0 + k * 100_000_000, fa, ring=ring)
        assert (got is None) == (k < 2)
        if k < 2:
            continue
        want = O.process(xyz, ring)
        sr.extract_features_dev(ctx, want["cloud"], want["ranges"], fb)
        assert fa.counts() == fb.counts() == got
        T_a, T_b = od_a.process(fa), od_b.process(fb)
        assert (T_a is None) == (T_b is None) == (k == 2)
        if T_a is not None:
            matched += 1
            assert np.array_equal(bits(T_a), bits(T_b)) and np.array_equal(bits(od_a.transform), bits(od_b.transform))
            assert np.any(od_a.transform != 0)
        assert np.array_equal(bits(od_a.last_corner), bits(od_b.last_corner)) and np.array_equal(bits(od_a.last_surf), bits(od_b.last_surf))
    assert matched == 2 and node.cloud_receive_count == 5 and node.last_stats.sweeps == 3
    for o in (od_a, od_b, fa, fb, node):
        o.close()


def test_cpp_organised_registration_equals_the_python_mirror(pkg, synth, small_problem, tmp_path):
    """tests/cpp/organised_registration_end_to_end.cpp (OrganisedScanRegistration -> LaserOdometry::processFeatureSet in C++) on
    four sweeps, the first two without an IMU: the same ABI calls as the Python mirrors, so the same counts, /imu_trans,
    _transform and registered-cloud bits."""
    sr = pkg.scan_registration
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "organised_registration_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "organised_registration_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    ctx = pkg.Context(0)
    node, odo, fs = pkg.OrganisedScanRegistration(ctx), pkg.DeviceLaserOdometry(ctx), sr.FeatureSet(ctx)
    want = []
    with open(tmp_path / "session.bin", "wb") as fo:
        for k in range(4):
            t0 = T0 + k * 100_000_000
            if k >= 2:
                for j in range(10):
                    roll, pitch, yaw, la = _motion(0.1 * k + 0.01 * j)
                    node.handle_imu_message(t0 + j * 10_000_000 - 50_000_000, (roll, pitch, yaw), la)
                    fo.write(struct.pack("<Iq6d", 1, t0 + j * 10_000_000 - 50_000_000, roll, pitch, yaw, *la))
            xyz, ring = _scan(synth, small_problem["world"], 16, 900, k)
            rec = O.as_point_xyzit(xyz, ring, fill=0x5A)
            fo.write(struct.pack("<IqII", 2, t0, 16, 900))
            fo.write(rec.tobytes())
            counts = node.process(rec, t0, fs)
            T = odo.process(fs)
            cloud, ranges = node.cloud()
            fnv = 1469598103934665603  # the C++ program's checksum of laserCloud(): FNV-1a over the cloud's words, then the ranges
            for word in np.concatenate([bits(cloud).reshape(-1), ranges.reshape(-1).view(np.uint32)]).tolist():
                fnv = ((fnv ^ word) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
            want.append((int(node.has_imu_data()), int(T is not None), list(counts.values()), node.imu_trans.reshape(-1).copy(), odo.transform.copy(),
                         [len(cloud), len(ranges), fnv]))
    for o in (node, odo, fs, ctx):
        o.close()
    out = subprocess.run([str(exe), str(tmp_path / "session.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("SWEEP ")]
    assert len(lines) == 4 and "OK sweeps 4" in out.stdout
    for k, (w, (imu, matched, counts, trans, tf, registered)) in enumerate(zip(lines, want)):
        assert [int(v) for v in w[1:8]] == [k, imu, matched] + counts, k
        got = np.array([float.fromhex(v) for v in w[8:26]], np.float32)
        assert [int(w[26]), int(w[27]), int(w[28], 16)] == registered, k  # laserCloud(cloud, &ranges) = cloud() of the Python mirror
        assert np.array_equal(bits(got[:12]), bits(trans)) and np.array_equal(bits(got[12:]), bits(tf)), k
    assert want[1][0] == 0 and want[2][0] == 1 and np.any(want[3][3] != 0) and min(want[0][2]) > 0


def test_nodes_give_their_memory_back(pkg, synth, small_problem):
    """Twenty nodes made, used once and destroyed on contexts that are destroyed: no device memory stays behind beyond what one
    used context with its node holds (the method of tests/test_gpu_scan_registration.py, its settling round included)."""
    import torch
    sr = pkg.scan_registration
    xyz, ring = _scan(synth, small_problem["world"], 64, 1800)

    def free():
        return torch.cuda.mem_get_info()[0]

    def use(c):
        node = pkg.OrganisedScanRegistration(c)
        node.handle_imu_message(T0, (0.0, 0.0, 0.1), (0.0, 0.0, 9.81))
        fs = sr.FeatureSet(c)
        counts = node.process(xyz, T0, fs, ring=ring)
        assert min(counts.values()) > 0
        return node, fs

    def eight_alive():
        ctxs = [pkg.Context(0) for _ in range(8)]
        made = [use(c) for c in ctxs]
        held = free()
        for (node, fs), c in zip(made, ctxs):
            node.close()
            fs.close()
            c.close()
        return held
    eight_alive()  # the runtime's per-queue state
    c = pkg.Context(0)
    for o in use(c):
        o.close()
    c.close()
    free0 = free()
    c = pkg.Context(0)
    node, fs = use(c)
    one = free0 - free()
    node.close()
    fs.close()
    c.close()
    for _ in range(20):
        c = pkg.Context(0)
        node, fs = use(c)
        node.close()
        fs.close()
        c.close()
    lost = free0 - free()
    print("one used context and node %.1f MiB, lost after twenty cycles %.1f MiB" % (one / 2 ** 20, lost / 2 ** 20))
    # a 115 200-cell sweep: the extraction's five point arrays alone are 5 x 16 B x 115 200 = 8.8 MiB, the lists' slices 7 MiB
    assert one > 8 << 20
    assert lost < one
