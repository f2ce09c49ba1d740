"""The registration node resident on the device (include/lslam_c.h lslam_sreg_*; csrc/lslam_features.hip): without an IMU
held, bit for bit, against the composed path (lslam_multiscan_register + lslam_extract_features_dev); the IMU branch held
against tests/scan_registration_ref.py to a rounding bound, with the extraction on the de-skewed cloud held bit for bit
against the oracle-pinned entry point -- so no feature label can flip inside the tolerance."""
import math

import numpy as np
import pytest

import scan_registration_ref as R

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000 * 10 ** 9
EPS = 2.0 ** -24
# the largest difference between the device's and the restatement's sin / cos of the same float angle: both round a double
# evaluation to float (half a float ulp each, <= 2^-25 for values below 1, plus the double's own error); states used as they
# are carry glibc's sinf / cosf on the device side, one ulp (2^-24) from the correctly rounded value at most
E_T = 2.0 ** -23
MAPPERS = {16: (-15.0, 15.0), 32: (-15.0, 15.0), 64: (-24.9, 2.0)}  # the ring tables synth.ring_elevations casts its rays with


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw(synth, rings, steps, seed=8):
    from test_oracle_features import _raw_sweep
    return _raw_sweep(synth, rings=rings, steps=steps, seed=seed)[0]


def _composed(pkg, ctx, raw, rings, params=None):
    sr = pkg.scan_registration
    lo, hi = MAPPERS[rings]
    reg, rr = sr.multiscan_register(ctx, raw, lo, hi, rings)
    fs = sr.FeatureSet(ctx)
    counts = sr.extract_features_dev(ctx, reg, rr, fs, params=params)
    lists = {k: fs.download(k) for k in sr.LISTS}
    fs.close()
    return reg, rr, counts, lists


def _node(pkg, ctx, rings, **kw):
    lo, hi = MAPPERS[rings]
    return pkg.MultiScanRegistration(ctx, lo, hi, rings, **kw)


def _assert_equals_composed(pkg, ctx, node, raw, rings, params=None, stamp=T0):
    sr = pkg.scan_registration
    reg, rr, counts, lists = _composed(pkg, ctx, raw[:, :4] if raw.shape[1] > 4 else raw, rings, params)
    fs = sr.FeatureSet(ctx)
    got = node.process(raw, stamp, fs)
    assert got == counts == fs.counts()
    for k in sr.LISTS:
        assert np.array_equal(bits(fs.download(k)), bits(lists[k])), k
    cloud, ranges = node.cloud()
    assert np.array_equal(bits(cloud), bits(reg)) and np.array_equal(ranges, rr)
    assert node.last_stats.n_points == len(reg) and node.last_stats.imu_states == 0
    assert np.all(node.imu_trans == 0)
    fs.close()
    return counts


@pytest.mark.parametrize("rings,steps", [(16, 1800), (64, 1800), (32, 2400)])
def test_no_imu_is_the_composed_path_bit_for_bit(pkg, ctx, synth, rings, steps):
    raw = _raw(synth, rings, steps)
    node = _node(pkg, ctx, rings)
    counts = _assert_equals_composed(pkg, ctx, node, raw, rings)
    assert min(counts.values()) > 0
    # a second sweep through the same node (its buffers are warm), stride 32
    raw2 = _raw(synth, rings, steps, seed=9)
    wide = np.concatenate([raw2, np.full((len(raw2), 4), 7.0, np.float32)], 1)
    assert wide.shape[1] * 4 == 32
    _assert_equals_composed(pkg, ctx, node, wide, rings)
    node.close()


def test_no_imu_params_and_dropped_points(pkg, ctx, synth):
    sr = pkg.scan_registration
    raw = _raw(synth, 16, 1800)
    p = sr.default_params(ctx)
    p.n_feature_regions, p.curvature_region, p.max_corner_sharp, p.max_surface_flat = 4, 4, 3, 5
    p.less_flat_filter_size, p.surface_curvature_threshold = 0.3, 0.05
    node = _node(pkg, ctx, 16, params=p)
    _assert_equals_composed(pkg, ctx, node, raw, 16, params=p)
    node.close()
    # NaN, zero and out-of-table points, at the front, inside and at the very end but one
    bad = np.array([[np.nan, 1, 1, 0], [1e-4, 1e-4, 1e-4, 0], [1.0, 0.0, 5.0, 0], [np.inf, 0, 0, 0], [1.0, 0.0, -5.0, 0]], np.float32)
    dirty = np.concatenate([raw[:1], bad, raw[1:5000], bad, raw[5000:-1], bad[:3], raw[-1:]])
    node = _node(pkg, ctx, 16)
    _assert_equals_composed(pkg, ctx, node, dirty, 16)
    assert node.last_stats.n_points == len(raw)
    # a ring table that leaves the lowest rings empty: {0, 0} at the front, as MultiScanRegistration.cpp:184-189 has it
    node.close()
    up = raw[np.degrees(np.arctan2(raw[:, 2], np.hypot(raw[:, 0], raw[:, 1]))) > -6.0]
    node = _node(pkg, ctx, 16)
    _assert_equals_composed(pkg, ctx, node, up, 16)
    assert node.cloud()[1][0].tolist() == [0, 0]
    node.close()


# ---- the IMU branch -----------------------------------------------------------------------------------------------------
def _motion(t, yaw_rate=0.8):
    """roll, pitch, yaw and the IMU's linear_acceleration at time t (s) of a vehicle that turns, rocks and accelerates."""
    roll = 0.05 * math.sin(2 * math.pi * 3.0 * t)
    pitch = 0.04 * math.cos(2 * math.pi * 2.0 * t)
    yaw = 0.4 + yaw_rate * t + 0.05 * math.sin(2 * math.pi * 2.0 * t)
    la = (2.5 - math.sin(pitch) * 9.81, 0.7 + math.sin(roll) * math.cos(pitch) * 9.81, math.cos(roll) * math.cos(pitch) * 9.81)
    return roll, pitch, yaw, la


def _feed(node, ref, hz, t_from=-0.05, t_to=0.16, yaw_rate=0.8, t0=T0):
    step = 10 ** 9 // hz
    for k in range(int(math.floor(t_from * hz)), int(math.ceil(t_to * hz)) + 1):
        roll, pitch, yaw, la = _motion(k / hz, yaw_rate)
        node.handle_imu_message(t0 + k * step, (roll, pitch, yaw), la)
        ref.history.push(t0 + k * step, roll, pitch, yaw, la)


def _tolerance(ref_out):
    """6 sqrt(2) (e_t + 3 2^-24) (|p| + |shift|) per point of the ring-sorted cloud: six plane rotations, each an isometry on
    the error it inherits, each adding the trig difference and three roundings."""
    o = ref_out["order"]
    norm = np.linalg.norm(ref_out["xyz_raw"].astype(np.float64), axis=1)[o]
    shift = np.linalg.norm(ref_out["shift"].astype(np.float64), axis=1)[o]
    return 6 * math.sqrt(2) * (E_T + 3 * EPS) * (norm + shift)


# By how much the device's relTime can differ from the restatement's: ori = -atan2f(x, z) is the device's (2 ulp, the bound the
# HIP math API documents) against the rounded double evaluation (0.5 ulp) at |ori| < 16 (ulp 2^-20); relTime =
# scanPeriod (ori - startOri) / (endOri - startOri) with endOri - startOri >= pi, and three float roundings of a value <= 0.11
SCAN_PERIOD = 0.1
D_REL = SCAN_PERIOD / math.pi * 2.5 * 2.0 ** -20 + 3 * EPS * 0.11


def _sensitivity(ref, out, stamp):
    """How the state of every kept point (arrival order) moves with its relTime: the slopes of the history segment it is
    interpolated (or extrapolated) on -- angles (sum of the three axes, rad/s), position, velocity -- its |ratio|, and the
    sizes of the segment's two states (S * (1 - ratio) + E * ratio: a rounding of ratio, of 1 - ratio and of the two products
    is relative to |ratio| times those sizes, not to their difference -- the sum cancels)."""
    n = len(out["rel"])
    z = np.zeros(n)
    if not len(ref.history) or n == 0:
        return dict(ang_rate=z, pos_rate=z, vel_rate=z, ratio=z, a_ang=z, a_pos=z, a_vel=z)
    tsec, dt, rows = ref.history.arrays(stamp)
    idx = out["index"]
    td = tsec[idx] + out["rel"].astype(np.float64)
    interp = ~((idx == 0) | (td > 0))
    S, E = rows[idx].astype(np.float64), rows[np.maximum(idx - 1, 0)].astype(np.float64)
    seg = np.where(interp, dt[idx], 1.0)
    d = np.abs(S - E) * interp[:, None]
    d[:, 2] = np.minimum(d[:, 2], np.abs(2 * math.pi - d[:, 2]))  # (the yaw wrap)
    d_ang, d_pos, d_vel = d[:, 0:3].sum(1), np.linalg.norm(d[:, 3:6], axis=1), np.linalg.norm(d[:, 6:9], axis=1)
    a = (np.abs(S) + np.abs(E)) * interp[:, None]
    return dict(ang_rate=d_ang / seg, pos_rate=d_pos / seg, vel_rate=d_vel / seg, ratio=np.abs(td / seg) * interp, a_ang=a[:, 0:3].sum(1),
                a_pos=np.linalg.norm(a[:, 3:6], axis=1), a_vel=np.linalg.norm(a[:, 6:9], axis=1))


def _rel_term(ref, out, stamp):
    """What the tolerance of the coordinates does NOT model, per kept point in arrival order: |d p / d relTime| D_REL (each
    plane rotation moves a point by at most its norm per radian; the shift moves with the position's slope and the start
    velocity) plus the roundings of the interpolation, which a different ratio makes fall differently: (1 + 2 |ratio|) 2^-24 of
    the two states' sizes."""
    k = _sensitivity(ref, out, stamp)
    norm = np.linalg.norm(out["xyz_raw"].astype(np.float64), axis=1) + np.linalg.norm(out["shift"].astype(np.float64), axis=1)
    return ((k["ang_rate"] * norm + k["pos_rate"] + np.linalg.norm(ref.start_vel)) * D_REL
            + EPS * (1 + 2 * k["ratio"]) * (k["a_ang"] * norm + k["a_pos"]))


def _assert_equals_ref(node_cloud, node_ranges, ref_out, rings, tag="", ref=None, stamp=T0):
    want = ref_out["cloud"]
    assert node_cloud.shape == want.shape and np.array_equal(node_ranges, ref_out["ranges"]), tag
    assert np.array_equal(np.floor(node_cloud[:, 3]), np.floor(want[:, 3])), tag  # same points in the same rings in the same order
    assert np.abs(node_cloud[:, 3] - want[:, 3]).max() <= 2e-6 * rings, tag
    tol = _tolerance(ref_out)
    err = np.linalg.norm(node_cloud[:, :3].astype(np.float64) - want[:, :3].astype(np.float64), axis=1)
    worst = (err / tol).max()
    print("%s de-skew: largest difference %.3e m, %.3f of its tolerance (median tolerance %.3e m)" % (tag, err.max(), worst, np.median(tol)))
    if ref is not None and len(err):  # how much of the tolerance the relTime difference can take, by the model above
        rel_term = _rel_term(ref, ref_out, stamp)[ref_out["order"]]
        print("%s   modelled relTime term: up to %.3f of the tolerance; at the worst point %.3e m" % (tag, (rel_term / tol).max(), rel_term[np.argmax(err / tol)]))
    assert worst <= 1.0, tag
    return tol


def _assert_trans(got, want, ref, ref_out, stamp=T0, tag=""):
    """imu_trans held to what its quantities allow.  The start angles are float operations of the host on the history alone:
    the same bits.  The current angles, the shift and the velocity change are those of the LAST kept point's state, which
    moves with that point's relTime (the device's atan2): its segment's slope times D_REL and the interpolation's roundings at that
    ratio ((1 + 2 |ratio|) 2^-24 of the two states' sizes); the two vectors then go through three plane
    rotations with the start state's sin / cos (E_T and three roundings each, as for the coordinates)."""
    print("%s imu_trans: largest difference %.3e" % (tag, np.abs(got - want).max()))
    assert np.array_equal(bits(got[0]), bits(want[0])), tag
    k = {key: (v[-1] if len(v) else 0.0) for key, v in _sensitivity(ref, ref_out, stamp).items()}
    wobble = EPS * (1 + 2 * k["ratio"])
    assert np.abs(got[1].astype(np.float64) - want[1]).max() <= k["ang_rate"] * D_REL + wobble * k["a_ang"] + 2 * EPS * np.abs(want[1]).max(), tag
    rot = 3 * math.sqrt(2) * (E_T + 3 * EPS)
    rows = ref.history.arrays(stamp)[2] if len(ref.history) else np.zeros((1, 15), np.float32)
    d_shift = (k["pos_rate"] + np.linalg.norm(ref.start_vel)) * D_REL + wobble * k["a_pos"] + 4 * EPS * np.abs(rows[:, 3:6]).max()
    assert np.linalg.norm(got[2].astype(np.float64) - want[2]) <= rot * np.linalg.norm(want[2]) + d_shift, tag
    d_vel = k["vel_rate"] * D_REL + wobble * k["a_vel"] + 4 * EPS * np.abs(rows[:, 6:9]).max()
    assert np.linalg.norm(got[3].astype(np.float64) - want[3]) <= rot * np.linalg.norm(want[3]) + d_vel, tag


@pytest.mark.parametrize("hz", [100, 400])
@pytest.mark.parametrize("rings,steps", [(16, 1800), (64, 1800)])
def test_imu_branch_equals_the_restatement(pkg, ctx, synth, rings, steps, hz):
    sr = pkg.scan_registration
    raw = _raw(synth, rings, steps)
    lo, hi = MAPPERS[rings]
    node, ref = _node(pkg, ctx, rings), R.Registration(lo, hi, rings)
    _feed(node, ref, hz)
    assert node.imu_info()[0] == len(ref.history)
    # the integration on the host: float operations on the C library's sinf / cosf of the pushed angles on both sides -- same bits
    assert np.array_equal(node.imu_info()[1].astype(np.float32), ref.history.rows[-1][3:6])
    want = ref.process(raw, T0)
    # the bound is wide: first make sure, on the restatement alone, that a de-skew that never ran could not hide in it
    tol = _tolerance(want)
    moved = np.linalg.norm(want["xyz"].astype(np.float64) - want["xyz_raw"].astype(np.float64), axis=1)
    assert np.median(moved) >= 100 * np.median(tol)
    fs = sr.FeatureSet(ctx)
    counts = node.process(raw, T0, fs)
    cloud, ranges = node.cloud()
    _assert_equals_ref(cloud, ranges, want, rings, "%d rings, %d Hz" % (rings, hz), ref)
    _assert_trans(node.imu_trans, want["imu_trans"], ref, want, tag="%d rings, %d Hz" % (rings, hz))
    assert node.last_stats.imu_states == len(ref.history) and min(counts.values()) > 0
    # the extraction on the de-skewed cloud is the pinned extraction
    f = sr.extract_features(ctx, cloud, ranges)
    for k in sr.LISTS:
        assert np.array_equal(bits(fs.download(k)), bits(f[k])), k
    fs.close()
    node.close()


def test_the_index_only_walks_forward(pkg, ctx, synth):
    """Points that arrive with relTime NOT monotone (the azimuth steps shuffled in blocks) under a fast, uneven turn."""
    sr = pkg.scan_registration
    rings, steps = 16, 1800
    raw = _raw(synth, rings, steps)
    chunks = np.array_split(np.arange(len(raw)), 30)  # (some rays have no return: the blocks are index ranges, 60 steps or so each)
    rng = np.random.default_rng(4)
    order = [0] + (1 + rng.permutation(28)).tolist() + [29]  # the first and the last block stay: the sweep's start and end orientation
    raw = raw[np.concatenate([chunks[b] for b in order])]
    lo, hi = MAPPERS[rings]
    node, ref, naive = _node(pkg, ctx, rings), R.Registration(lo, hi, rings), R.Registration(lo, hi, rings, index_rule="search")
    for r in (ref, naive):
        _feed(node if r is ref else _Null(), r, 400, yaw_rate=3.0)
    want, other = ref.process(raw, T0), naive.process(raw, T0)
    assert np.any(np.diff(want["rel"]) < -0.01)
    assert np.array_equal(want["index"], R.closed_form_indices(ref.history.arrays(T0)[0], want["rel"]))
    fs = sr.FeatureSet(ctx)
    node.process(raw, T0, fs)
    cloud, ranges = node.cloud()
    tol = _assert_equals_ref(cloud, ranges, want, rings, "shuffled blocks", ref)
    _assert_trans(node.imu_trans, want["imu_trans"], ref, want, tag="shuffled blocks")
    # a search per point that forgets the points before it is another function: the case discriminates
    gap = np.linalg.norm(other["cloud"][:, :3].astype(np.float64) - want["cloud"][:, :3].astype(np.float64), axis=1)
    assert (gap > 100 * tol).sum() > 100
    f = sr.extract_features(ctx, cloud, ranges)
    for k in sr.LISTS:
        assert np.array_equal(bits(fs.download(k)), bits(f[k])), k
    fs.close()
    node.close()


def test_dropped_points_do_not_advance_the_index(pkg, ctx, synth):
    """An IMU history and a cloud with points the registration drops -- NaN, closer than 1 cm, outside the ring table -- whose
    azimuth WOULD give a late relTime, put between early kept points: the device agrees with the restatement, and the kept
    points come out with the bits they have without the dropped ones (they contribute the identity to the prefix maximum)."""
    sr = pkg.scan_registration
    rings = 16
    lo, hi = MAPPERS[rings]
    raw = _raw(synth, rings, 1800)
    late = raw[-3000:-2000].copy()  # relTime about 0.09 s
    up, nan = late.copy(), late.copy()
    up[:, 2] = 5.0 * np.hypot(late[:, 0], late[:, 1])
    nan[:, 1] = np.nan
    near = late * (np.float32(5e-3) / np.linalg.norm(late[:, :3], axis=1, keepdims=True)).astype(np.float32)
    dirty = np.concatenate([raw[:1500], up[:700], raw[1500:4000], near[:1300], raw[4000:9000], nan[:900], raw[9000:]])
    node, ref = _node(pkg, ctx, rings), R.Registration(lo, hi, rings)
    _feed(node, ref, 400, yaw_rate=2.0)
    want = ref.process(dirty, T0)
    assert len(want["rel"]) == len(raw)
    tsec = ref.history.arrays(T0)[0]
    assert R.first_index(tsec, 0.085) > want["index"][1500:9000].max() + 10  # had they counted, these would sit on later states
    fs = sr.FeatureSet(ctx)
    node.process(dirty, T0, fs)
    cloud, ranges = node.cloud()
    _assert_equals_ref(cloud, ranges, want, rings, "dropped points", ref)
    _assert_trans(node.imu_trans, want["imu_trans"], ref, want, tag="dropped points")
    trans = node.imu_trans.copy()
    node.process(raw, T0, fs)
    clean, clean_ranges = node.cloud()
    assert np.array_equal(bits(clean), bits(cloud)) and np.array_equal(clean_ranges, ranges) and np.array_equal(bits(node.imu_trans), bits(trans))
    fs.close()
    node.close()


class _Null:
    def handle_imu_message(self, *a):
        pass


def test_history_edge_cases(pkg, ctx, synth):
    sr = pkg.scan_registration
    rings = 16
    raw = _raw(synth, rings, 900)
    lo, hi = MAPPERS[rings]
    fs = sr.FeatureSet(ctx)
    cases = dict(before=(-0.40, -0.20, 100, 200), after=(0.30, 0.50, 100, 200), one=(0.03, 0.03, 100, 200),
                 inside=(0.02, 0.07, 100, 200), wrapped=(-1.0, 0.16, 100, 50))
    for name, (t_from, t_to, hz, cap) in cases.items():
        node, ref = _node(pkg, ctx, rings, imu_history_size=cap), R.Registration(lo, hi, rings, imu_history_size=cap)
        _feed(node, ref, hz, t_from, t_to)
        assert node.imu_info()[0] == len(ref.history) == (1 if name == "one" else min(cap, len(ref.history)))
        want = ref.process(raw, T0)
        node.process(raw, T0, fs)
        cloud, ranges = node.cloud()
        _assert_equals_ref(cloud, ranges, want, rings, name, ref)
        _assert_trans(node.imu_trans, want["imu_trans"], ref, want, tag=name)
        if name == "wrapped":
            # a second sweep: _imuStart is new, the history has moved on
            _feed(node, ref, hz, 0.17, 0.27)
            want = ref.process(raw, T0 + 100_000_000)
            node.process(raw, T0 + 100_000_000, fs)
            _assert_equals_ref(*node.cloud(), want, rings, "wrapped, second sweep", ref, T0 + 100_000_000)
            _assert_trans(node.imu_trans, want["imu_trans"], ref, want, T0 + 100_000_000, "wrapped, second sweep")
            # forget the IMU: the node is again the composed path, bit for bit
            node.imu_clear()
            assert not node.has_imu_data()
            _assert_equals_composed(pkg, ctx, node, raw, rings)
        node.close()
    fs.close()


def test_refusals_leave_the_node_usable(pkg, ctx, synth):
    sr = pkg.scan_registration
    rings = 16
    lo, hi = MAPPERS[rings]
    raw = _raw(synth, rings, 900)
    node, ref = _node(pkg, ctx, rings), R.Registration(lo, hi, rings)
    fs = sr.FeatureSet(ctx)
    _feed(node, ref, 100)
    want = ref.process(raw, T0)
    node.process(raw, T0, fs)
    trans = node.imu_trans.copy()
    # a stamp that goes back (or stays) is refused, and the history is as it was
    n_before = node.imu_info()[0]
    for stamp in (T0, T0 + 160_000_000):
        with pytest.raises(pkg.LslamError, match="lslam_sreg_imu_push"):
            node.handle_imu_message(stamp, (0, 0, 0), (0, 0, 9.81))
    assert node.imu_info()[0] == n_before
    # an empty cloud is refused, outputs reading nothing
    with pytest.raises(pkg.LslamError, match="lslam_sreg_process"):
        node.process(np.zeros((0, 4), np.float32), T0, fs)
    assert fs.counts() == dict.fromkeys(sr.LISTS, 0)
    # a ring above 2560 points: refused behind the wait; no cloud to hand out; the node works afterwards as before
    big = _raw(synth, rings, 2600)
    with pytest.raises(pkg.LslamError, match="2560"):
        node.process(big, T0, fs)
    assert fs.counts() == dict.fromkeys(sr.LISTS, 0)
    with pytest.raises(pkg.LslamError, match="lslam_sreg_cloud"):
        node.cloud()
    node.process(raw, T0, fs)
    _assert_equals_ref(*node.cloud(), want, rings, "after the refusals")
    assert np.array_equal(bits(node.imu_trans), bits(trans))
    # a sweep without a kept point succeeds with empty lists and leaves _imuCur and the shift as they were: the /imu_trans
    # of the next message still has them (the start state is the new sweep's)
    nothing = np.full((64, 4), np.nan, np.float32)
    assert node.process(nothing, T0, fs) == dict.fromkeys(sr.LISTS, 0)
    assert node.cloud()[0].shape == (0, 4) and node.last_stats.n_points == 0
    assert np.array_equal(bits(node.imu_trans), bits(trans))
    want0 = ref.process(nothing, T0)  # (the restatement carries them over in the same way)
    assert np.array_equal(bits(want0["imu_trans"]), bits(want["imu_trans"]))
    _assert_trans(node.imu_trans, want["imu_trans"], ref, want, tag="after a sweep without a kept point")
    fs.close()
    node.close()


def test_chain_into_the_odometry_node(pkg, ctx, synth, small_problem):
    """Ten consecutive VLP-16 sweeps through MultiScanRegistration.process -> DeviceLaserOdometry.process: the chain the two
    free functions build, bit for bit (no IMU)."""
    from test_gpu_odom import _raw as sweep
    sr = pkg.scan_registration
    world = small_problem["world"]
    node = _node(pkg, ctx, 16)
    od_a, od_b = pkg.DeviceLaserOdometry(ctx), pkg.DeviceLaserOdometry(ctx)
    fa, fb = sr.FeatureSet(ctx), sr.FeatureSet(ctx)
    for k in range(12):  # SYSTEM_DELAY drops the first two clouds of a session: ten sweeps are compared
        raw = sweep(synth, world, k)
        got = node.handle_cloud_message(raw, T0 + k * 100_000_000, fa)
        assert (got is None) == (k < 2)
        if k < 2:
            continue
        reg, rr = sr.multiscan_register(ctx, raw, -15.0, 15.0, 16)
        sr.extract_features_dev(ctx, reg, rr, fb)
        assert fa.counts() == fb.counts()
        T_a, T_b = od_a.process(fa), od_b.process(fb)
        assert (T_a is None) == (T_b is None) == (k == 2)
        if T_a is not None:
            assert np.array_equal(bits(T_a), bits(T_b)) and np.array_equal(bits(od_a.transform), bits(od_b.transform))
        assert np.array_equal(bits(od_a.last_corner), bits(od_b.last_corner)) and np.array_equal(bits(od_a.last_surf), bits(od_b.last_surf))
    assert node.cloud_receive_count == 12 and node.last_stats.sweeps == 10
    for o in (od_a, od_b, fa, fb, node):
        o.close()


def test_nodes_give_their_memory_back(pkg, synth):
    """Eight nodes made, used once and destroyed on contexts that are destroyed: no device memory stays behind beyond what one
    used context with its node holds (the method of tests/test_gpu_ctx_lifetime.py, its settling round included)."""
    import torch
    sr = pkg.scan_registration
    raw = _raw(synth, 64, 2400, seed=5)

    def free():
        return torch.cuda.mem_get_info()[0]

    def use(c):
        node = _node(pkg, c, 64)
        node.handle_imu_message(T0, (0.0, 0.0, 0.1), (0.0, 0.0, 9.81))
        node.handle_imu_message(T0 + 50_000_000, (0.0, 0.0, 0.2), (0.0, 0.0, 9.81))
        fs = sr.FeatureSet(c)
        counts = node.process(raw, T0, fs)
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
    held = eight_alive()
    lost = free0 - free()
    print("one used context and node %.1f MiB, eight %.1f MiB, lost after closing them %.1f MiB" % (one / 2 ** 20, (free0 - held) / 2 ** 20, lost / 2 ** 20))
    assert one > 16 << 20  # (a 153 600-point sweep: the node's arrays and the grouping's sort scratch are tens of megabytes)
    assert lost < one


def test_cpp_registration_equals_the_python_mirror(pkg, synth, small_problem, tmp_path):
    """tests/cpp/registration_end_to_end.cpp (MultiScanRegistration -> LaserOdometry::processFeatureSet in C++) on five sweeps,
    the first two without an IMU: the same ABI calls as the Python mirrors, so the same counts, /imu_trans, _transform and registered-cloud bits."""
    import os
    import struct
    import subprocess
    from test_gpu_odom import _raw as sweep
    sr = pkg.scan_registration
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "registration_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "registration_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    ctx = pkg.Context(0)
    node, odo, fs = pkg.MultiScanRegistration(ctx), pkg.DeviceLaserOdometry(ctx), sr.FeatureSet(ctx)
    want = []
    with open(tmp_path / "session.bin", "wb") as fo:
        for k in range(5):
            t0 = T0 + k * 100_000_000
            if k >= 2:
                for j in range(10):
                    roll, pitch, yaw, la = _motion(0.1 * k + 0.01 * j)
                    node.handle_imu_message(t0 + j * 10_000_000, (roll, pitch, yaw), la)
                    fo.write(struct.pack("<Iq6d", 1, t0 + j * 10_000_000, roll, pitch, yaw, *la))
            raw = np.ascontiguousarray(sweep(synth, small_problem["world"], k)[:, :4], np.float32)
            fo.write(struct.pack("<IqI", 2, t0, len(raw)))
            fo.write(raw.tobytes())
            counts = node.process(raw, t0, fs)
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
    assert len(lines) == 5 and "OK sweeps 5" in out.stdout
    for k, (w, (imu, matched, counts, trans, tf, registered)) in enumerate(zip(lines, want)):
        assert [int(v) for v in w[1:8]] == [k, imu, matched] + counts, k
        got = np.array([float.fromhex(v) for v in w[8:26]], np.float32)
        assert [int(w[26]), int(w[27]), int(w[28], 16)] == registered, k  # laserCloud(cloud, &ranges) = cloud() of the Python mirror
        assert np.array_equal(bits(got[:12]), bits(trans)) and np.array_equal(bits(got[12:]), bits(tf)), k
    assert want[1][0] == 0 and want[2][0] == 1 and np.any(want[4][3] != 0)
