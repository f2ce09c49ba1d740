"""CPU checks of tests/scan_registration_ref.py (the restatement of the registration's IMU branch the GPU tests compare the
device with), against things that do not depend on it: known properties of the de-skew, a scan distorted by a known motion, the
sequential index rule against its closed form, the oracle's ring / relTime."""
import math

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import scan_registration_ref as R

EPS = 2.0 ** -24  # half an ulp of a float32 in [1, 2): the relative rounding error of one float32 operation
G = 9.81
T0 = 1_700_000_000 * 10 ** 9


def _rest_acc(roll, pitch):
    """linear_acceleration of an IMU at rest (zero specific force after handleIMUMessage removes gravity)."""
    return (-math.sin(pitch) * G, math.sin(roll) * math.cos(pitch) * G, math.cos(roll) * math.cos(pitch) * G)


def _cloud(n=4000, seed=0, rings=16):
    """A raw driver cloud in arrival order: azimuth falling along the sweep, every ring per step, ranges 3 .. 40 m."""
    rng = np.random.default_rng(seed)
    steps = n // rings
    az = np.repeat(-np.linspace(0.0, 2 * math.pi * (1 - 1 / steps), steps), rings) + 1.0
    el = np.tile(np.deg2rad(np.linspace(-15, 15, rings)), steps)
    rg = rng.uniform(3.0, 40.0, steps * rings)
    return np.stack([rg * np.cos(el) * np.cos(az), rg * np.cos(el) * np.sin(az), rg * np.sin(el), np.zeros_like(rg)], 1).astype(np.float32)


def test_register_points_is_the_oracles_registration(oracle, synth):
    from test_oracle_features import _raw_sweep
    for rings, lo, hi in ((16, -15.0, 15.0), (64, -24.9, 2.0)):
        raw, _ = _raw_sweep(synth, rings=rings, steps=900, seed=8)
        raw = np.concatenate([raw[:1], [[np.nan, 0, 0, 0], [1e-4, 1e-4, 1e-4, 0], [1.0, 0.0, 5.0, 0]], raw[1:]]).astype(np.float32)
        ref, oranges = oracle.multiscan_register(raw, lo, hi, rings)
        got = R.Registration(lo, hi, rings).process(raw, T0)
        assert np.array_equal(got["ranges"], oranges) and got["cloud"].shape == ref.shape
        assert np.array_equal(got["cloud"][:, :3].view(np.uint32), ref[:, :3].view(np.uint32))
        assert np.array_equal(np.floor(got["cloud"][:, 3]), np.floor(ref[:, 3]))
        assert np.abs(got["cloud"][:, 3] - ref[:, 3]).max() <= 2e-6 * rings  # (atan2 of libm there, of numpy here)
        assert np.all(got["imu_trans"] == 0)


def test_constant_orientation_at_rest_is_the_identity():
    roll, pitch, yaw = 0.21, -0.13, 1.7
    reg = R.Registration()
    for k in range(-3, 15):
        reg.history.push(T0 + k * 10_000_000, roll, pitch, yaw, _rest_acc(roll, pitch))
    raw = _cloud()
    out = reg.process(raw, T0 + 1_234_567)
    assert len(out["xyz"]) == len(raw)
    # gravity leaves a residue of a rounding of 9.81 in acc (float(double)): position of the order 1e-7 * t^2 -- far below
    # the rotation's own rounding.  Six plane rotations there and back with the same rounded sin / cos (c^2 + s^2 = 1 +- 2 EPS):
    # each adds (2 EPS trig + 3 roundings) * sqrt(2) |p|
    norm = np.linalg.norm(out["xyz_raw"].astype(np.float64), axis=1)
    err = np.linalg.norm(out["xyz"].astype(np.float64) - out["xyz_raw"].astype(np.float64), axis=1)
    assert np.all(err <= 6 * math.sqrt(2) * (2 * EPS + 3 * EPS) * norm + 1e-6)
    assert err.max() > 0  # (it did run)


def test_constant_velocity_has_zero_shift():
    reg = R.Registration()
    # accelerate for 50 ms, then coast: the states the sweep sees have a constant velocity
    for k in range(-10, 15):
        la = np.array(_rest_acc(0.0, 0.0)) + ((3.0, -2.0, 1.0) if k < -5 else (0.0, 0.0, 0.0))
        reg.history.push(T0 + k * 10_000_000, 0.0, 0.0, 0.0, la)
    tsec, dt, rows = reg.history.arrays(T0)
    vel = rows[-1, 6:9]
    assert np.linalg.norm(vel) > 0.1 and np.array_equal(rows[-12:, 6:9], np.tile(vel, (12, 1)))
    out = reg.process(_cloud(), T0)
    # position - start position - velocity * t: the LOAM property.  Each term is a float32 of the size of the position
    # (<= |v| * 0.25 s) with a handful of roundings: 16 EPS of that
    shift = np.linalg.norm(out["xyz"].astype(np.float64) - out["xyz_raw"].astype(np.float64), axis=1)
    assert shift.max() <= 16 * EPS * (np.abs(rows[:, 3:6]).max() + 1e-3) + 4 * EPS * 40.0
    assert np.abs(out["imu_trans"][2]).max() <= 16 * EPS * (np.abs(rows[:, 3:6]).max() + 1e-3)
    assert np.abs(out["imu_trans"][3]).max() == 0


@pytest.mark.parametrize("omega,psi0", [(1.0, 0.3), (-2.0, -0.4)])
def test_constant_yaw_rate_restores_the_static_scan(omega, psi0):
    """A static scene seen by a sensor that yaws at a constant rate from rest: the point measured at relTime t is the static
    point turned by -omega t about the vertical.  De-skewing with the IMU stream of that motion gives the static scan back.
    This fixes the conventions: acc.x = a.y ..., yaw -> rotY in the swapped axes = a turn about the sensor's z."""
    reg = R.Registration()
    for k in range(-2, 14):
        t = k * 0.01
        reg.history.push(T0 + k * 10_000_000, 0.0, 0.0, psi0 + omega * t, _rest_acc(0.0, 0.0))
    raw = _cloud(seed=1)
    out = reg.process(raw, T0)
    rel = out["rel"].astype(np.float64)
    x, y, z = (raw[:, k].astype(np.float64) for k in range(3))
    a = omega * rel  # the static point: the measured one turned by +omega t about z
    W = np.stack([x * np.cos(a) - y * np.sin(a), x * np.sin(a) + y * np.cos(a), z], 1)
    got = out["xyz"][:, [2, 0, 1]].astype(np.float64)  # (x', y', z') = (y, z, x)
    # yaw error: the pushed yaws are float32 (EPS |yaw| each, two of them), the interpolation has three roundings of values
    # of that size and a ratio rounded to float32 (EPS * omega * 10 ms): <= 6 EPS max|yaw|; linear interpolation of a linear
    # yaw is otherwise exact.  Then six plane rotations, each sqrt(2) |p| (trig EPS + 3 roundings)
    yaw_max = abs(psi0) + abs(omega) * 0.14
    norm = np.linalg.norm(W, axis=1)
    tol = norm * (6 * EPS * max(yaw_max, 1.0) + 6 * math.sqrt(2) * (EPS + 3 * EPS))
    err = np.linalg.norm(got - W, axis=1)
    assert np.all(err <= tol), (err / tol).max()
    moved = np.linalg.norm(got - raw[:, :3].astype(np.float64), axis=1)
    assert np.median(moved) > 100 * np.median(tol)  # the distortion is far above the bound: the check discriminates
    # _imuTrans: the start yaw and the yaw of the last point's state
    assert abs(out["imu_trans"][0, 1] - psi0) <= 2 * EPS * yaw_max
    assert abs(out["imu_trans"][1, 1] - (psi0 + omega * rel[-1])) <= 6 * EPS * max(yaw_max, 1.0)


@settings(max_examples=300, deadline=None)
@given(st.data())
def test_walking_index_equals_the_closed_form(data):
    """The sequential rule (one index, walked forward over the KEPT points in arrival order) against the closed form the device
    computes over ALL points (prefix maximum in which a dropped point is the identity, then a search): non-monotone relTime,
    dropped points with any relTime between kept ones, history before / after / around the sweep, one state, and a history
    taken from a ring buffer that has wrapped."""
    k = data.draw(st.integers(1, 40))
    gaps = data.draw(st.lists(st.integers(1, 30_000_000), min_size=k, max_size=k))
    where = data.draw(st.sampled_from(["around", "before", "after"]))
    stamps = np.cumsum(gaps)
    if data.draw(st.booleans()):  # through the ring buffer: more pushes than it holds, the oldest overwritten
        h = R.ImuHistory(data.draw(st.integers(1, k)))
        for s_ns in stamps:
            h.push(int(s_ns), 0.0, 0.0, 0.0, (0.0, 0.0, G))
        assert len(h) == h.capacity and h.stamps == [int(v) for v in stamps[k - h.capacity:]]
        stamps = np.array(h.stamps)
    first, span = int(stamps[0]), int(stamps[-1])
    scan = {"around": data.draw(st.integers(first - 20_000_000, span)), "before": span + 500_000_000, "after": first - 500_000_000}[where]
    tsec = np.array([R.to_sec(scan - int(s)) for s in stamps])
    n = data.draw(st.integers(0, 60))
    rel = (np.array(data.draw(st.lists(st.integers(-2000, 15000), min_size=n, max_size=n)), np.float64) * 1e-5).astype(np.float32)
    keep = np.array(data.draw(st.lists(st.booleans(), min_size=n, max_size=n)), bool)  # dropped points never touch the index
    i0, _ = R.walk_indices(tsec, np.zeros(1, np.float32))
    walk, _ = R.walk_indices(tsec, rel[keep], start=i0[0])
    assert np.array_equal(walk, R.closed_form_indices(tsec, rel, keep))
    if where == "before":
        assert np.all(walk == len(stamps) - 1)  # every state is older than the sweep: the last one, as it is
    if where == "after":
        assert np.all(walk == 0)


def test_dropped_points_do_not_advance_the_index():
    """Points the registration drops (NaN, closer than 1 cm, outside the ring table) whose azimuth WOULD give a late relTime,
    put between early kept points: the kept points get the states they get without them."""
    reg_a, reg_b = R.Registration(), R.Registration()
    for k in range(-3, 15):
        t = k * 0.01
        for r in (reg_a, reg_b):
            r.history.push(T0 + k * 10_000_000, 0.05 * math.sin(20 * t), 0.03 * math.cos(15 * t), 0.3 + 2.0 * t, np.array(_rest_acc(0, 0)) + (2.0, 0.5, 0.0))
    raw = _cloud()
    late = raw[-400:-300].copy()          # azimuths of the sweep's end: relTime about 0.09 s
    up = late.copy()
    up[:, 2] = 5.0 * np.hypot(late[:, 0], late[:, 1])   # 78 degrees up: outside the ring table, azimuth kept
    near = late * np.float32(1e-4 / 40.0)                # closer than 1 cm
    nan = late.copy()
    nan[:, 2] = np.nan
    dirty = np.concatenate([raw[:200], up[:40], raw[200:400], near[:30], raw[400:600], nan[:30], raw[600:]])
    a, b = reg_a.process(raw, T0), reg_b.process(dirty, T0)
    # had they counted, the kept points after them would sit on the state of 0.09 s
    tsec = reg_a.history.arrays(T0)[0]
    assert R.first_index(tsec, 0.09) > a["index"][200:600].max() + 3
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["ranges"], b["ranges"])
    assert np.array_equal(a["cloud"].view(np.uint32), b["cloud"].view(np.uint32))
    assert np.array_equal(a["imu_trans"].view(np.uint32), b["imu_trans"].view(np.uint32))


def test_index_over_a_wrapped_history():
    """A ring buffer of 50 that has seen 170 states: the sweep's states are the last 50, and the index walks over those."""
    reg = R.Registration(imu_history_size=50)
    full = R.Registration(imu_history_size=500)
    for k in range(-150, 20):
        t = k * 0.01
        for r in (reg, full):
            r.history.push(T0 + k * 10_000_000, 0.0, 0.0, 0.3 + 1.5 * t, _rest_acc(0, 0))
    assert len(reg.history) == 50 and len(full.history) == 170 and reg.history.stamps == full.history.stamps[-50:]
    raw = _cloud(seed=2)
    a, b = reg.process(raw, T0), full.process(raw, T0)
    assert np.array_equal(a["index"] + 120, b["index"]) and a["index"].min() >= 1 and a["index"].max() < 49
    assert np.array_equal(a["index"], R.closed_form_indices(reg.history.arrays(T0)[0], a["rel"]))
    assert np.array_equal(a["cloud"].view(np.uint32), b["cloud"].view(np.uint32))  # (the states before the window are never looked at)


def test_per_point_search_is_not_the_reference():
    tsec = np.array([R.to_sec(-k * 10_000_000) for k in range(12)])
    rel = np.array([0.0, 0.075, 0.015, 0.045], np.float32)
    walk, _ = R.walk_indices(tsec, rel)
    assert walk.tolist() == [0, 8, 8, 8] and R.per_point_indices(tsec, rel).tolist() == [0, 8, 2, 5]


def test_ring_buffer_wraps():
    h = R.ImuHistory(200)
    for k in range(250):
        h.push(T0 + k * 5_000_000, 0.0, 0.0, 0.0, np.array(_rest_acc(0.0, 0.0)) + (0.0, 1.0, 0.0))
    assert len(h) == 200 and h.stamps[0] == T0 + 50 * 5_000_000 and h.stamps[-1] == T0 + 249 * 5_000_000
    # the integration went on through the overwritten states: v = a t with a = 1 m/s^2 along acc.x (= a.y)
    assert abs(h.rows[-1][6] - 249 * 0.005) <= 1e-4 and abs(h.rows[-1][3] - 0.5 * (249 * 0.005) ** 2) <= 1e-3


def test_yaw_interpolation_across_pi():
    for ya, yb in ((3.1, -3.1), (-3.1, 3.1)):
        h = R.ImuHistory()
        h.push(T0, 0.0, 0.0, ya, _rest_acc(0.0, 0.0))
        h.push(T0 + 10_000_000, 0.0, 0.0, yb, _rest_acc(0.0, 0.0))
        tsec, dt, rows = h.arrays(T0)
        rel = np.array([0.0025, 0.005, 0.0075], np.float32)
        idx, _ = R.walk_indices(tsec, rel)
        ang, trig, _, _ = R.states_for(tsec, dt, rows, idx, rel)
        # the short way round: through +-pi, never through 0
        want = np.array([ya + np.sign(ya) * (2 * math.pi - 6.2) * f for f in (0.25, 0.5, 0.75)])
        d = np.angle(np.exp(1j * (ang[:, 2].astype(np.float64) - want)))
        assert np.abs(d).max() <= 1e-5
        assert np.all(trig[:, 5] < -0.99)
