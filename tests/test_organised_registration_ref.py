"""The CPU restatement of the organised registration node (tests/organised_registration_ref.py) held against a literal
transcription of the reference's double loop, on the cases the node's quirks live in."""
import numpy as np
import pytest

import organised_registration_ref as O
import scan_registration_ref as R

F = np.float32
T0 = 1_700_000_000 * 10 ** 9


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(xyz, ring, **kw):
    a, b = O.process(xyz, ring, **kw), O.process_literal(xyz, ring, **kw)
    assert a["cloud"].shape == b["cloud"].shape
    assert np.array_equal(bits(a["cloud"]), bits(b["cloud"])) and np.array_equal(a["ranges"], b["ranges"])
    return a


def _image(h, w, seed=0, lo=3.0, hi=40.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(h, w, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return (d * rng.uniform(lo, hi, (h, w, 1))).astype(np.float32)


def test_scattered_invalid_points_and_rings_that_are_not_the_row():
    xyz = _image(5, 37, seed=1)
    rng = np.random.default_rng(2)
    bad = rng.permutation(5 * 37)[:60]
    flat = xyz.reshape(-1, 3)
    flat[bad[:15], 0] = np.nan
    flat[bad[15:25], 1] = np.inf
    flat[bad[25:35], 2] = -np.inf
    flat[bad[35:]] *= F(0.05)  # nearer than the blind radius
    ring = (1000 + np.arange(5, dtype=np.uint16)[::-1])[:, None].repeat(37, 1)  # reversed, offset: not the row
    out = _assert_same(xyz, ring)
    keep = np.ones(5 * 37, bool)
    keep[bad] = False
    assert np.array_equal(out["keep"].reshape(-1), keep) and len(out["cloud"]) == 5 * 37 - 60
    # x, y, z unchanged (no axis swap); the 4th channel is the ring FIELD plus the column's time
    assert np.array_equal(bits(out["cloud"][:, :3]), bits(flat[keep]))
    rows, cols = np.nonzero(out["keep"])
    want = np.array([F(F(int(ring[r, c])) + F(float(F(0.1)) * float(c) / 37)) for r, c in zip(rows, cols)], np.float32)
    assert np.array_equal(bits(out["cloud"][:, 3]), bits(want))
    assert np.array_equal(np.floor(out["cloud"][:, 3]).astype(int), 1004 - rows)


def test_rel_time_is_the_double_expression_rounded_once():
    for w, period in ((1800, 0.1), (2048, 0.1), (37, 0.05), (1, 0.1), (3000, 0.1)):
        want = np.array([F(float(F(period)) * float(c) / w) for c in range(w)], np.float32)
        assert np.array_equal(bits(O.rel_times(w, period)), bits(want))
    # not the float expression: the two differ somewhere on a real sensor's width
    as_float = (F(0.1) * np.arange(1800, dtype=np.float32)) / F(1800)
    assert np.any(bits(as_float) != bits(O.rel_times(1800)))


def test_the_blind_radius_is_strict():
    xyz = np.array([[[2.5, 0, 0], [1.5, 2.0, 0], [0, 0, np.nextafter(F(2.5), F(0))], [0, 0, 0], [0, 1.5, -2.0]]], np.float32)
    ring = np.zeros((1, 5), np.uint16)
    out = _assert_same(xyz, ring, blind_radius=2.5)
    assert out["keep"].tolist() == [[True, True, False, False, True]]  # x*x + y*y + z*z == 6.25 is not < 6.25
    # blind radius 0: nothing is "< 0", a zero point stays
    out = _assert_same(xyz, ring, blind_radius=0.0)
    assert out["keep"].all() and len(out["cloud"]) == 5


def test_all_invalid_and_one_by_one():
    xyz = np.full((4, 9, 3), np.nan, np.float32)
    out = _assert_same(xyz, np.zeros((4, 9), np.uint16))
    assert out["cloud"].shape == (0, 4) and out["ranges"].tolist() == [[0, 0]] * 4
    one = np.array([[[3.0, 4.0, 0.0]]], np.float32)
    out = _assert_same(one, np.array([[7]], np.uint16))
    assert out["cloud"].tolist() == [[3.0, 4.0, 0.0, 7.0]] and out["ranges"].tolist() == [[0, 0]]
    out = _assert_same(one * F(0.1), np.array([[7]], np.uint16))
    assert out["cloud"].shape == (0, 4) and out["ranges"].tolist() == [[0, 0]]


def test_empty_rows_at_front_middle_and_end():
    xyz = _image(7, 11, seed=3)
    for r in (0, 1, 3, 6):
        xyz[r] = np.nan
    out = _assert_same(xyz, np.arange(7, dtype=np.uint16)[:, None].repeat(11, 1))
    # {0, 0} at the front, {size, size - 1} later (IndexRange(first, size > 0 ? size - 1 : 0))
    assert out["ranges"].tolist() == [[0, 0], [0, 0], [0, 10], [11, 10], [11, 21], [22, 32], [33, 32]]


def _feed(history, t_from, t_to, hz=100):
    import math
    step = 10 ** 9 // hz
    for k in range(int(math.floor(t_from * hz)), int(math.ceil(t_to * hz)) + 1):
        t = k / hz
        roll, pitch, yaw = 0.05 * math.sin(19 * t), 0.04 * math.cos(12 * t), 0.4 + 0.8 * t
        history.push(T0 + k * step, roll, pitch, yaw, (2.5 - math.sin(pitch) * 9.81, 0.7, 9.7))


@pytest.mark.parametrize("span", [(-0.05, 0.16), (0.02, 0.07), (-0.4, -0.2), (0.03, 0.03)])
def test_imu_trans_has_the_start_state_and_nothing_of_the_sweep(span):
    reg = O.Registration()
    assert np.all(reg.process(_image(2, 5), np.zeros((2, 5), np.uint16), T0)["imu_trans"] == 0)  # no IMU heard: zeros
    other = R.Registration()  # the multi-scan restatement on the same history: its start state is the same function
    for h in (reg.history, other.history):
        _feed(h, *span)
    t = reg.process(_image(2, 5), np.zeros((2, 5), np.uint16), T0)["imu_trans"]
    want = other.process(np.full((4, 4), np.nan, np.float32), T0)["imu_trans"]  # no kept point: _imuCur and the shift stay zero
    assert np.array_equal(bits(t[0]), bits(want[0]))
    assert np.all(t[1] == 0) and np.all(t[2] == 0)  # (as numbers: a rotated zero vector may be -0)
    ang, trig, vel = O.start_state(reg.history, T0)
    assert np.array_equal(bits(t[3]), bits(np.array(R.rotate_yxz_neg(tuple(F(0) - v for v in vel), tuple(trig)), np.float32)))
    # against the other restatement: its interpolated start carries the correctly rounded sin / cos, the host's Angle(float)
    # the C library's -- one ulp apart at most, three plane rotations
    assert np.abs(t[3] - want[3]).max() <= 3 * 2.0 ** -22 * max(1e-30, np.abs(vel).max())
    if span in ((-0.4, -0.2), (0.03, 0.03)):
        assert len(reg.history) == (1 if span[0] == span[1] else 21)
    if span == (-0.05, 0.16):
        assert np.linalg.norm(t[3]) > 1e-3  # the history moves: the row is not trivially zero
