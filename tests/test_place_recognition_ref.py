"""The numpy restatement of the scan-context specification (tests/place_recognition_ref.py) against the properties the
specification states: no device, no library."""
import numpy as np
import pytest

import place_recognition_ref as ref


def _to_loam(c):
    o = c.copy()
    o[:, :3] = c[:, [1, 2, 0]]  # (x, y, z)_loam = (y, z, x)_world
    return o


@pytest.fixture(scope="module")
def scan(synth, small_problem):
    c, s, _gt = synth.make_scan(small_problem["world"], 16, 900, gt_pose=(0, 0, 0.3, 3.0, -2.0, synth.SENSOR_HEIGHT), seed=11)
    return c, s


def test_column_permutation_is_distance_zero_at_that_shift(scan):
    p = ref.params(up_axis=2)
    D = ref.descriptor(scan[0], scan[1], p)
    assert (D > 0).sum() > 50
    for k in (0, 1, 17, p["n_sector"] - 1):
        # Q[:, j] = D[:, (j + k) mod S]
        d, s = ref.distance(np.roll(D, -k, axis=1), D)
        assert d <= 1e-15 and s == k


def test_empty_descriptor_is_at_distance_one(scan):
    p = ref.params(up_axis=2)
    D = ref.descriptor(scan[0], scan[1], p)
    E = ref.descriptor(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), p)
    assert not E.any()
    assert ref.distance(E, D) == (1.0, 0) and ref.distance(D, E) == (1.0, 0) and ref.distance(E, E) == (1.0, 0)


@pytest.mark.parametrize("up_axis", [1, 2])
@pytest.mark.parametrize("shape", [(20, 60), (7, 33)])
def test_rotation_about_the_up_axis_is_the_shift(scan, up_axis, shape):
    p = ref.params(n_ring=shape[0], n_sector=shape[1], up_axis=up_axis)
    conv = _to_loam if up_axis == 1 else (lambda c: c)
    c, s = conv(scan[0]), conv(scan[1])
    C = ref.descriptor(c, s, p)
    step = ref.TWO_PI / p["n_sector"]
    # round(psi / step) is the specified shift; at a fraction near one half two shifts are equally good, so the angles keep the
    # fraction within 0.3 of an integer
    for psi in (10.03 * step, -7.25 * step, (p["n_sector"] - 3.8) * step, 0.3 * step, 2.0 * step):
        Q = ref.descriptor(ref.rotate_about_up(c, psi, up_axis), ref.rotate_about_up(s, psi, up_axis), p)
        d, sh = ref.distance(Q, C)
        assert sh == ref.yaw_shift(psi, p["n_sector"]), (psi, sh, d)


@pytest.mark.parametrize("n_sector", [60, 33])
def test_drop_ambiguous_removes_at_most_one_percent(scan, n_sector):
    """A condition of the GPU descriptor tests: the scan's azimuth grid lands on sector walls for some points."""
    p = ref.params(n_sector=n_sector, up_axis=2)
    cloud = np.concatenate(scan)  # the scan: its corner and surf points
    kept = ref.drop_ambiguous(cloud, p)
    print("drop_ambiguous at %d sectors: %d of %d points" % (n_sector, len(cloud) - len(kept), len(cloud)))
    assert len(cloud) - len(kept) <= 0.01 * len(cloud)
    assert len(ref.drop_ambiguous(kept, p)) == len(kept)


def test_dropped_and_edge_points(scan):
    p = ref.params(n_ring=4, n_sector=8, max_range=10.0, height_offset=2.0, up_axis=2)
    def one(x, y, z):
        return ref.descriptor(np.array([[x, y, z, 0]], np.float32), np.zeros((0, 4), np.float32), p)
    assert one(1.0, 0.1, 0.5)[0, 0] == np.float32(2.5)
    assert one(0.1, 1.0, 0.5)[0, 1] == np.float32(2.5)       # +a towards +b
    assert one(1.0, -0.1, 0.5)[0, 7] == np.float32(2.5)      # a negative angle wraps to the last sector
    assert one(9.9, 0.1, 0.5)[3, 0] == np.float32(2.5)
    for bad in ((10.0, 0.0, 0.5), (0.0, 0.0, 0.5), (1.0, 0.1, -2.0), (1.0, 0.1, -3.0), (np.nan, 0.1, 0.5), (1.0, np.inf, 0.5),
                (1.0, 0.1, -np.inf)):
        assert not one(*bad).any(), bad
