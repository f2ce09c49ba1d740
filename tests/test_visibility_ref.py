"""Analytic cases of tests/visibility_ref.py, the numpy restatement of the visibility-vote specification: a sensor at the origin
(z up, the identity pose) whose range image is filled by hand, and query points whose vote can be said without computing."""
import numpy as np

import visibility_ref as V

P = V.params(up_axis=2)
EYE = np.eye(4, dtype=np.float32)
INF = np.float32(np.inf)


def _wall(r=10.0):
    return np.full((P["n_row"], P["n_col"]), np.float32(r), np.float32)


def _at(r, az_deg, el_deg):
    """The point at range r, azimuth and elevation in degrees (z up)."""
    az, el = np.deg2rad(az_deg), np.deg2rad(el_deg)
    return np.array([[r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)]], np.float32)


def _vote(img, pt, p=P):
    f, h = V.vote(img, EYE, pt, p)
    return bool(f[0]), bool(h[0])


def test_pixels_of_ring_centres_and_the_packing():
    q = V.project(np.concatenate([_at(5.0, 0.5, -15.0), _at(5.0, 359.5, 15.0), _at(5.0, 90.5, 1.0)]), P)
    assert q["obs"].all() and q["row"].tolist() == [0, 15, 8] and q["col"].tolist() == [0, 359, 90]
    assert np.allclose(q["r"], 5.0, atol=1e-6)
    w = V.votes([_wall(), _wall()], [EYE, EYE], _at(5.0, 10.0, 1.0), P)
    assert w.dtype == np.uint32 and w.tolist() == [2]                      # two free votes, no hit
    assert V.votes([_wall()] * 3, [EYE] * 3, _at(10.0, 10.0, 1.0), P).tolist() == [3 << 16]
    assert V.dynamic(np.array([2, 1, 2 | (2 << 16), 3 | (2 << 16)], np.uint32), P).tolist() == [True, False, False, True]


def test_in_front_of_on_and_behind_a_wall():
    img = _wall(10.0)
    assert _vote(img, _at(5.0, 40.0, 1.0)) == (True, False)      # the sensor looked through the place: free
    assert _vote(img, _at(10.2, 40.0, 1.0)) == (False, True)     # within max(0.5, 0.02 * 10.2) of the wall: a hit
    assert _vote(img, _at(9.6, 40.0, 1.0)) == (False, True)
    assert _vote(img, _at(9.4, 40.0, 1.0)) == (True, False)      # 0.6 m in front of it: beyond the margin
    assert _vote(img, _at(15.0, 40.0, 1.0)) == (False, False)    # behind the wall: occluded, no vote
    far = _wall(70.0)
    assert _vote(far, _at(68.7, 40.0, 1.0)) == (False, True)     # the relative margin: 0.02 * 68.7 = 1.37 > 1.3
    assert _vote(far, _at(68.5, 40.0, 1.0)) == (True, False)


def test_not_observable_means_no_vote():
    img = _wall(10.0)
    assert _vote(img, _at(0.5, 40.0, 1.0)) == (False, False)     # inside min_range
    assert _vote(_wall(200.0), _at(90.0, 40.0, 1.0)) == (False, False)   # beyond max_range
    assert _vote(img, _at(5.0, 40.0, 30.0)) == (False, False)    # above the field of view
    assert _vote(img, _at(5.0, 40.0, -16.5)) == (False, False)   # below it
    assert _vote(img, np.array([[np.nan, 1.0, 0.0]], np.float32)) == (False, False)
    assert _vote(img, np.array([[np.inf, 1.0, 0.0]], np.float32)) == (False, False)


def test_ground_between_two_rings_is_not_free_with_a_window():
    """A sensor 1.8 m above flat ground: ring -15 deg meets it at 6.95 m, ring -13 deg at 8.0 m.  A ground point between them
    (elevation -13.92 deg, range 7.48 m) falls into the -13 deg row, whose pixel is 0.52 m behind it -- free by the centre pixel
    alone -- but the lower ring's return is nearer than the point: with window = 1 the vote is not free."""
    img = np.full((P["n_row"], P["n_col"]), INF, np.float32)
    img[0, :] = np.float32(1.8 / np.sin(np.deg2rad(15.0)))
    img[1, :] = np.float32(1.8 / np.sin(np.deg2rad(13.0)))
    pt = _at(1.8 / np.sin(np.deg2rad(13.92)), 200.0, -13.92)
    assert V.project(pt, P)["row"].tolist() == [1]
    assert _vote(img, pt, V.params(up_axis=2, window=0)) == (True, False)
    assert _vote(img, pt, V.params(up_axis=2, window=1)) == (False, False)


def test_the_column_window_wraps():
    img = np.full((P["n_row"], P["n_col"]), INF, np.float32)
    img[8, 0] = 20.0                # the centre pixel of a point at azimuth 0.5 deg, elevation 1 deg
    img[8, P["n_col"] - 1] = 5.0    # its left neighbour, across the seam
    assert _vote(img, _at(5.0, 0.5, 1.0)) == (False, True)
    assert _vote(img, _at(5.0, 0.5, 1.0), V.params(up_axis=2, window=0)) == (True, False)
    img2 = np.full_like(img, INF)
    img2[8, P["n_col"] - 1] = 20.0
    img2[8, 0] = 5.0
    assert _vote(img2, _at(5.0, 359.5, 1.0)) == (False, True)
    # rows do not wrap: the top row's window has no row above it
    img3 = np.full_like(img, INF)
    img3[15, 40] = 20.0
    img3[0, 40] = 5.0
    assert _vote(img3, _at(5.0, 40.5, 15.0)) == (True, False)


def test_a_centre_pixel_without_a_return_never_votes_free():
    img = np.full((P["n_row"], P["n_col"]), INF, np.float32)
    img[8, 39] = img[8, 41] = img[7, 40] = img[9, 40] = 30.0     # returns all around, all far behind
    assert _vote(img, _at(5.0, 40.5, 1.0)) == (False, False)
    img[8, 40] = 30.0
    assert _vote(img, _at(5.0, 40.5, 1.0)) == (True, False)
    assert _vote(np.full_like(img, INF), _at(5.0, 40.5, 1.0)) == (False, False)


def test_range_image_is_the_minimum_and_up_axis_1_is_loams_frame():
    pts = np.concatenate([_at(12.0, 40.5, 1.0), _at(7.0, 40.4, 1.2), _at(9.0, 40.6, 0.8), _at(0.5, 10.0, 1.0), _at(5.0, 10.0, 40.0)])
    cloud = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], axis=1)
    img = V.range_image(cloud[:1], cloud[1:], P)
    assert np.isfinite(img).sum() == 1 and abs(float(img[8, 40]) - 7.0) < 1e-5
    loam = cloud[:, [1, 2, 0, 3]]                                # (x, y, z) -> LOAM's (y, z, x): z forward, x left, y up
    assert np.array_equal(V.range_image(loam[:1], loam[1:], V.params(up_axis=1)), img)
    assert np.isinf(V.range_image(cloud[:0], cloud[:0], P)).all()


def test_inverse_pose_and_the_ambiguity_mask():
    T = V.pose_matrix(np.array([0.1, -0.2, 0.7, 3.0, -2.0, 1.5])).astype(np.float32)
    pts = np.random.default_rng(0).uniform(-20, 20, (50, 3)).astype(np.float32)
    back = V.transform(V.inverse_pose(T), V.transform(T, pts))
    assert np.abs(back - pts).max() < 1e-4
    edge = _at(5.0, 40.0, 1.0)          # azimuth exactly on the edge of columns 39 / 40 (up to rounding)
    centre = _at(5.0, 40.5, 1.0)
    keep = V.unambiguous(np.concatenate([edge, centre]), None, P, margin=1e-6)
    assert keep.tolist() == [False, True]
    assert len(V.drop_ambiguous(np.concatenate([edge, centre]), [EYE], P, margin=1e-6)) == 1
