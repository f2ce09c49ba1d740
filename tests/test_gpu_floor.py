"""Floor detection on the device (csrc/lslam_floor.hip) against tests/floor_ref.py, through the debug tap: the candidate list
and the hypothesis triples integer-equal, every downloaded fp32 plane within the fp32 rounding of the reference's fp64 plane,
the counts integer-equal to counts the reference recomputes from the DOWNLOADED planes, best index and status equal, the refitted
plane within the fp64 summation bound of the reference's exact sums.  Shapes are the smallest at which the kernels can go wrong:
a tile is 1024 points, a wavefront 64, a scoring workgroup takes 128 hypotheses."""
import numpy as np
import pytest

import floor_ref as F

pytestmark = pytest.mark.gpu


def ground_scene(K, n_other=40, n_bad=9, seed=0, sigma=0.01):
    """K candidates near z = -1.8 (x, y in +-8 m), n_other points above the height band, n_bad points with a NaN or an infinite
    coordinate (their other coordinates inside the band), shuffled.  (In IEEE arithmetic such a point can never pass the band
    test either -- a non-finite coordinate times a non-zero up component is infinite or NaN, times a zero one NaN, and every
    sum with those is non-finite -- so the specification's finiteness rule and its band rule agree on every input; the points
    are here so that NaN and infinity flow through every kernel.)"""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-8, 8, K), rng.uniform(-8, 8, K), -1.8 + rng.normal(0, sigma, K)], 1)
    o = np.stack([rng.uniform(-8, 8, n_other), rng.uniform(-8, 8, n_other), rng.uniform(0.0, 3.0, n_other)], 1)
    b = np.stack([rng.uniform(-8, 8, n_bad), rng.uniform(-8, 8, n_bad), np.full(n_bad, -1.8)], 1)
    for i in range(n_bad):
        b[i, i % 3 if i % 3 < 2 else 0] = (np.nan, np.inf, -np.inf)[i % 3]
    pts = np.concatenate([g, o, b])
    pts = pts[rng.permutation(len(pts))]
    out = np.zeros((len(pts), 4), np.float32)
    out[:, :3] = pts
    return out


def check_against_reference(pkg, ctx, pts, **kw):
    """One detection through the host entry point, held to the reference as the module docstring says -> (result, tap, ref)."""
    p = F.params(**kw)
    got = pkg.floor.detect(ctx, pts, kw)
    tap = pkg.floor.debug_hypotheses(ctx)
    own = F.detect(pts, p)  # the reference's own planes
    assert np.array_equal(tap["cand_idx"], own["cand_idx"])
    assert got["n_candidates"] == len(own["cand_idx"])
    assert np.array_equal(tap["triples"], own["triples"])
    assert np.array_equal(np.minimum(tap["counts"], 0), own["marks"])  # which hypotheses are degenerate (-1) / steep (-2)
    finite = pts[np.isfinite(pts[:, :3]).all(1), :3]
    extent = float(np.abs(finite).max()) if len(finite) else 1.0
    bn, bd = F.plane32_bounds(extent)
    live = own["marks"] != -1
    assert np.all(tap["planes"][~live] == 0)
    if live.any():
        err = np.abs(tap["planes"][live].astype(np.float64) - own["planes"][live])
        print("plane error: normal %.3g (bound %.3g), d %.3g (bound %.3g)" % (err[:, :3].max(), bn, err[:, 3].max(), bd))
        assert err[:, :3].max() <= bn and err[:, 3].max() <= bd
    ref = F.detect(pts, p, planes32=tap["planes"])  # ... and from the downloaded planes: every integer must be equal
    assert np.array_equal(tap["counts"], ref["counts"])
    for k in ("status", "best_hypothesis", "best_count", "n_candidates", "n_inliers"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    if ref["refits"]:
        plane, w, N, E = ref["refits"][-1]
        rn, rd = F.refit_bounds(N, E, w)
        err = np.abs(got["plane"] - ref["plane"])
        print("refit error: normal %.3g (bound %.3g), d %.3g (bound %.3g), N %d, gap %.3g" % (err[:3].max(), rn, err[3], rd, N, w[1] - w[0]))
        assert err[:3].max() <= rn and err[3] <= rd
        assert abs(np.linalg.norm(got["plane"][:3]) - 1.0) <= 8 * F.U53
        # every inlier's distance moves by at most sqrt(3) E rn + rd with the plane; the fp64 sum of N squares adds N u relative
        assert abs(got["rms_distance"] - ref["rms_distance"]) <= np.sqrt(3.0) * E * rn + rd + N * F.U53 * max(ref["rms_distance"], 1e-30)
    else:
        assert np.array_equal(got["plane"], ref["plane"])
    return got, tap, ref


@pytest.mark.parametrize("H", [64, 192])
@pytest.mark.parametrize("K", [0, 2, 3, 63, 64, 65, 257, 1024 + 37])
def test_detection_equals_the_reference(pkg, ctx, K, H):
    """K around the wavefront (63, 64, 65), several waves (257), a ragged tail beyond a workgroup's tile (1061), too few to
    fit (0, 2), the fewest that fit (3); H = 64 (one chunk) and 192 (a full scoring chunk of 128 and a ragged one of 64); NaN and
    infinite points mixed in."""
    pts = ground_scene(K, seed=K + H)
    got, tap, ref = check_against_reference(pkg, ctx, pts, n_hypotheses=H, min_inliers=0)
    assert got["n_candidates"] == K and len(tap["counts"]) == H
    if K < 3:
        assert got["status"] == F.FLOOR_FEW_CANDIDATES and got["best_hypothesis"] == -1 and np.all(got["plane"] == 0)
        assert np.all(tap["counts"] == -1)
    elif K >= 63:
        assert got["status"] == F.FLOOR_OK
        ang, dist = F.plane_error(got["plane"], np.array([0, 0, 1, 1.8]))
        assert ang <= 0.01 and dist <= 0.01  # (the planted noise over the patch; the equalities above are the test)


def test_min_inliers_gates_candidates_and_inliers(pkg, ctx):
    pts = ground_scene(257, seed=5)
    got, _, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=258)
    assert got["status"] == F.FLOOR_FEW_CANDIDATES
    pts[:, 2] += np.where(np.arange(len(pts)) % 2 == 0, 0.0, 0.5).astype(np.float32)  # two layers: no plane holds 200 of 257
    got, _, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=200)
    assert got["status"] == F.FLOOR_FEW_INLIERS


def test_identical_candidates_make_every_hypothesis_degenerate(pkg, ctx):
    pts = np.zeros((100, 4), np.float32)
    pts[:, :3] = (1.25, -0.5, -1.75)
    got, tap, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=0)
    assert got["status"] == F.FLOOR_NO_HYPOTHESIS and got["n_candidates"] == 100 and np.all(tap["counts"] == -1)


def layered_scene(seed=3):
    """200 points exactly on z = -2, 20 exactly 0.125 above and 20 exactly 0.125 below: every coordinate is a multiple of 2^-6, so
    a hypothesis drawn from three on-plane points is exactly (0, 0, 1, 2) and the off-plane points lie exactly at the threshold."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(-512, 512, (240, 2)) / 64.0
    z = np.concatenate([np.full(200, -2.0), np.full(20, -1.875), np.full(20, -2.125)])
    pts = np.zeros((240, 4), np.float32)
    pts[:, :2], pts[:, 2] = xy, z
    return pts[rng.permutation(240)]


def test_points_exactly_at_the_threshold_are_inliers_and_ties_go_to_the_lowest_index(pkg, ctx):
    pts = layered_scene()
    # (no refit: the final plane is the winning hypothesis, so the final pass over the inliers meets the equality too)
    got, tap, ref = check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=0, inlier_threshold=0.125, refit_iterations=0)
    flat = np.all(tap["planes"] == np.array([0, 0, 1, 2], np.float32), axis=1)
    assert flat.sum() >= 2, "the scene must hold several exactly horizontal hypotheses"
    assert np.all(tap["counts"][flat] == 240)  # |dist| == threshold counts
    # ... so they tie, at the largest count there can be, and the lowest index wins
    assert got["best_count"] == 240 and got["best_hypothesis"] == int(np.flatnonzero(tap["counts"] == 240)[0])
    assert (tap["counts"] == 240).sum() >= 2
    assert got["status"] == F.FLOOR_OK and got["n_inliers"] == 240


def test_tiny_scene_and_a_refit_that_turns_steep(pkg, ctx):
    """The reference's tiny scene (ground on a 2 % slope, a wall, clutter): found; with 0.5 degrees allowed a few poor
    hypotheses still vote and the refit on their inliers turns beyond the angle -- LSLAM_FLOOR_STEEP, on both sides."""
    pts, planted = F.tiny_scene()
    got, _, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=128)
    ang, dist = F.plane_error(got["plane"], planted)
    assert got["status"] == F.FLOOR_OK and ang <= F.TINY_SIGMA / F.TINY_HALF and dist <= F.TINY_SIGMA
    got, _, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=128, max_normal_angle_deg=0.5)
    assert got["status"] == F.FLOOR_STEEP


def test_max_range_and_a_tilted_up(pkg, ctx):
    """The range gate and an up direction that is not an axis (given unnormalised): both candidate rules and the orientation."""
    rng = np.random.default_rng(11)
    up = np.array([0.1, -0.05, 1.0])
    u = up / np.linalg.norm(up)
    e1 = np.cross(u, [1.0, 0, 0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    ab = rng.uniform(-12, 12, (500, 2))
    g = ab[:, :1] * e1 + ab[:, 1:] * e2 - 1.8 * u + rng.normal(0, 0.01, (500, 1)) * u
    pts = np.zeros((500, 4), np.float32)
    pts[:, :3] = g
    got, _, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=0, max_range=9.0, up=tuple(2.0 * up))
    inside = (np.linalg.norm(pts[:, :3].astype(np.float64), axis=1) <= 8.9).sum()
    assert inside <= got["n_candidates"] < 500 and got["status"] == F.FLOOR_OK
    ang, dist = F.plane_error(got["plane"], np.concatenate([u, [1.8]]))
    assert ang <= 0.01 and dist <= 0.01


def test_synth_scan_floor_against_ground_truth(pkg, ctx, synth):
    """synth.make_scan(rings=16, azimuth_steps=450): the surface cloud's floor against the world floor carried into the sensor
    frame by the returned pose, within ten times what the reference itself achieves there (floor_ref.SYNTH_REF_*, measured on
    the CPU by tests/test_floor_ref.py)."""
    world = synth.World(half_extent=60.0, wall_half=55.0)
    _, surf, pose = synth.make_scan(world, 16, 450)
    R, t = synth.pose_to_Rt(pose)
    got = pkg.floor.detect(ctx, surf)
    assert got["status"] == F.FLOOR_OK
    ang, dist = F.plane_error(got["plane"], F.plane_in_sensor_frame((0, 0, 1, 0), R, t))
    print("synth floor: angle %.3g rad, distance %.3g m" % (ang, dist))
    assert ang <= 10 * F.SYNTH_REF_ANGLE and dist <= 10 * F.SYNTH_REF_DIST


def test_keyframes_in_one_call_equal_single_detections_and_move_no_cloud(pkg, ctx):
    """Five keyframes -- a ground patch, an EMPTY surface cloud, a larger patch with a ragged tile, an all-WALL cloud, a small
    patch -- through lslam_floor_detect_keyframes in one call: bit for bit the five lslam_floor_detect_device results on the
    clouds where they lie, and the store's byte counters do not move."""
    rng = np.random.default_rng(2)
    wall = np.zeros((300, 4), np.float32)
    wall[:, 0], wall[:, 1], wall[:, 2] = 5.0, rng.uniform(-6, 6, 300), rng.uniform(-2.7, -0.9, 300)
    surfs = [ground_scene(300, seed=21), np.zeros((0, 4), np.float32), ground_scene(1024 + 300, seed=22), wall,
             ground_scene(70, seed=23)]
    corner = np.zeros((4, 4), np.float32)
    store = pkg.KeyframeStore(ctx)
    try:
        ids = [store.add(corner, s) for s in surfs]
        before = store.info()
        order = [ids[2], ids[1], ids[0], ids[3], ids[4], ids[2]]  # any order, an id twice
        batch = store.floor_detect(order, dict(n_hypotheses=192, min_inliers=50))
        after = store.info()
        assert after["cloud_bytes_uploaded"] == before["cloud_bytes_uploaded"]
        assert after["cloud_bytes_downloaded"] == before["cloud_bytes_downloaded"]
        for kid, b in zip(order, batch):
            _, _, ps, ns = store.view(kid)
            one = pkg.floor.detect_device(ctx, ps, ns, dict(n_hypotheses=192, min_inliers=50))
            assert one.keys() == b.keys()
            for k in one:
                assert np.array_equal(np.asarray(one[k]), np.asarray(b[k])) and np.asarray(one[k]).tobytes() == np.asarray(b[k]).tobytes(), (kid, k)
            ref = F.detect(surfs[kid], F.params(n_hypotheses=192, min_inliers=50))
            assert b["status"] == ref["status"] and b["n_candidates"] == ref["n_candidates"]
        status = {kid: b["status"] for kid, b in zip(order, batch)}
        assert status[ids[0]] == F.FLOOR_OK and status[ids[2]] == F.FLOOR_OK and status[ids[4]] == F.FLOOR_OK
        assert status[ids[1]] == F.FLOOR_FEW_CANDIDATES and status[ids[3]] == F.FLOOR_NO_HYPOTHESIS
        assert store.floor_detect([]) == []
        with pytest.raises(pkg.LslamError) as e:
            store.floor_detect([ids[0], 99])
        assert e.value.code == pkg.Status.ERR_INVALID and "out of range" in str(e.value)
    finally:
        store.close()


BAD_PARAMS = [dict(up=(0.0, 0.0, 0.0)), dict(up=(np.nan, 0.0, 1.0)), dict(up=(np.inf, 0.0, 1.0)), dict(inlier_threshold=0.0),
              dict(inlier_threshold=-0.1), dict(inlier_threshold=np.nan), dict(n_hypotheses=0), dict(n_hypotheses=32),
              dict(n_hypotheses=100), dict(n_hypotheses=4160), dict(n_hypotheses=-64), dict(min_inliers=-1),
              dict(refit_iterations=-1), dict(sensor_height=np.inf), dict(height_clip_range=-1.0), dict(max_range=-1.0),
              dict(max_normal_angle_deg=np.nan)]


def test_every_rejected_parameter_returns_invalid_and_changes_nothing(pkg, ctx):
    pts = ground_scene(100, seed=9)
    good = pkg.floor.detect(ctx, pts, dict(n_hypotheses=64, min_inliers=0))
    tap = pkg.floor.debug_hypotheses(ctx)
    store = pkg.KeyframeStore(ctx)
    try:
        kid = store.add(np.zeros((1, 4), np.float32), pts)
        _, _, ps, ns = store.view(kid)
        for bad in BAD_PARAMS:
            for call in (lambda: pkg.floor.detect(ctx, pts, bad), lambda: pkg.floor.detect_device(ctx, ps, ns, bad),
                         lambda: store.floor_detect([kid], bad)):
                with pytest.raises(pkg.LslamError) as e:
                    call()
                assert e.value.code == pkg.Status.ERR_INVALID, bad
                assert list(bad)[0] in str(e.value), (bad, str(e.value))  # the message names the parameter
        # ... and leaves the caller's result struct as it was
        import ctypes as C
        capi = __import__("importlib").import_module("the-cooper-mapper_amd.capi")
        r = capi.LslamFloorResult()
        C.memset(C.byref(r), 0xA5, C.sizeof(r))
        image = bytes(C.string_at(C.byref(r), C.sizeof(r)))
        p = pkg.floor.floor_params(n_hypotheses=100)
        assert ctx.lib.lslam_floor_detect(ctx.h, pts.ctypes.data_as(C.c_void_p), len(pts), 16, C.byref(p), C.byref(r)) == -1
        assert ctx.lib.lslam_floor_detect_device(ctx.h, C.c_void_p(ps), ns, C.byref(p), C.byref(r)) == -1
        bad_id = np.array([99], np.int32)
        assert ctx.lib.lslam_floor_detect_keyframes(store.h, 1, bad_id.ctypes.data_as(C.POINTER(C.c_int32)), None, C.byref(r)) == -1
        assert bytes(C.string_at(C.byref(r), C.sizeof(r))) == image
        # nothing has changed: the tap still holds the last good detection, and the same call gives the same bits
        again = pkg.floor.debug_hypotheses(ctx)
        assert all(np.array_equal(tap[k], again[k]) for k in tap)
        once_more = pkg.floor.detect(ctx, pts, dict(n_hypotheses=64, min_inliers=0))
        assert all(np.asarray(good[k]).tobytes() == np.asarray(once_more[k]).tobytes() for k in good)
    finally:
        store.close()


def test_refit_iterations_zero_and_two(pkg, ctx):
    """No refit: the plane is the winning hypothesis's fp32 plane; two refits: two passes, each within its bound of the reference."""
    pts = ground_scene(257, seed=31)
    got, tap, _ = check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=0, refit_iterations=0)
    assert np.array_equal(got["plane"], tap["planes"][got["best_hypothesis"]].astype(np.float64))
    check_against_reference(pkg, ctx, pts, n_hypotheses=64, min_inliers=0, refit_iterations=2)
