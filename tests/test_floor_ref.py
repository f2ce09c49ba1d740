"""tests/floor_ref.py held to the specification on the CPU: the hash against vectors worked out once from MurmurHash3's
published finaliser, the stages' rules on hand-made inputs, the whole detection on the tiny scene and on a synthetic scan (whose
measured errors are the figures floor_ref records for the GPU test)."""
import math

import numpy as np

import floor_ref as F


def test_hash_vectors():
    # fmix32: h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16 (mod 2^32).  0 is its fixed point;
    # 1 -> 1 * 0x85EBCA6B = 0x85EBCA6B, ^ >> 13 = 0x85EBE6F4 ... the published values:
    assert F.fmix32(0) == 0
    assert F.fmix32(1) == 0x514E28B7
    assert F.fmix32(2) == 0x30F4C306
    assert F.fmix32(0xFFFFFFFF) == 0x81F16F39
    assert F.fmix32(0x9E3779B9) == 0x92CA2F0E
    # slot j of hypothesis h: (fmix32(seed + 0x9E3779B9 (3 h + j + 1)) K) >> 32, everything mod 2^32
    assert F.slots(1, 3, 1000).tolist() == [[588, 73, 590], [475, 348, 802], [972, 354, 106]]
    assert F.slots(0xDEADBEEF, 65, 65)[62:].tolist() == [[31, 32, 2], [19, 18, 12], [0, 30, 28]]  # the sum wraps past 2^32
    assert np.all(F.slots(7, 64, 1) == 0) and np.all(F.slots(7, 64, 0) == 0)
    s = F.slots(3, 256, 65)
    assert s.min() >= 0 and s.max() <= 64


def test_candidate_rule():
    p = F.params(max_range=5.0)
    pts = np.array([[0, 0, -1.8, 0],        # in the band
                    [0, 0, -0.8, 0],        # on its upper edge: -(1.8 - 1.0), inclusive
                    [0, 0, -2.8, 0],        # on its lower edge
                    [0, 0, -0.79, 0],       # above
                    [0, 0, -2.81, 0],       # below
                    [3, 4, 0.0, 0],         # range 5 exactly but outside the band
                    [3, 3.8, -1.0, 0],      # inside both: range^2 = 24.44
                    [4, 3, -1.0, 0],        # range^2 = 26 > 25
                    [np.nan, 0, -1.8, 0], [0, np.inf, -1.8, 0], [0, 0, -np.inf, 0]], np.float32)
    assert F.candidates(pts, p).tolist() == [0, 1, 2, 6]
    assert F.candidates(pts, F.params()).tolist() == [0, 1, 2, 6, 7]
    # an up that is not unit is normalised; a flipped one looks for the floor above
    assert F.candidates(pts, F.params(up=(0, 0, 3.0))).tolist() == [0, 1, 2, 6, 7]
    assert F.candidates(-pts, F.params(up=(0, 0, -1.0))).tolist() == [0, 1, 2, 6, 7]
    assert F.candidates(pts[:0], p).tolist() == []


def test_hypothesis_marks_orientation_and_tie_rule():
    cand = np.array([[0, 0, -2], [1, 0, -2], [0, 1, -2], [2, 0, -2], [0, 0, -1], [0, 3, -2]], np.float32)
    p = F.params(n_hypotheses=64, seed=5)
    tri, planes, mark = F.hypotheses(cand, p)
    assert tri.shape == (64, 3) and set(np.unique(mark)) <= {0, -1, -2}
    for h in range(64):
        a, b, c = (cand[s].astype(np.float64) for s in tri[h])
        n = np.cross(b - a, c - a)
        if len(set(tri[h].tolist())) < 3 or n @ n <= 1e-12 * ((b - a) @ (b - a)) * ((c - a) @ (c - a)):
            assert mark[h] == -1 and np.all(planes[h] == 0)  # coincident slots, or collinear points (0, 1, 3 lie on a line)
            continue
        assert abs(np.linalg.norm(planes[h, :3]) - 1) < 1e-15 and planes[h, 2] >= 0  # unit, oriented to up
        assert np.abs(cand[tri[h]].astype(np.float64) @ planes[h, :3] + planes[h, 3]).max() < 1e-15
        assert mark[h] == (-2 if planes[h, 2] < math.cos(math.radians(10.0)) else 0)
    assert (mark == 0).any() and (mark == -1).any() and (mark == -2).any()
    assert F.best(np.array([-1, 3, 7, -2, 7, 2])) == 2  # the lowest index among equals
    assert F.best(np.array([-1, -2, -1])) == -1 and F.best(np.array([-1, 0, 0])) == 1
    assert np.all(F.hypotheses(cand[:0], p)[2] == -1) and np.all(F.hypotheses(cand[:2], p)[2] == -1)


def test_inlier_test_is_inclusive_in_fp32():
    cand = np.array([[0.5, 0.25, -2.0], [1, 1, -1.875], [1, 1, -2.125], [1, 1, -1.8125]], np.float32)
    assert F.inliers32(np.array([0, 0, 1, 2], np.float32), cand, 0.125).tolist() == [True, True, True, False]
    assert F.inliers32(np.array([np.nan] * 4, np.float32), cand, 0.125).tolist() == [False] * 4


def test_tiny_scene_finds_the_planted_plane_within_the_planted_noise():
    """1600 ground points on a 2 % slope, a 400-point wall, 300 clutter points; 128 hypotheses as in the prototype.  The normal
    within noise / half width of the patch, the distance within the noise."""
    pts, planted = F.tiny_scene()
    r = F.detect(pts, F.params(n_hypotheses=128))
    assert r["status"] == F.FLOOR_OK and r["n_candidates"] > 1600 and r["best_count"] >= 1590 and r["n_inliers"] >= 1590
    ang, dist = F.plane_error(r["plane"], planted)
    print("tiny scene: angle %.3g rad, distance %.3g m, rms %.3g" % (ang, dist, r["rms_distance"]))
    assert ang <= F.TINY_SIGMA / F.TINY_HALF and dist <= F.TINY_SIGMA
    assert r["rms_distance"] <= 3 * F.TINY_SIGMA
    assert abs(np.linalg.norm(r["plane"][:3]) - 1) < 1e-15 and r["plane"][2] > 0
    assert r["best_hypothesis"] == F.best(r["counts"]) and r["counts"][r["best_hypothesis"]] == r["best_count"]
    # the statuses on the same scene
    assert F.detect(pts, F.params(n_hypotheses=128, min_inliers=5000))["status"] == F.FLOOR_FEW_CANDIDATES
    assert F.detect(pts, F.params(n_hypotheses=128, min_inliers=1800))["status"] == F.FLOOR_FEW_INLIERS
    # the slope is 1.15 deg: at 0.5 deg a few poor hypotheses still vote, and the refit on their inliers turns beyond the angle
    assert F.detect(pts, F.params(n_hypotheses=128, max_normal_angle_deg=0.5))["status"] == F.FLOOR_STEEP
    assert F.detect(pts, F.params(n_hypotheses=128, max_normal_angle_deg=0.0))["status"] == F.FLOOR_NO_HYPOTHESIS
    assert F.detect(pts[:2], F.params(min_inliers=0))["status"] == F.FLOOR_FEW_CANDIDATES


def test_synth_scan_floor_and_the_recorded_figures(synth):
    """What the reference achieves on synth.make_scan(rings=16, azimuth_steps=450) with the default parameters, against the
    world floor in the sensor frame: the recorded figures (floor_ref.SYNTH_REF_*) are these, rounded up."""
    world = synth.World(half_extent=60.0, wall_half=55.0)
    _, surf, pose = synth.make_scan(world, 16, 450)
    R, t = synth.pose_to_Rt(pose)
    r = F.detect(surf, F.params())
    assert r["status"] == F.FLOOR_OK
    ang, dist = F.plane_error(r["plane"], F.plane_in_sensor_frame((0, 0, 1, 0), R, t))
    print("synth scan: %d points, %d candidates, angle %.3g rad, distance %.3g m" % (len(surf), r["n_candidates"], ang, dist))
    assert ang <= F.SYNTH_REF_ANGLE and dist <= F.SYNTH_REF_DIST
    assert ang >= F.SYNTH_REF_ANGLE / 4 or dist >= F.SYNTH_REF_DIST / 4, "the recorded figures are stale: record the new ones"


def test_bounds_are_what_their_derivations_say():
    bn, bd = F.plane32_bounds(10.0)
    assert 2.0 ** -25 < bn < 2.0 ** -24 and 2.0 ** -20 < bd < 2.0 ** -18  # sqrt(3) 10 = 17.3 < 32: half an ulp is 2^-20
    rn, rd = F.refit_bounds(1600, 10.0, np.array([1e-4, 30.0, 35.0]))
    assert 1e-12 < rn < 1e-9 and rn < rd < 1e-8


# ---- plane priors ----------------------------------------------------------------------------------------------------------
def _random_pose(rng):
    import posegraph_prior_ref as pp
    d = np.concatenate([rng.uniform(-10, 10, 3), np.clip(rng.normal(0, 0.4, 3), -0.55, 0.55)])
    return pp.po.pose_mul(pp.IDENT[None], pp.po.from_vector_mqt(d[None]))[0]


def test_plane_jacobian_against_central_differences_under_the_update_rule():
    """200 random poses (|t| up to 10 m, rotations up to about 70 degrees) and plane pairs: the analytic J against central
    differences of the error under X <- X * fromVectorMQT(d), and the differences against themselves at h / 2 -- the recorded
    floor PLANE_FD_REL, (a) of floor_ref's plane-prior docstring."""
    rng = np.random.default_rng(0)
    worst = worst_h = 0.0
    for _ in range(200):
        pose = _random_pose(rng)
        w, m = (np.concatenate([rng.normal(size=3), [rng.uniform(-3, 3)]]) for _ in range(2))
        J, Jn, Jh = F.plane_jacobian(pose, w, m), F.plane_jacobian_numeric(pose, w, m), F.plane_jacobian_numeric(pose, w, m, 5e-7)
        worst = max(worst, np.abs(J - Jn).max() / np.abs(J).max())
        worst_h = max(worst_h, np.abs(Jn - Jh).max() / np.abs(J).max())
    print("analytic against central differences %.3e, h against h / 2 %.3e" % (worst, worst_h))
    assert worst <= F.PLANE_FD_REL and worst_h <= F.PLANE_FD_REL
    assert worst_h >= F.PLANE_FD_REL / 10, "the recorded floor is stale: record the new one"


def test_tangent_basis_is_orthonormal_and_its_tie_rule_holds():
    rng = np.random.default_rng(1)
    for _ in range(100):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        b1, b2 = F.tangent_basis(n)
        B = np.stack([b1, b2, n])
        assert np.abs(B @ B.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(B) - 1.0) < 1e-15  # right-handed (b1, b2, n)
    # ties: the lowest index among the smallest |components|
    b1, _ = F.tangent_basis(np.array([0.0, 0.0, 1.0]))      # |x| = |y| = 0: axis x -> b1 = z x x = y
    assert np.array_equal(b1, [0.0, 1.0, 0.0])
    b1, _ = F.tangent_basis(np.array([1.0, 0.0, 0.0]))      # |y| = |z| = 0: axis y -> b1 = x x y = z
    assert np.array_equal(b1, [0.0, 0.0, 1.0])
    s = 1.0 / np.sqrt(3.0)
    b1, _ = F.tangent_basis(np.array([s, -s, s]))           # all equal: axis x
    assert b1[0] == 0.0 and abs(b1 @ np.array([s, -s, s])) < 1e-16
    b1, _ = F.tangent_basis(np.array([0.6, 0.0, -0.8]))     # the smallest is y alone
    assert np.allclose(b1, np.cross([0.6, 0.0, -0.8], [0, 1, 0]))


def test_plane_error_is_zero_at_the_truth_and_measures_tilt_and_distance():
    import posegraph_prior_ref as pp
    rng = np.random.default_rng(2)
    pose = _random_pose(rng)
    world = np.array([0.0, 0.0, 2.0, 1.0])  # un-normalised on purpose: the plane z = -0.5
    nl, dl = F.plane_local(pose, world)
    assert abs(np.linalg.norm(nl) - 1) < 1e-15 and abs(dl - (0.5 + pose[2])) < 1e-15
    assert np.abs(F.plane_error3(pose, world, 3.0 * np.concatenate([nl, [dl]]))).max() < 1e-15
    e = F.plane_error3(pose, world, np.concatenate([nl, [dl - 0.25]]))
    assert np.abs(e[:2]).max() < 1e-15 and abs(e[2] - 0.25) < 1e-15
    # a yaw of the keyframe about the world normal changes nothing: the constraint is blind to it (a POSE prior's error is not)
    yaw = pp.po.pose_mul(np.array([[0, 0, 0, 0, 0, np.sin(0.35), np.cos(0.35)]]), pose[None])[0]
    yaw[:3] = pose[:3]
    assert np.abs(pp.quat_matrix(yaw[3:]) - pp.quat_matrix(pose[3:])).max() > 0.1
    meas = np.concatenate([nl, [dl]]) + np.array([0.02, -0.01, 0.03, 0.1])
    assert np.abs(F.plane_error3(yaw, world, meas) - F.plane_error3(pose, world, meas)).max() < 1e-15


def test_plane_system_floors_hold():
    """(b) of floor_ref's plane-prior docstring: the two references with plane priors on top, and the plane priors permuted."""
    import posegraph_prior_ref as pp
    import posegraph_se3 as se3
    for name in ["n1_xyz", "n2_free_mixed", "n7_pose_fixed", "n65_mixed"]:
        g, pr, fixed = pp.lin_case(name)
        n = len(g["init"])
        pl = F.make_planes(g, np.random.default_rng(7).integers(0, n, min(2 * n, 40)), 1)
        a, b = F.plane_system(g, pr, pl, oracle="c", fixed=fixed), F.plane_system(g, pr, pl, oracle="np", fixed=fixed)
        d = pp.differences(a, b)
        assert d["h"] <= se3.O2O_H and d["b"] <= se3.O2O_B and d["chi2"] <= se3.O2O_CHI2, (name, d)
        for r in range(4):
            c = F.plane_system(g, pr, F.planes_permuted(pl, np.random.default_rng(r).permutation(len(pl["vertex"]))), oracle="c", fixed=fixed)
            dd = pp.differences(c, a)
            assert dd["diag"] <= se3.SPREAD_H and dd["b"] <= se3.SPREAD_B and dd["chi2"] <= se3.SPREAD_CHI2, (name, dd)
        no_planes = pp.prior_system(g, pr, oracle="np", fixed=fixed)
        assert a["chi2"] > no_planes["chi2"] and np.abs(b["diag"] - no_planes["diag"]).max() > 0
