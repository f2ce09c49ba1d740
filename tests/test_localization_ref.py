"""CPU checks of the localisation node's restatement (tests/localization_ref.py): the reset-after-match quirk, the velocity
rule, the dropped sweep before initialisation, transformMerge against float64, and convergence on the test scene."""
import numpy as np
import pytest

import localization_ref as lr


@pytest.fixture(scope="module")
def scene(synth):
    return lr.make_scene(synth)


def _ref(oracle, scene, filter=False):
    ref = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
    ref.set_map(scene["map_corner"], scene["map_surf"], filter=filter)
    return ref


def test_scene_is_the_one_the_issue_describes(scene, oracle):
    assert (len(scene["map_corner"]), len(scene["map_surf"])) == (3177, 181104)
    ref = _ref(oracle, scene, filter=True)
    assert (len(ref.map[0]), len(ref.map[1])) == (1481, 41611)
    assert len(ref.cubes[1]) == 9  # the map spans nine cubes


def test_transform_merge_matches_float64():
    rng = np.random.default_rng(3)

    def iso():
        a = rng.uniform(-1, 1, 3)
        cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, rng.uniform(-10, 10, 3)
        return T.astype(np.float32)
    for _ in range(10):
        Lo, Ln, Wo = iso(), iso(), iso()
        W = lr.transform_associate(Lo, Ln, Wo)
        ref = Wo.astype(np.float64) @ np.linalg.inv(Lo.astype(np.float64)) @ Ln.astype(np.float64)
        assert np.abs(W - ref).max() < 2e-5 and np.array_equal(W[3], [0, 0, 0, 1])
    I = np.eye(4, dtype=np.float32)
    assert np.array_equal(lr.transform_associate(I, I, Wo), Wo)  # identity odometry leaves the pose as it is, bit for bit


def test_cube_index_is_round_half_away_from_zero():
    p = np.array([[25.0, -25.0, 24.99, 0], [-75.0, 74.9, -0.1, 0]], np.float32)
    assert lr.cube_index(p, 50.0, (60, 60, 5)).tolist() == [[61, 59, 5], [58, 61, 5]]


def test_a_sweep_before_the_initial_pose_is_dropped(scene, oracle):
    ref = _ref(oracle, scene)
    c, s = scene["sweeps"][0]
    T, flags = ref.process(c, s, np.eye(4, dtype=np.float32), 1_000_000_000)
    assert T is None and flags == lr.DROPPED
    assert ref.stamp_last == 0 and np.array_equal(ref.mapped_last, np.eye(4)) and ref.last is None


def test_reset_quirk_velocity_rule_and_convergence(scene, oracle):
    """The first sweep's match result is discarded for the pending pose (and no velocity yet); the later sweeps converge to the
    ground truth from the perturbed start; a jump of more than 30 m/s is zeroed."""
    ref = _ref(oracle, scene)
    run = lr.run_trajectory(ref, scene, ref.pose_to_isometry)
    T0, v0, f0 = run[0]
    assert f0 == lr.POSE_RESET and v0 is None
    assert np.array_equal(T0, ref.pose_to_isometry(scene["start"]))  # the reset pose exactly: the match result is gone
    for k in (1, 2, 3):
        T, v, f = run[k]
        gt = np.asarray(scene["poses"][k], np.float64)
        assert f == lr.HAS_VELOCITY
        err_t = np.abs(T[:3, 3] - gt[3:]).max()
        print("sweep %d: |t - gt| %.4f m" % (k, err_t))
        assert err_t < 0.03
        prev = run[k - 1][0]
        assert np.allclose(v, (T[:3, 3] - prev[:3, 3]) / np.float32(0.2), rtol=1e-6, atol=1e-6)
    assert np.abs(run[3][0][:3, 3] - np.asarray(scene["poses"][3][3:])).max() < 0.005
    # the > 30 rule: the same sweep again 1 ms later after a pending pose 1 m away -> 1000 m/s -> zero
    far = run[3][0].copy()
    far[0, 3] += 1.0
    ref.handle_initial_pose(far)
    c, s = scene["sweeps"][3]
    T, flags = ref.process(c, s, ref.odom_last, ref.stamp_last + 1_000_000)
    assert flags == lr.POSE_RESET | lr.HAS_VELOCITY | lr.VELOCITY_ZEROED
    assert np.array_equal(T, far) and np.array_equal(ref.velocity, np.zeros(3, np.float32))


def test_filtered_map_converges(scene, oracle):
    ref = _ref(oracle, scene, filter=True)
    run = lr.run_trajectory(ref, scene, ref.pose_to_isometry)
    err = np.abs(run[3][0][:3, 3] - np.asarray(scene["poses"][3][3:])).max()
    print("filtered map: final |t - gt| %.4f m" % err)
    assert err < 0.05
