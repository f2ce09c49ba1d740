"""Global re-localisation of the localisation node on the device (lslam_reloc_*, csrc/lslam_reloc_impl.hpp) against its numpy
restatement (tests/relocalization_ref.py) on the scene of tests/localization_ref.py: the occupancy sets, every hypothesis'
score as an integer, the selection with its tie rules, the refinement bit for bit against lslam_loc_match by hand, the whole
stage without an initial pose, ``apply``, lifetime and errors, and the C++ mirror."""
import os
import struct
import subprocess

import numpy as np
import pytest

import localization_ref as lr
import relocalization_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TOL_T, TOL_R = 1e-4, 1e-5  # the project's pose tolerances (tests/test_gpu_localization.py)
POS_TILE, CHUNK = 32, 1024  # LSLAM_RELOC_POS_TILE, LSLAM_RELOC_CHUNK: the scoring kernel's position tile and LDS chunk
VOXEL = 2.0


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def scene(synth):
    return lr.make_scene(synth)


@pytest.fixture(scope="module")
def ref(scene, oracle):
    r = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
    r.set_map(scene["map_corner"], scene["map_surf"], filter=False)
    return r


@pytest.fixture(scope="module")
def sets(ref):
    return rr.occupancy_sets(ref, VOXEL)


def _node(pkg, ctx, scene):
    node = pkg.LaserLocalization(ctx, *lr.DIMS)
    node.set_map(scene["map_corner"], scene["map_surf"], filter=False)
    return node


def _Rs(ctx, rot):
    return np.stack([ctx.pose_to_isometry(np.array([a[0], a[1], a[2], 0, 0, 0], F))[:3, :3] for a in np.asarray(rot, F).reshape(-1, 3)])


def _yaws(step_deg):
    out = np.zeros((int(round(360 / step_deg)), 3), F)
    out[:, 2] = np.deg2rad(np.arange(len(out)) * step_deg)
    return out


def _box(center, half, step, z=1.8):
    off = np.arange(-int(round(half / step)), int(round(half / step)) + 1) * step
    return np.array([[center[0] + dx, center[1] + dy, z] for dx in off for dy in off], F)


def _line_map():
    """~5 000 occupied voxels of 0.5 m packed along one line: consecutive keys, the worst clustering for a hash."""
    x = (np.arange(5000) * 0.5 - 1250.0 + 0.25).astype(F)
    surf = np.stack([x, np.full_like(x, 0.25), np.full_like(x, 0.25), np.zeros_like(x)], 1)
    return surf[::7].copy(), surf


@pytest.mark.parametrize("which_map", ["scene", "line"])
def test_occupancy_tap_equals_the_restatement(pkg, ctx, scene, ref, sets, oracle, which_map):
    if which_map == "scene":
        node, r, s, voxel = _node(pkg, ctx, scene), ref, sets, VOXEL
    else:
        mc, ms = _line_map()
        voxel = 0.5
        r = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
        r.set_map(mc, ms, filter=False)
        s = rr.occupancy_sets(r, voxel)
        assert len(s[1]) == 5000
        node = pkg.LaserLocalization(ctx, *lr.DIMS)
        node.set_map(mc, ms, filter=False)
    rng = np.random.default_rng(11)
    for t in range(2):
        pts = r.map[t][:, :3]
        lo, hi = pts.min(0) - 2 * voxel, pts.max(0) + 2 * voxel
        cand = rng.uniform(lo, hi, (4 * len(pts) + 64, 3)).astype(F)
        if which_map == "line":  # next to the line, where the probe sequences of a clustered table would run into each other
            cand[:, 1:] = rng.uniform(-1.0, 1.5, (len(cand), 2)).astype(F)
        empty = cand[rr.occupied(s, t, cand, voxel) == 0][:len(pts)]
        assert len(empty) == len(pts)
        odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [3e6, 0, 0], [-3e6, 1, 1]], F)  # points without a voxel
        q = np.concatenate([pts, empty, odd])
        got = node.reloc_occupied(t, q, voxel)
        want = rr.occupied(s, t, q, voxel)
        assert want[:len(pts)].all() and not want[len(pts):].any()
        assert np.array_equal(got, want), (which_map, t, int((got != want).sum()))
    info = node.reloc_info()
    assert info["occupied_voxels"] == (len(s[0]), len(s[1])) and info["valid"] == 1 and info["builds"] == 1 and info["voxel"] == F(voxel)
    node.reloc_occupied(0, q[:4], voxel)
    assert node.reloc_info()["builds"] == 1           # built once per map and voxel ...
    node.reloc_occupied(0, q[:4], 2 * voxel)
    assert node.reloc_info()["builds"] == 2           # ... and again when the voxel changes
    node.close()


def _first_k_filtered(ref, c, s, kc, ks):
    fc, fs = ref.prepare_frame(c, s)
    return fc[:kc].copy(), fs[:ks].copy()


def test_scores_equal_the_restatement_for_every_hypothesis(pkg, ctx, scene, ref, sets):
    node = _node(pkg, ctx, scene)
    c, s = scene["sweeps"][0]
    gt = scene["poses"][0]
    centre = (gt[3] + 0.37, gt[4] - 0.41)
    yaw45, yaw3 = _yaws(8.0), _yaws(8.0)[[2, 13, 40]]
    box9, box5 = _box(centre, 4.0, 1.0), _box(centre, 1.0, 1.0)[:5]
    none = np.zeros((0, 4), F)
    def counts(kc, ks):
        return lambda n, want, res: n == (kc, ks)

    def subsampled(n, want, res):
        exp = tuple(v if v <= 500 else -(-v // -(-v // 500)) for v in n)
        return max(n) > 500 and res.n_scored == exp and max(exp) <= 500

    cases = [("scene 45 x 9 x 9", c, s, yaw45, box9, {}, lambda n, want, res: sum(n) == 3274 and sum(n) > CHUNK)]
    for k in (63, 64, 65):
        kc, ks = _first_k_filtered(ref, c, s, k, k)
        cases.append(("P = %d per type" % k, kc, ks, yaw3, box5, {}, counts(k, k)))
    one_c, _ = _first_k_filtered(ref, c, s, 1, 0)
    cases.append(("P = 1", one_c, none, yaw3, box5, {}, counts(1, 0)))
    cases.append(("empty corner cloud", none, s, yaw3, box5, {}, lambda n, want, res: n[0] == 0 and n[1] > 0))
    cases.append(("n_rot = 1", c, s, yaw3[:1], box9, {}, None))
    cases.append(("n_pos = 1", c, s, yaw45, box9[40:41], {}, None))
    cases.append(("n_pos = tile + 1", c, s, yaw3[:2], _box(centre, 3.0, 1.0)[:POS_TILE + 1], {}, None))
    kc, ks = _first_k_filtered(ref, c, s, 100, CHUNK + 1 - 100)
    cases.append(("P = chunk + 1", kc, ks, yaw3, box5, {}, lambda n, want, res: sum(n) == CHUNK + 1))
    cases.append(("max_points 500", c, s, yaw3, box5, dict(max_points=500), subsampled))
    outside = np.array([[2000.0, 2000.0, 1.8], [-2200.0, 1500.0, 1.8]], F)
    cases.append(("outside the map", c, s, yaw3, outside, {}, lambda n, want, res: not want.any()))
    edge = np.array([[centre[0], centre[1], 1.8], [2876.0, 0.0, 1.8], [0.0, -2900.0, 1.8], [0.0, 0.0, 130.0], [2874.0, 0.0, 1.8]], F)
    cases.append(("the refused edge band", c, s, yaw3, edge, {},
                  lambda n, want, res: (want[:, 1:4] == -1).all() and (want[:, 0] > 0).all() and (want[:, 4] == 0).all() and res.skipped == 9))
    for name, cc, ss, rot, pos, kw, check in cases:
        want, n = rr.scores(ref, cc, ss, _Rs(ctx, rot), pos, VOXEL, kw.get("max_points", 0), sets=sets)
        got, _, _, res = node.reloc_scores(cc, ss, rot, pos, voxel=VOXEL, **kw)
        print("%s: %d hypotheses, %d + %d points, best %d, %d differ" % (name, want.size, n[0], n[1], want.max(), int((got != want).sum())))
        assert got.dtype == np.int32 and np.array_equal(got, want), name
        assert res.n_points == n and res.n_hypotheses == want.size and res.skipped == int((want < 0).sum()), name
        assert check is None or check(n, want, res), name
    node.close()


def _periodic_case():
    """A map that repeats every 4 m in x (every second 2 m voxel column is occupied) and a scan of a few points: only a handful
    of distinct scores over 16 384 hypotheses, so the cut of the top list falls inside long runs of equal scores."""
    i, j = np.meshgrid(np.arange(-40, 41), np.arange(-80, 81), indexing="ij")
    surf = np.stack([4.0 * i.ravel() + 1.0, 2.0 * j.ravel() + 1.0, np.full(i.size, 1.0), np.zeros(i.size)], 1).astype(F)
    corner = surf[::50].copy()
    scan_s = np.array([[0.3, 0.2, 1.0, 0], [5.1, 3.0, 1.0, 0], [10.2, -7.0, 1.0, 0], [-8.4, 2.2, 1.0, 0], [3.3, -12.5, 1.0, 0]], F)
    scan_c = np.array([[1.0, 1.0, 1.0, 0]], F)
    pos = np.array([[0.5 * a - 16.0, 0.5 * b - 16.0, 0.0] for a in range(64) for b in range(64)], F)
    return corner, surf, scan_c, scan_s, _yaws(90.0), pos


def test_selection_equals_the_restatement_under_ties(pkg, ctx, oracle):
    corner, surf, scan_c, scan_s, rot, pos = _periodic_case()
    r = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
    r.set_map(corner, surf, filter=False)
    node = pkg.LaserLocalization(ctx, *lr.DIMS)
    node.set_map(corner, surf, filter=False)
    want, _ = rr.scores(r, scan_c, scan_s, _Rs(ctx, rot), pos, VOXEL)
    values, counts = np.unique(want, return_counts=True)
    print("scores", dict(zip(values.tolist(), counts.tolist())))
    assert len(values) <= 7 and counts.max() > 1024
    for top_m, sub in ((0, slice(None)), (1024, slice(None)), (100, slice(None)), (256, slice(0, 50)), (1, slice(None))):
        p = pos[sub]
        w = want[:, sub]
        got, ti, ts, res = node.reloc_scores(scan_c, scan_s, rot, p, voxel=VOXEL, top_m=top_m)
        assert np.array_equal(got, w)
        wi, ws = rr.top_m(w, top_m or 256)
        assert res.n_selected == len(wi) == len(ti) and np.array_equal(ti, wi) and np.array_equal(ts, ws), top_m
        for kw in (dict(nms_m=1.0, nms_rot=1, rot_cyclic=1, max_candidates=16), dict(nms_m=3.0, nms_rot=-1, rot_cyclic=0, max_candidates=64), {}):
            keep = node.reloc_nms(ti, rot, p, **kw)
            wk = rr.nms(wi, p, len(rot), kw.get("nms_m", 2.0), {0: 2, -1: 0}.get(kw.get("nms_rot", 0), kw.get("nms_rot", 0)),
                        bool(kw.get("rot_cyclic", 0)), kw.get("max_candidates", 8))
            assert np.array_equal(keep, wk), (top_m, kw)
    # the candidates of the full call are the survivors, in rank order
    res = node.relocalize(scan_c, scan_s, rot, pos, voxel=VOXEL, top_m=1024, nms_m=1.0, nms_rot=1, rot_cyclic=1, max_candidates=16, refine_rounds=1)
    wi, ws = rr.top_m(want, 1024)
    wk = rr.nms(wi, pos, len(rot), 1.0, 1, True, 16)
    assert [c.hypothesis for c in res.candidates] == wi[wk].tolist() and [c.coarse_score for c in res.candidates] == ws[wk].tolist()
    node.close()


def _check_candidate(pkg, node, c, s, cd, rot, pos, ran):
    """The candidate against lslam_loc_match called by hand from the same Twist, as often: every bit of pose and counters."""
    pose = np.concatenate([rot[cd.hypothesis // len(pos)], pos[cd.hypothesis % len(pos)]]).astype(F)
    status, k, st = pkg.Status.NOT_CONVERGED, 0, None
    while k < 3 and status == pkg.Status.NOT_CONVERGED:
        status, pose, st = node.match(c, s, pose)
        k += 1
    assert (cd.status, cd.rounds, cd.n_rows) == (status, k, st.n_rows), cd
    assert np.array_equal(bits(cd.pose), bits(pose)), cd
    ran.add(k)


def test_refinement_equals_matches_by_hand(pkg, ctx, scene, ref):
    node = _node(pkg, ctx, scene)
    c, s = scene["sweeps"][0]
    gt = np.asarray(scene["poses"][0], np.float64)
    rot = np.array([[0, 0, gt[2] + a] for a in np.deg2rad([-6.0, 1.0, 8.0, 91.0])], F)
    pos = _box((gt[3] + 0.25, gt[4] + 0.25), 0.5, 0.5)
    res = node.relocalize(c, s, rot, pos, voxel=VOXEL, nms_m=0.4, nms_rot=-1, max_candidates=6, refine_rounds=3)
    assert len(res.candidates) == 6 and res.winner >= 0
    # hypotheses far from the truth as well: their first match runs out of iterations and is repeated from its own result
    far_rot = np.array([[0, 0, gt[2] + a] for a in np.deg2rad([-27.0, 25.0])], F)
    far_pos = _box((gt[3] + 2.5, gt[4] + 2.5), 0.5, 0.5)
    far = node.relocalize(c, s, far_rot, far_pos, voxel=VOXEL, nms_m=0.4, nms_rot=-1, max_candidates=6, refine_rounds=3)
    ran = set()
    for res_k, rot_k, pos_k in ((res, rot, pos), (far, far_rot, far_pos)):
        for cd in res_k.candidates:
            _check_candidate(pkg, node, c, s, cd, rot_k, pos_k, ran)
    print("rounds run per candidate:", sorted(ran), "statuses:", [cd.status for cd in res.candidates + far.candidates])
    assert max(ran) > 1
    w = res.candidates[res.winner]
    ok = [i for i, cd in enumerate(res.candidates) if cd.status == 0]
    assert res.winner == max(ok, key=lambda i: (res.candidates[i].n_rows, -i))
    hyp = np.concatenate([rot[w.hypothesis // len(pos)], pos[w.hypothesis % len(pos)]]).astype(F)
    rs, rp, rn, rk = rr.refine(ref, c, s, hyp, 3)
    dt, dr = np.abs(w.pose[3:] - rp[3:]).max(), np.abs(w.pose[:3] - rp[:3]).max()
    print("winner against the restatement: |dt| %.2e m |dr| %.2e rad, rows %d / %d" % (dt, dr, w.n_rows, rn))
    assert (rs, rk) == (w.status, w.rounds) and dt <= TOL_T and dr <= TOL_R
    assert np.array_equal(bits(res.T), bits(ctx.pose_to_isometry(w.pose)))
    node.close()


def _end_to_end_inputs(scene):
    gt = np.asarray(scene["poses"][0], np.float64)
    pos = _box((gt[3] + 0.25, gt[4] + 0.25), 4.0, 0.5)
    assert np.hypot(*(pos[:, :2] - gt[3:5]).T).min() >= 0.35
    return gt, _yaws(2.0), pos


def _yaw_of(ctx, pose):
    T = ctx.pose_to_isometry(np.asarray(pose, F))
    return np.arctan2(T[1, 0], T[0, 0])


def test_end_to_end_without_an_initial_pose(pkg, ctx, scene):
    node = _node(pkg, ctx, scene)
    c, s = scene["sweeps"][0]
    gt, rot, pos = _end_to_end_inputs(scene)
    assert node.process(c, s, np.eye(4, dtype=F), 1_000_000_000) is None and node.last_flags & 1
    res = node.relocalize(c, s, rot, pos, voxel=VOXEL, rot_cyclic=1)
    w = res.candidates[res.winner]
    coarse = np.concatenate([rot[w.hypothesis // len(pos)], pos[w.hypothesis % len(pos)]])
    err_c = np.hypot(*(coarse[3:5] - gt[3:5]))
    err_t, err_z = np.hypot(*(w.pose[3:5] - gt[3:5])), abs(w.pose[5] - gt[5])
    err_yaw = abs((_yaw_of(ctx, w.pose) - gt[2] + np.pi) % (2 * np.pi) - np.pi)
    print("%d hypotheses (%d skipped), %d points, coarse %.1f ms, refine %.1f ms, %d candidates" %
          (res.n_hypotheses, res.skipped, sum(res.n_points), res.ms_coarse, res.ms_refine, len(res.candidates)))
    print("winner: coarse score %d at %.3f m from the truth -> refined %.4f m (z %.4f m, yaw %.5f rad), fraction %.3f, rows %d" %
          (w.coarse_score, err_c, err_t, err_z, err_yaw, res.fraction, w.n_rows))
    assert res.status == 0 and res.accepted and sum(res.n_points) == 3274 and res.n_hypotheses == 180 * 289
    assert err_c >= 0.35 and np.sqrt(err_t ** 2 + err_z ** 2) <= 0.1
    assert res.fraction == F(w.n_rows) / F(3274) and res.fraction >= 0.4
    if res.runner_up >= 0:  # the world is square: only a quarter-turn alias may stand beside the winner
        ru = res.candidates[res.runner_up]
        d = np.rad2deg(_yaw_of(ctx, ru.pose) - _yaw_of(ctx, w.pose)) % 360.0
        print("runner-up: yaw %.1f deg from the winner's, rows %d" % (d, ru.n_rows))
        assert min(abs(d - q) for q in (90.0, 180.0, 270.0)) <= 5.0
        assert np.abs(ru.pose[3:] - w.pose[3:]).max() > 2.0
    assert node.process(c, s, np.eye(4, dtype=F), 1_200_000_000) is None  # apply was not asked for
    node.close()


def test_apply_hands_the_pose_to_the_node(pkg, ctx, scene):
    c, s = scene["sweeps"][0]
    gt, _, _ = _end_to_end_inputs(scene)
    rot = np.array([[0, 0, gt[2] + a] for a in np.deg2rad(np.arange(-8.0, 9.0, 2.0) + 0.7)], F)
    pos = _box((gt[3] + 0.25, gt[4] + 0.25), 1.0, 0.5)
    node = _node(pkg, ctx, scene)
    assert node.process(c, s, np.eye(4, dtype=F), 1_000_000_000) is None and node.last_flags & 1
    before = node.info()
    res = node.relocalize(c, s, rot, pos, voxel=VOXEL, apply=0)
    assert res.accepted and res.status == 0
    assert node.info() == before and node.process(c, s, np.eye(4, dtype=F), 1_000_000_000) is None
    rej = node.relocalize(c, s, rot, pos, voxel=VOXEL, apply=1, min_fraction=1.1)
    assert not rej.accepted and rej.status == pkg.Status.TOO_FEW_MATCHES and rej.winner == res.winner
    assert np.array_equal(bits(rej.T), bits(res.T)) and rej.fraction == res.fraction
    assert node.info() == before and node.process(c, s, np.eye(4, dtype=F), 1_000_000_000) is None
    assert node.reloc_info()["builds"] == 1 and node.reloc_info()["occupied_voxels"] == res.occupied_voxels
    res1 = node.relocalize(c, s, rot, pos, voxel=VOXEL, apply=1)
    assert res1.accepted and np.array_equal(bits(res1.T), bits(res.T))
    other = _node(pkg, ctx, scene)
    other.handle_initial_pose(res.T)
    for k, (ck, sk) in enumerate(scene["sweeps"]):
        odom = ctx.pose_to_isometry(np.asarray(scene["poses"][k], F))
        Ta = node.process(ck, sk, odom, 1_000_000_000 + k * 200_000_000)
        Tb = other.process(ck, sk, odom, 1_000_000_000 + k * 200_000_000)
        assert Ta is not None and np.array_equal(bits(Ta), bits(Tb)) and node.last_flags == other.last_flags, k
        assert node.last_stats.n_rows == other.last_stats.n_rows and node.last_stats.iterations == other.last_stats.iterations
    err = np.abs(Ta[:3, 3] - np.asarray(scene["poses"][3][3:])).max()
    print("after the run: %.4f m from the ground truth of the last sweep" % err)
    assert err <= 0.1
    node.close()
    other.close()


def test_lifetime_and_errors(pkg, ctx, scene, ref, sets, oracle, tmp_path):
    c, s = scene["sweeps"][0]
    gt = scene["poses"][0]
    rot, pos = _yaws(90.0), _box((gt[3], gt[4]), 1.0, 1.0)
    INVALID = pkg.Status.ERR_INVALID

    def refused(node, *a, **kw):
        with pytest.raises(pkg.LslamError) as e:
            node.relocalize(*a, **kw)
        assert e.value.code == INVALID, e.value
        return str(e.value)

    (tmp_path / "index2.txt").write_text("")
    paged = pkg.LaserLocalization(ctx, *lr.DIMS, dynamic_mode=True, files_directory=str(tmp_path))
    assert "paged" in refused(paged, c, s, rot, pos)
    with pytest.raises(pkg.LslamError):
        paged.reloc_occupied(0, pos)
    paged.close()
    for _ in range(2):  # create and destroy twice in one process
        node = pkg.LaserLocalization(ctx, *lr.DIMS)
        assert "no map" in refused(node, c, s, rot, pos)
        assert node.reloc_info()["valid"] == 0
        node.set_map(scene["map_corner"], scene["map_surf"], filter=False)
        assert "hypotheses" in refused(node, c, s, np.zeros((4097, 3), F), pos)
        assert "hypotheses" in refused(node, c, s, np.zeros((4096, 3), F), np.zeros((16385, 3), F))
        refused(node, c, s, rot, pos, top_m=1025)
        refused(node, c, s, rot, pos, max_candidates=65)
        refused(node, c, s, rot, pos, voxel=-1.0)
        got, _, _, res = node.reloc_scores(c, s, rot, pos, voxel=VOXEL)
        want, _ = rr.scores(ref, c, s, _Rs(ctx, rot), pos, VOXEL, sets=sets)
        assert np.array_equal(got, want) and res.occupied_voxels == (len(sets[0]), len(sets[1]))
        # another map between two calls: the sets are rebuilt
        half_c, half_s = scene["map_corner"][::2], scene["map_surf"][scene["map_surf"][:, 0] < 10.0]
        node.set_map(half_c, half_s, filter=False)
        assert node.reloc_info()["valid"] == 0
        r2 = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
        r2.set_map(half_c, half_s, filter=False)
        s2 = rr.occupancy_sets(r2, VOXEL)
        got2, _, _, res2 = node.reloc_scores(c, s, rot, pos, voxel=VOXEL)
        want2, _ = rr.scores(r2, c, s, _Rs(ctx, rot), pos, VOXEL, sets=s2)
        assert np.array_equal(got2, want2) and not np.array_equal(want2, want)
        assert res2.occupied_voxels == (len(s2[0]), len(s2[1])) != res.occupied_voxels and node.reloc_info()["builds"] == 2
        node.close()


def test_cpp_mirror_relocalises(pkg, ctx, scene, tmp_path):
    """tests/cpp/relocalization_end_to_end.cpp: no pose, a dropped sweep, relocalize(apply), one processed sweep."""
    c, s = scene["sweeps"][0]
    gt, _, _ = _end_to_end_inputs(scene)
    rot = np.array([[0, 0, gt[2] + a] for a in np.deg2rad(np.arange(-8.0, 9.0, 2.0) + 0.7)], F)
    pos = _box((gt[3] + 0.25, gt[4] + 0.25), 1.0, 0.5)
    data = tmp_path / "reloc.bin"
    with open(data, "wb") as f:
        for a in (scene["map_corner"], scene["map_surf"], c, s, rot, pos):
            a = np.ascontiguousarray(a, F)
            f.write(struct.pack("<I", a.size))
            f.write(a.tobytes())
    exe = tmp_path / "relocalization_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "relocalization_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), str(data)] + [str(d) for d in lr.DIMS] + [str(VOXEL), "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines()}
    node = _node(pkg, ctx, scene)
    res = node.relocalize(c, s, rot, pos, voxel=VOXEL, apply=1)
    T = node.process(c, s, np.eye(4, dtype=F), 1_200_000_000)
    rl = lines["RELOC"]
    assert [int(v) for v in rl[:4]] == [1, res.winner, res.runner_up, len(res.candidates)]
    assert np.array_equal(bits([float.fromhex(v) for v in rl[4:5]]), bits([res.fraction]))
    assert np.array_equal(bits([float.fromhex(v) for v in rl[5:21]]), bits(res.T.ravel()))
    sw = lines["SWEEP"]
    assert int(sw[0]) == node.last_flags and np.array_equal(bits([float.fromhex(v) for v in sw[1:17]]), bits(T.ravel()))
    assert np.array_equal(bits(T), bits(res.T))  # the first sweep after the hand-over takes the pose
    node.close()
