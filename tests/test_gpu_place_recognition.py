"""Loop candidates by appearance on the device (lslam_sc_*, csrc/lslam_sc.hip) against the numpy restatement
tests/place_recognition_ref.py: descriptors bit for bit, distances to the bound the header states, the selection as exact
conditions, the refusals, and the two consumers -- LoopDetector.detect_appearance and Graph(appearance_loops=True) -- on drives
whose drift is beyond the reference detector's radius."""
import numpy as np
import pytest

import place_recognition_ref as ref

pytestmark = pytest.mark.gpu

E4 = np.zeros((0, 4), np.float32)
SHAPES = [dict(n_ring=20, n_sector=60), dict(n_ring=7, n_sector=33, max_range=50.0, height_offset=1.5)]


def _consts(pkg):
    from importlib import import_module
    capi = import_module("the-cooper-mapper_amd.capi")
    return capi.SC_POINT_CHUNK, capi.SC_CAND_TILE


def _to_loam(c):
    o = c.copy()
    o[:, :3] = c[:, [1, 2, 0]]  # (x, y, z)_loam = (y, z, x)_world
    return o


def _clean(cloud, plist):
    for p in plist:
        cloud = ref.drop_ambiguous(cloud, p)
    return np.ascontiguousarray(cloud, np.float32)


def _rand(rng, n, span=60.0):
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = rng.uniform(-span, span, (n, 3))
    c[:, 2] = rng.uniform(-3.0, 8.0, n)
    return c


@pytest.fixture(scope="module")
def scan450(synth, small_problem):
    c, s, _ = synth.make_scan(small_problem["world"], 16, 450, gt_pose=(0, 0, 0.3, 3.0, -2.0, synth.SENSOR_HEIGHT), seed=11)
    return c, s


def _edge_keyframes(scan450, chunk):
    """(corner, surf) pairs in the z-up sensor frame, before the ambiguous points are dropped."""
    rng = np.random.default_rng(41)
    c, s = scan450
    far = _rand(rng, 300)
    far[:, 0] = rng.uniform(100.0, 200.0, 300)  # every point beyond any max_range used
    bad = _rand(rng, 64)
    bad[3, 0], bad[9, 1], bad[17, 2], bad[30, 0], bad[31, 1], bad[40, 2] = np.nan, np.nan, np.nan, np.inf, -np.inf, np.inf
    bad[50, :3] = np.nan
    centre = _rand(rng, 20)
    centre[4, :3] = (0.0, 0.0, 5.0)       # rho == 0
    centre[5, :3] = (1e-30, -1e-30, 5.0)  # rho underflows to 0
    low = _rand(rng, 40, span=20.0)
    low[:20, 2] = -2.0   # v == 0 at height_offset 2.0
    low[20:30, 2] = -1.5  # v == 0 at height_offset 1.5
    low[30:, 2] = -3.0
    dup = np.concatenate([s[:200], s[:200], s[100:150]])
    out = [(c, s), (E4, s), (E4, E4), (far[:100], far[100:]), (bad[:20], bad[20:]), (centre, E4), (low[:15], low[15:]), (c[:50], dup)]
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
        out.append((E4, _rand(rng, n)))
        out.append((_rand(rng, n), _rand(rng, 7)))
    return out


@pytest.mark.parametrize("up_axis", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["20x60", "7x33"])
def test_descriptors_bit_for_bit(pkg, ctx, scan450, shape, up_axis):
    chunk, _tile = _consts(pkg)
    p = ref.params(up_axis=up_axis, **shape)
    other = ref.params(up_axis=up_axis, **SHAPES[1 if shape is SHAPES[0] else 0])
    conv = _to_loam if up_axis == 1 else (lambda x: x)
    kfs = [(_clean(conv(c), (p, other)), _clean(conv(s), (p, other))) for c, s in _edge_keyframes(scan450, chunk)]
    store = pkg.KeyframeStore(ctx, slab_points=4096)
    try:
        assert not store.sc_info()["is_set"] and store.sc_info()["descriptor_bytes"] == 0
        store.sc_setup(**p)
        for c, s in kfs:
            store.add(c, s)
        for i, (c, s) in enumerate(kfs):
            D = store.sc_descriptor(i)
            want = ref.descriptor(c, s, p)
            assert D.shape == want.shape and D.tobytes() == want.tobytes(), "keyframe %d" % i
        assert ref.descriptor(*kfs[0], p).any() and not ref.descriptor(*kfs[2], p).any() and not ref.descriptor(*kfs[3], p).any()
        info = store.sc_info()
        assert info["describe_launches"] == 1 and info["n_described"] == len(kfs) and info["descriptor_bytes"] > 0
        assert all(info[k] == p[k] for k in ("n_ring", "n_sector", "up_axis")) and info["max_range"] == np.float32(p["max_range"])
        # a keyframe added after a query: the lazy describe picks it up, in one more launch
        store.sc_distances(0)
        assert store.sc_info()["describe_launches"] == 1
        late = (kfs[1][1][::3].copy(), kfs[0][1][::2].copy())
        lid = store.add(*late)
        d, _sh = store.sc_distances(0)
        assert len(d) == len(kfs) + 1 and store.sc_info()["describe_launches"] == 2 and store.sc_info()["n_described"] == len(kfs) + 1
        assert store.sc_descriptor(lid).tobytes() == ref.descriptor(*late, p).tobytes()
        # other parameters: the descriptors held are dropped and rebuilt as those of the new parameters
        store.sc_setup(**other)
        assert store.sc_info()["n_described"] == 0
        for i, (c, s) in enumerate(kfs + [late]):
            assert store.sc_descriptor(i).tobytes() == ref.descriptor(c, s, other).tobytes(), "keyframe %d, new parameters" % i
        assert store.sc_info()["describe_launches"] == 3
        # clear frees them; the parameters stay
        store.clear()
        assert store.sc_info()["descriptor_bytes"] == 0 and store.sc_info()["is_set"]
        store.add(*kfs[0])
        assert store.sc_descriptor(0).tobytes() == ref.descriptor(*kfs[0], other).tobytes()
    finally:
        store.close()


# ---- the 1 m-step square (the drive of test_graph_closes_the_loop_end_to_end, one lap) and four revisits ----------------------
REVISITS = [(5, 1.0, (0.4, 0.3)), (15, -2.0, (-0.7, 0.6)), (25, 3.0, (0.9, -0.9)), (35, 0.5, (0.2, -0.5))]  # (keyframe, yaw change, offset)


@pytest.fixture(scope="module")
def square(pkg, _session_ctx, synth, small_problem):
    world = small_problem["world"]
    p = ref.params(up_axis=2)
    xy = [(0.0, 0.0)]
    for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
        for _ in range(10):
            xy.append((xy[-1][0] + dx, xy[-1][1] + dy))
    xy = xy[:40]
    poses = [(0.0, 0.0, 0.3, x, y, synth.SENSOR_HEIGHT) for x, y in xy]
    for k, dyaw, (ox, oy) in REVISITS:
        poses.append((0.0, 0.0, 0.3 + dyaw, xy[k][0] + ox, xy[k][1] + oy, synth.SENSOR_HEIGHT))
    clouds = []
    for i, gt in enumerate(poses):
        c, s, _ = synth.make_scan(world, 16, 450, gt_pose=gt, seed=1000 + i)
        clouds.append((_clean(c, (p,)), _clean(s, (p,))))
    store = pkg.KeyframeStore(_session_ctx, slab_points=1 << 14)
    store.sc_setup(**p)
    for c, s in clouds:
        store.add(c, s)
    D = [ref.descriptor(c, s, p) for c, s in clouds]
    taps = {40 + r: store.sc_distances(40 + r) for r in range(4)}
    yield dict(store=store, p=p, D=D, xy=xy, poses=poses, taps=taps)
    store.close()


def test_distances_against_float64(square):
    store, p, D = square["store"], square["p"], square["D"]
    tol = ref.tol(p)
    assert abs(tol - 1.05e-5) < 1e-7
    for r, (k, dyaw, _off) in enumerate(REVISITS):
        q = 40 + r
        assert store.sc_descriptor(q).tobytes() == D[q].tobytes()
        d, sh = square["taps"][q]
        assert d.dtype == np.float32 and len(d) == 44 and ((sh >= 0) & (sh < p["n_sector"])).all()
        worst = [0.0, 0.0]
        for i in range(44):
            d64 = ref.shift_distances(D[q], D[i])
            worst = [max(worst[0], abs(float(d[i]) - d64[sh[i]])), max(worst[1], d64[sh[i]] - d64.min())]
        order = np.argsort(d[:40], kind="stable")
        print("revisit %d: |gpu - f64| max %.3g, f64(shift) - f64 min max %.3g (tol %.3g); nearest %s dist %s shift %d (yaw predicts %d)"
              % (r, worst[0], worst[1], tol, order[:3], d[order[:3]], sh[k], ref.yaw_shift(dyaw, p["n_sector"])))
        assert worst[0] <= tol and worst[1] <= 2 * tol
        assert abs(float(d[q])) <= tol and sh[q] == 0


def _check_list(lst, tap, eligible, top_k):
    """The selection's exact conditions for one query against the tap."""
    ids, sh, d = lst
    td, tsh = tap
    assert len(ids) == len(sh) == len(d) == min(top_k, eligible)
    assert ((ids >= 0) & (ids < eligible)).all() and len(set(ids.tolist())) == len(ids)
    assert d.tobytes() == td[ids].tobytes() and (sh == tsh[ids]).all()
    keys = [(float(d[i]), int(ids[i])) for i in range(len(ids))]
    assert keys == sorted(keys)
    if len(ids):
        inside = set(ids.tolist())
        for i in range(eligible):
            if i not in inside:
                assert (float(td[i]), i) > keys[-1]


def test_selection_is_exact(square):
    store, taps = square["store"], square["taps"]
    singles = []
    for q in range(40, 44):
        lst = store.sc_query([q], [39], 4)[0]
        _check_list(lst, taps[q], 40, 4)
        singles.append(lst)
        _check_list(store.sc_query([q], None, 32)[0], taps[q], q, 32)  # NULL limits: query id - 1
        _check_list(store.sc_query([q], [43], 32)[0], taps[q], 44, 32)  # the query itself is eligible then: first, at 0
    launches = store.sc_info()["query_launches"]
    batch = store.sc_query([40, 41, 42, 43], [39, 39, 39, 39], 4)
    assert store.sc_info()["query_launches"] == launches + 1
    for a, b in zip(batch, singles):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    again = store.sc_query([40, 41, 42, 43], [39, 39, 39, 39], 4)
    assert all(x.tobytes() == y.tobytes() for a, b in zip(batch, again) for x, y in zip(a, b))
    # limits: none, fewer eligible than top_k, a mix in one batch
    mixed = store.sc_query([43, 42, 41, 5], [-1, 2, 39, 0], 8)
    assert len(mixed[0][0]) == 0
    _check_list(mixed[1], taps[42], 3, 8)
    _check_list(mixed[2], taps[41], 40, 8)
    assert mixed[3][0].tolist() == [0]
    assert len(store.sc_query([0], None, 4)[0][0]) == 0  # keyframe 0 has no earlier keyframe


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_identical_clouds_tie_by_id_across_the_tile_edge(pkg, ctx, square, delta):
    _chunk, tile = _consts(pkg)
    n = tile + delta
    rng = np.random.default_rng(43)
    p = square["p"]
    three = [(_clean(_rand(rng, 150), (p,)), _clean(_rand(rng, 300), (p,))) for _ in range(3)]
    store = pkg.KeyframeStore(ctx, slab_points=1 << 14)
    try:
        store.sc_setup(**p)
        for i in range(n):
            store.add(*three[i % 3])
        q = n - 1
        d, sh = store.sc_distances(q)
        for i in range(n):  # the same pair of descriptors: the same bits, wherever the candidate sits
            assert d[i].tobytes() == d[i % 3].tobytes() and sh[i] == sh[i % 3]
        assert d[q] <= ref.tol(p) and sh[q] == 0
        for top_k in (1, 5, 32):
            _check_list(store.sc_query([q], None, top_k)[0], (d, sh), n - 1, top_k)
            _check_list(store.sc_query([q], [n - 1], top_k)[0], (d, sh), n, top_k)
        ids = store.sc_query([q], [n - 1], 32)[0][0]
        same = [i for i in range(n) if i % 3 == q % 3]
        assert ids.tolist()[:min(32, len(same))] == same[:32]  # distance 0 (the query's own cloud), ascending id
    finally:
        store.close()


def test_refusals_leave_the_store_usable(pkg, ctx, square):
    p = square["p"]
    rng = np.random.default_rng(44)
    store = pkg.KeyframeStore(ctx, slab_points=1 << 14)
    def refused(fn, word):
        with pytest.raises(pkg.LslamError) as e:
            fn()
        assert e.value.code == pkg.Status.ERR_INVALID and word in str(e.value), str(e.value)
    try:
        for _ in range(3):
            store.add(_rand(rng, 100), _rand(rng, 200))
        refused(lambda: store.sc_query([2], None, 2), "lslam_sc_setup")  # before setup
        refused(lambda: store.sc_distances(2), "lslam_sc_setup")
        for field, values in (("n_ring", (1, 33)), ("n_sector", (3, 129)), ("max_range", (0.0, -1.0, float("nan"), float("inf"))),
                              ("height_offset", (float("nan"),)), ("up_axis", (0, 3))):
            for v in values:
                refused(lambda: store.sc_setup(**{field: v}), field)
        assert not store.sc_info()["is_set"]
        store.sc_setup(**p)
        good = store.sc_query([2], None, 2)[0]
        refused(lambda: store.sc_setup(n_ring=40), "n_ring")
        refused(lambda: store.sc_query([3], None, 2), "out of range")
        refused(lambda: store.sc_query([-1], None, 2), "out of range")
        refused(lambda: store.sc_query([2], [3], 2), "out of range")
        refused(lambda: store.sc_descriptor(3), "out of range")
        refused(lambda: store.sc_distances(7), "out of range")
        refused(lambda: store.sc_query([2], None, 0), "top_k")
        refused(lambda: store.sc_query([2], None, 33), "top_k")
        after = store.sc_query([2], None, 2)[0]
        assert len(good[0]) == 2 and all(x.tobytes() == y.tobytes() for x, y in zip(good, after))
    finally:
        store.close()
    own = pkg.Context(0)
    st = pkg.KeyframeStore(own, slab_points=1 << 14)
    st.add(_rand(rng, 100), _rand(rng, 200))
    st.sc_setup(**p)
    own.close()
    for fn in (lambda: st.sc_setup(**p), lambda: st.sc_query([0], [0], 1), lambda: st.sc_distances(0), lambda: st.sc_descriptor(0),
               lambda: st.sc_info()):
        refused(fn, "its ctx was destroyed")
    st.close()


def appearance_scenario(pkg, synth, world, store):
    """The world and the first two keyframes of test_detect_nearest_closes_a_loop, five fillers that are real scans elsewhere,
    and a revisit whose estimate is 20 m off.  -> (keyframes, new keyframe, {id(kf): true pose}, true pose of the new one)"""
    def frame(pose6, seed, accum, drift=None):
        c, s, gt = synth.make_scan(world, 16, 900, gt_pose=pose6, seed=seed)
        R, t = synth.pose_to_Rt(gt)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        est = T.copy()
        if drift is not None:
            est[:3, 3] += drift
        kf = pkg.KeyFrame(est, accum, c, s)
        kf.put_in_store(store)
        return kf, T
    H = synth.SENSOR_HEIGHT
    k0, T0 = frame((0, 0, 0.30, 3.0, -2.0, H), 11, 0.0)
    k1, T1 = frame((0, 0, 0.32, 3.8, -2.2, H), 12, 1.0)
    fill = [frame((0, 0, 0.1 * i, x, y, H), 20 + i, 2.0 + i)[0] for i, (x, y) in
            enumerate(((20, 20), (-20, 20), (-25, -15), (15, -30), (30, 5)))]
    new, Tn = frame((0, 0, 1.35, 3.4, -1.8, H), 13, 60.0, drift=np.array([16.0, -12.0, 0.0]))
    return [k0, k1] + fill, new, {id(k0): T0, id(k1): T1}, Tn


def test_detect_appearance_closes_a_loop_detect_nearest_cannot(pkg, ctx, synth, small_problem):
    store = pkg.KeyframeStore(ctx)
    try:
        store.sc_setup(up_axis=2)  # synth's sensor frame
        kfs, new, truth_of, Tn = appearance_scenario(pkg, synth, small_problem["world"], store)
        det = pkg.LoopDetector(ctx=ctx)
        assert det.detect_nearest(kfs, [new]) == [] and det.get_loop_count() == 0
        ids, shifts, dists = det.appearance_candidates(kfs, new)
        print("candidates", ids, shifts, dists)
        loops = det.detect_appearance(kfs, [new])
        assert len(loops) == 1 and det.get_loop_count() == 1
        lp = loops[0]
        assert lp.key1 in kfs[:2] and lp.key2 is new
        listed = int(shifts[ids.tolist().index(lp.key1.store_id)])
        psi = 1.35 - (0.30, 0.32)[lp.key1.store_id]
        assert min((listed - ref.yaw_shift(psi, 60)) % 60, (ref.yaw_shift(psi, 60) - listed) % 60) <= 1
        truth = np.linalg.inv(truth_of[id(lp.key1)]) @ Tn
        err = np.abs(lp.relative_pose[:3, 3] - truth[:3, 3]).max()
        print("relative pose error %.4f m" % err)
        assert err < 0.05
        assert det.last_loop_accum_distance == 60.0
        # the interval rule: too little travel since that loop
        assert det.detect_appearance(kfs, [new]) == []
    finally:
        store.close()


def test_cpp_appearance_mirror_equals_python(pkg, ctx, synth, small_problem, tmp_path):
    """tests/cpp/appearance_loop_end_to_end.cpp on the scenario above: the C++ mirror's candidate list equals the Python mirror's
    bit for bit (ids, shifts, distances), its accepted loop has the same key1 and the same pose to 1e-6."""
    import subprocess
    from test_abi import _build_cpp
    exe = _build_cpp(pkg, tmp_path, "appearance_loop_end_to_end")
    store = pkg.KeyframeStore(ctx)
    try:
        store.sc_setup(up_axis=2)
        kfs, new, _truth, _Tn = appearance_scenario(pkg, synth, small_problem["world"], store)
        det = pkg.LoopDetector(ctx=ctx)
        ids, shifts, dists = det.appearance_candidates(kfs, new)
        loops = det.detect_appearance(kfs, [new])
        assert len(ids) == 4 and len(loops) == 1
        path = tmp_path / "keyframes.bin"
        with open(path, "wb") as fo:
            for k in kfs + [new]:
                fo.write(np.ascontiguousarray(k.estimate, np.float64).tobytes())
                fo.write(np.float64(k.accum_distance).tobytes())
                for a in (k.corner_cloud, k.surf_cloud):
                    fo.write(np.uint32(len(a)).tobytes())
                    fo.write(np.ascontiguousarray(a, np.float32).tobytes())
    finally:
        store.close()
    out = subprocess.run([str(exe), str(path), "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l for l in lines if l[0] == "NEAREST"] == [["NEAREST", "0"]]
    cand = [l for l in lines if l[0] == "CAND"]
    assert [int(l[1]) for l in cand] == ids.tolist() and [int(l[2]) for l in cand] == shifts.tolist()
    assert [int(l[3], 16) for l in cand] == dists.view(np.uint32).tolist()
    lp = [l for l in lines if l[0] == "LOOP"]
    assert len(lp) == 1 and int(lp[0][1]) == loops[0].key1.store_id
    pose = np.array([float(v) for v in lp[0][2:]]).reshape(4, 4)
    assert np.abs(pose - loops[0].relative_pose).max() <= 1e-6
    sc = [l for l in lines if l[0] == "SC"][0]
    assert (int(sc[1]), int(sc[2]), int(sc[3])) == (len(kfs) + 1, 1, 2)  # one describe; the list was asked for twice


def _drive(pkg, ctx, synth, world, appearance, scans):
    """The two-lap square of test_graph_closes_the_loop_end_to_end, the second lap driven at another sensor yaw, with a drift
    bias of 0.3 m per 1 m step.  A linear drift lets the estimated path cross itself -- and the reference's radius search then
    pairs places that are metres apart -- unless it outruns the square: with this bias and the detector's own
    accum_distance_thresh (30 m) no keyframe comes within 3.6 m of the estimate of an eligible earlier one (the search radius
    is sqrt(5) m), so whatever closes the loop found it by appearance."""
    rng = np.random.default_rng(5)
    P = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    g = pkg.Graph(ctx=ctx, resident=True, appearance_loops=appearance)
    way = [(dx, dy) for lap in range(2) for (dx, dy) in ((1, 0), (0, 1), (-1, 0), (0, -1)) for k in range(10)]
    x = y = 0.0
    drift = np.zeros(2)
    gts, odoms, n_loops = [], [], 0
    for step, (dx, dy) in enumerate([(0, 0)] + way):
        x += dx
        y += dy
        drift += rng.normal(0, 0.01, 2) + np.array([0.21, 0.21])
        yaw = 0.3 if step <= 40 else 1.3
        if step not in scans:  # (the two drives see the same scans: made once)
            scans[step] = synth.make_scan(world, 16, 450, gt_pose=(0.0, 0.0, yaw, x, y, synth.SENSOR_HEIGHT), seed=1000 + step)
        c, s, gtp = scans[step]
        R, t = synth.pose_to_Rt(gtp)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        O = T.copy()
        O[:2, 3] += drift
        T, O = P @ T @ P.T, P @ O @ P.T
        assert g.add_frame(O, _to_loam(c), _to_loam(s)) is not None
        gts.append(T)
        odoms.append(O)
        loops, _its = g.optimize(20)
        n_loops += len(loops)
    est = np.array([k.estimate[:3, 3] for k in g.keyframes])
    gt_xyz = np.array([T[:3, 3] for T in gts])
    od_xyz = np.array([O[:3, 3] for O in odoms])
    g.store.close()
    return n_loops, np.linalg.norm(est - gt_xyz, axis=1), np.linalg.norm(od_xyz - gt_xyz, axis=1)


def test_graph_with_appearance_loops_closes_a_drifted_lap(pkg, ctx, synth, small_problem):
    world = small_problem["world"]
    scans = {}
    n_off, _err_off, err_odo = _drive(pkg, ctx, synth, world, False, scans)
    assert err_odo[41:].min() > 3.0
    assert n_off == 0
    n_on, err_est, err_odo = _drive(pkg, ctx, synth, world, True, scans)
    print("loops %d, final error %.3f m (odometry %.3f m)" % (n_on, err_est[-1], err_odo[-1]))
    assert n_on >= 1 and err_est[-1] < 0.6 * err_odo[-1]
