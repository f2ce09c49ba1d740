"""Visibility votes on the device (lslam_vis_*, csrc/lslam_vis.hip) against the numpy restatement tests/visibility_ref.py:
range images bit for bit, votes count for count, additivity over voters, the stable filter, vis_add_to_fmap against
lslam_kfs_add_to_fmap, the refusals, and the scene of a box that is there for two keyframes of six -- through the votes and
through Graph(remove_dynamic=True).

Where two correct fp64 atan2 implementations may choose different bins (a rowd or scaled azimuth within 1e-9 of an integer) a
point is left out of the comparison (visibility_ref.unambiguous); every test that does so asserts that this is at most 1 % of
its points."""
import numpy as np
import pytest

import visibility_ref as V

pytestmark = pytest.mark.gpu

E4 = np.zeros((0, 4), np.float32)
SHAPES = [dict(), dict(n_row=7, n_col=33, fov_down_deg=-20.0, fov_up_deg=10.0, min_range=0.5, max_range=50.0)]
# five general SE(3) poses (rx, ry, rz, x, y, z) a few metres apart, and further ones for voters that repeat a keyframe
POSES6 = [(0.03, -0.02, 0.3, 3.0, -2.0, 1.8), (-0.05, 0.04, 1.2, 5.5, -1.0, 1.9), (0.02, 0.06, -0.7, 4.0, 1.5, 1.7),
          (0.08, -0.03, 2.6, 1.0, -3.5, 1.85), (-0.04, -0.05, -2.1, 6.0, -4.0, 1.75)]


def _consts(pkg):
    return pkg.visibility.POINT_TILE, pkg.visibility.KF_CHUNK


def _to_loam(c):
    o = np.array(c, np.float32)
    o[:, :3] = np.asarray(c)[:, [1, 2, 0]]  # (x, y, z)_loam = (y, z, x)_world
    return o


def _rand(rng, n, span=60.0):
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = rng.uniform(-span, span, (n, 3))
    c[:, 2] = rng.uniform(-3.0, 8.0, n)
    return c


def _pose(p6):
    return V.pose_matrix(np.asarray(p6, np.float64)).astype(np.float32)


@pytest.fixture(scope="module")
def scans(synth, small_problem):
    """One 16 x 450 scan per pose of POSES6, in the z-up sensor frame."""
    out = []
    for i, p6 in enumerate(POSES6):
        c, s, _ = synth.make_scan(small_problem["world"], 16, 450, gt_pose=p6, seed=70 + i)
        out.append((c, s))
    return out


def _image_keyframes(scans, tile):
    rng = np.random.default_rng(5)
    c, s = scans[0]
    bad = _rand(rng, 64, span=20.0)
    bad[3, 0], bad[9, 1], bad[17, 2], bad[30, 0], bad[31, 1], bad[40, 2] = np.nan, np.nan, np.nan, np.inf, -np.inf, np.inf
    bad[50, :3] = np.nan
    bad[51, :3] = (1e30, 1e30, 0.0)        # r overflows to inf: outside the gate
    bad[52, :3] = (0.0, 0.0, 5.0)          # straight up: rho == 0, above the field of view
    bad[53, :3] = (0.3, 0.2, 0.1)          # inside min_range
    far = _rand(rng, 100)
    far[:, 0] = rng.uniform(100.0, 200.0, 100)  # beyond any max_range used
    out = [(c[:400], s[:2600]), (E4, E4), (bad[:20], bad[20:]), (far[:1], far[1:])]
    for n in (1, tile - 1, tile, tile + 1):
        out.append((E4, _rand(rng, n, span=30.0)))
        out.append((_rand(rng, n, span=30.0), _rand(rng, 7, span=30.0)))
    return out


@pytest.mark.parametrize("up_axis", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["16x360", "7x33"])
def test_range_images_bit_for_bit(pkg, ctx, scans, shape, up_axis):
    tile, _chunk = _consts(pkg)
    p = V.params(up_axis=up_axis, **shape)
    other = V.params(up_axis=up_axis, **SHAPES[1 if shape is SHAPES[0] else 0])
    conv = _to_loam if up_axis == 1 else (lambda x: np.array(x, np.float32))
    kfs, total, dropped = [], 0, 0
    for c, s in _image_keyframes(scans, tile):
        pair = []
        for cloud in (conv(c), conv(s)):
            keep = V.unambiguous(cloud, None, p) & V.unambiguous(cloud, None, other)
            total, dropped = total + len(cloud), dropped + int((~keep).sum())
            pair.append(np.ascontiguousarray(cloud[keep]))
        kfs.append(tuple(pair))
    assert dropped <= 0.01 * total
    store = pkg.KeyframeStore(ctx, slab_points=4096)
    try:
        assert not store.vis_info()["is_set"] and store.vis_info()["image_bytes"] == 0
        store.vis_setup(**p)
        assert store.vis_info()["image_bytes"] == 0  # nothing is allocated before an image is needed
        for c, s in kfs:
            store.add(c, s)
        for i, (c, s) in enumerate(kfs):
            img, want = store.vis_range_image(i), V.range_image(c, s, p)
            assert img.shape == want.shape and img.tobytes() == want.tobytes(), "keyframe %d" % i
        assert np.isfinite(V.range_image(*kfs[0], p)).sum() > 100 and np.isinf(V.range_image(*kfs[1], p)).all()
        assert np.isinf(V.range_image(*kfs[3], p)).all()
        info = store.vis_info()
        assert info["image_launches"] == 1 and info["n_images"] == len(kfs) and info["image_bytes"] > 0  # all in one lazy launch
        assert all(info[k] == p[k] for k in ("n_row", "n_col", "window", "up_axis")) and info["max_range"] == np.float32(p["max_range"])
        # a keyframe added later: the lazy build picks it up, in one more launch
        late = (kfs[0][1][::3].copy(), kfs[0][0][::2].copy())
        lid = store.add(*late)
        assert store.vis_range_image(lid).tobytes() == V.range_image(*late, p).tobytes()
        assert store.vis_info()["image_launches"] == 2 and store.vis_info()["n_images"] == len(kfs) + 1
        # other parameters: the images held are dropped and rebuilt as those of the new parameters
        store.vis_setup(**other)
        assert store.vis_info()["n_images"] == 0 and store.vis_info()["image_bytes"] == 0
        for i, (c, s) in enumerate(kfs + [late]):
            assert store.vis_range_image(i).tobytes() == V.range_image(c, s, other).tobytes(), "keyframe %d, new parameters" % i
        assert store.vis_info()["image_launches"] == 3
        # clear frees them; the parameters stay
        store.clear()
        assert store.vis_info()["image_bytes"] == 0 and store.vis_info()["is_set"]
        store.add(*kfs[0])
        assert store.vis_range_image(0).tobytes() == V.range_image(*kfs[0], other).tobytes()
    finally:
        store.close()


def _edge_points(T0, p):
    """Points built to sit in column 0 and n_col - 1 and in the first and last row of the keyframe at T0 (z up)."""
    step_c, step_r = 360.0 / p["n_col"], (p["fov_up_deg"] - p["fov_down_deg"]) / p["n_row"]
    out = []
    for az in (0.5 * step_c, 360.0 - 0.5 * step_c):
        for el in (p["fov_down_deg"] + 0.5 * step_r, p["fov_up_deg"] - 0.5 * step_r, 0.3):
            for r in (4.0, 9.0, 25.0):
                a, e = np.deg2rad(az), np.deg2rad(el)
                out.append((r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e)))
    return V.transform(T0, np.array(out, np.float32))


def five_data(scans, tile):
    """The host side of the `five` fixture: poses, reference images and ~3000 query points in the graph frame -- returns of every
    keyframe (hits), the same pulled towards their sensor (free space), pushed behind (occluded), far away, non-finite, and the
    edge points of keyframe 0, which come first."""
    p = V.params(up_axis=2)
    poses = [_pose(p6) for p6 in POSES6]
    rng = np.random.default_rng(9)
    parts = []
    for (c, s), T in zip(scans, poses):
        pick = s[rng.choice(len(s), 180, replace=False), :3]
        for scale in (1.0, 0.5, 0.8, 1.3):
            parts.append(V.transform(T, (pick[:160] * np.float32(scale)).astype(np.float32)))
    edge = _edge_points(poses[0], p)
    parts.append(edge)
    parts.append(rng.uniform(-250.0, 250.0, (60, 3)).astype(np.float32))
    bad = rng.uniform(-10.0, 10.0, (12, 3)).astype(np.float32)
    bad[0, 0], bad[3, 1], bad[5, 2], bad[7, :] = np.nan, np.inf, -np.inf, np.nan
    parts.append(bad)
    q = np.concatenate(parts)
    n = 12 * tile + 1
    assert len(q) >= n
    q = np.ascontiguousarray(q[rng.permutation(len(q))[:n]])
    q[:len(edge)] = edge  # the edge points stay, in front
    images = [V.range_image(c, s, p) for c, s in scans]
    return dict(p=p, poses=poses, images=images, query=q, n_edge=len(edge), tile=tile)


@pytest.fixture(scope="module")
def five(pkg, _session_ctx, scans):
    """Five keyframes at general SE(3) poses in a store (z up), with five_data's query points and reference images."""
    tile, chunk = _consts(pkg)
    d = five_data(scans, tile)
    store = pkg.KeyframeStore(_session_ctx, slab_points=1 << 14)
    store.vis_setup(**d["p"])
    for c, s in scans:
        store.add(c, s)
    yield dict(d, store=store, chunk=chunk)
    store.close()


def _voters(five, n_ids):
    """n_ids voters: the five keyframes in turn; beyond the fifth the same clouds at poses shifted and turned a little."""
    ids = [k % 5 for k in range(n_ids)]
    poses = []
    for k in range(n_ids):
        p6 = np.array(POSES6[k % 5], np.float64)
        lap = k // 5
        p6 += lap * np.array([0.01, -0.008, 0.11, 0.4, -0.3, 0.02])
        poses.append(_pose(p6))
    return ids, poses


def _ref_votes(five, ids, poses, pts, p=None):
    return V.votes([five["images"][i] for i in ids], poses, pts, p or five["p"])


def _pad4(q):
    return np.ascontiguousarray(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1))


@pytest.mark.parametrize("window", [0, 1])
def test_votes_are_exact(pkg, ctx, five, window):
    import torch
    store, tile, chunk, q = five["store"], five["tile"], five["chunk"], five["query"]
    p = V.params(up_axis=2, window=window)
    store.vis_setup(**p)
    # the edge points do sit where they were built to sit
    e = V.project(V.transform(V.inverse_pose(five["poses"][0]), q[:five["n_edge"]]), p)
    assert e["obs"].all() and {0, p["n_col"] - 1} == set(e["col"].tolist()) and {0, p["n_row"] - 1} <= set(e["row"].tolist())
    seen = np.zeros(2, np.int64)
    for n, n_ids in ((len(q), chunk + 1), (tile + 1, chunk - 1), (tile + 1, chunk), (tile - 1, 5), (tile, 5), (1, 1), (len(q), 2 * chunk + 1)):
        ids, poses = _voters(five, n_ids)
        pts = q[:n]
        keep = V.unambiguous(pts, poses, p)
        assert (~keep).sum() <= 0.01 * len(pts)
        want = _ref_votes(five, ids, poses, pts, p)
        got = store.vis_votes(ids, poses, _pad4(pts))
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got[keep], want[keep]), (n, n_ids, np.flatnonzero(got != want)[:8])
        dev = store.vis_votes(ids, poses, torch.from_numpy(_pad4(pts)).to("cuda:0"))
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), got)  # host and device variants: the same bits
        nf, nh = pkg.visibility.split_votes(want)
        seen += (int((nf > 0).sum()), int((nh > 0).sum()))
    assert seen.min() > 200  # the comparison saw both kinds of vote, many times
    # a stride of 32 bytes (pcl::PointXYZI) reads the same points
    wide = np.zeros((tile + 1, 8), np.float32)
    wide[:, :3] = q[:tile + 1]
    wide[:, 4:] = 7.0
    ids, poses = _voters(five, 5)
    assert np.array_equal(store.vis_votes(ids, poses, wide), store.vis_votes(ids, poses, _pad4(q[:tile + 1])))
    assert store.vis_votes([], np.zeros((0, 4, 4)), _pad4(q[:10])).tolist() == [0] * 10  # no voters: no votes


def test_votes_add_up_over_voters(pkg, ctx, five, scans):
    """votes(A u B) == votes(A) + votes(B) for disjoint voters -- with a sixth keyframe 300 m away, so that most query points
    are further than 2 * max_range from some voter (a tile cull that is not conservative shows here); an id named twice votes
    twice; two identical calls give identical bits."""
    store, q = five["store"], five["query"]
    p = V.params(up_axis=2)
    store.vis_setup(**p)
    far6 = np.array(POSES6[1], np.float64) + np.array([0, 0, 0, 300.0, 40.0, 0])
    fid = store.add(*scans[1])  # (it stays in the module's store: the other tests name their voters)
    ids, poses = list(range(5)) + [fid], five["poses"] + [_pose(far6)]
    near_far = V.transform(_pose(far6), scans[1][1][::9, :3] * np.float32(0.7))
    pts = _pad4(np.concatenate([q, near_far]))
    whole = store.vis_votes(ids, poses, pts)
    assert np.array_equal(store.vis_votes(ids, poses, pts), whole)
    for split in ([0, 1, 2], [1, 4, 5], [5], []):
        A = [k for k in range(6) if k in split]
        B = [k for k in range(6) if k not in split]
        va = store.vis_votes([ids[k] for k in A], [poses[k] for k in A], pts)
        vb = store.vis_votes([ids[k] for k in B], [poses[k] for k in B], pts)
        assert np.array_equal(va + vb, whole), split
    only_far = store.vis_votes([fid], [poses[5]], pts)
    assert only_far[len(q):].any() and whole[:len(q)].any()  # both groups of points get votes, from their own side
    twice = store.vis_votes([2, 2], [poses[2], poses[2]], pts)
    assert np.array_equal(twice, 2 * store.vis_votes([2], [poses[2]], pts))
    # against the reference as well, far voter included
    keep = V.unambiguous(pts, poses, p)
    want = V.votes(five["images"] + [five["images"][1]], poses, pts, p)
    assert (~keep).sum() <= 0.01 * len(pts) and np.array_equal(whole[keep], want[keep])


def test_filter_keeps_the_reference_mask_in_order(pkg, ctx, five):
    import torch
    store, q = five["store"], five["query"]
    p = V.params(up_axis=2)
    store.vis_setup(**p)
    ids, poses = list(range(5)), five["poses"]
    keep = V.unambiguous(q, poses, p)
    assert (~keep).sum() <= 0.01 * len(q)
    pts = _pad4(q[keep])
    pts[:, 3] = np.arange(len(pts), dtype=np.float32)  # the fourth float travels with its point
    dyn = V.dynamic(_ref_votes(five, ids, poses, pts), p)
    assert 50 < dyn.sum() < len(pts) - 50
    out = store.vis_filter(ids, poses, pts)
    assert out.dtype == np.float32 and out.tobytes() == pts[~dyn].tobytes()
    dev = store.vis_filter(ids, poses, torch.from_numpy(pts).to("cuda:0"))
    assert dev.cpu().numpy().tobytes() == out.tobytes()
    for n in (1, five["tile"] - 1, five["tile"], five["tile"] + 1):  # the compaction's workgroup edge
        assert store.vis_filter(ids, poses, pts[:n]).tobytes() == pts[:n][~dyn[:n]].tobytes()
    assert store.vis_filter(ids, poses, pts[:0]).shape == (0, 4)
    store.vis_setup(**V.params(up_axis=2, min_free_votes=65535))
    assert store.vis_filter(ids, poses, pts).tobytes() == pts.tobytes()  # nothing can collect that many votes: everything stays


def test_add_to_fmap_without_removals_is_add_to_fmap(pkg, ctx, five):
    """min_free_votes = 65535 removes nothing: the map is, bit for bit, the one lslam_kfs_add_to_fmap builds, and no cloud byte
    crosses PCIe; with the default rule the counts are the reference's."""
    store, poses = five["store"], five["poses"]
    ids = list(range(5))
    maps = []
    for filtered in (False, True):
        store.vis_setup(**V.params(up_axis=2, min_free_votes=65535))
        fm = pkg.FeatureMap(ctx, 21, 11, 21)
        try:
            before = store.info()
            for k in ids:
                fm.update(poses[k][:3, 3])
                if filtered:
                    assert store.vis_add_to_fmap(k, fm, poses[k], ids, poses) == (0, 0)
                else:
                    store.add_to_fmap(k, fm, poses[k])
            after = store.info()
            assert (after["cloud_bytes_uploaded"], after["cloud_bytes_downloaded"]) == (before["cloud_bytes_uploaded"], before["cloud_bytes_downloaded"])
            maps.append(fm.get_full_map())
        finally:
            fm.close()
    assert len(maps[0]) > 1000 and maps[0].tobytes() == maps[1].tobytes()
    p = V.params(up_axis=2)
    store.vis_setup(**p)
    fm = pkg.FeatureMap(ctx, 21, 11, 21)
    try:
        fm.update(poses[0][:3, 3])
        c, s = store.get(0, 0), store.get(0, 1)
        want = []
        for cloud in (c, s):
            g = V.transform(poses[0], cloud)
            keep = V.unambiguous(g, poses, p)
            dyn = V.dynamic(_ref_votes(five, ids, poses, g), p)
            want.append((int((dyn & keep).sum()), int((~keep).sum())))
        got = store.vis_add_to_fmap(0, fm, poses[0], ids, poses)
        for t in range(2):
            assert abs(got[t] - want[t][0]) <= want[t][1], (got, want)
    finally:
        fm.close()


def test_refusals_leave_the_store_usable(pkg, ctx, five, scans):
    import ctypes as C
    rng = np.random.default_rng(44)
    p = V.params(up_axis=2)
    poses = five["poses"]
    store = pkg.KeyframeStore(ctx, slab_points=1 << 14)

    def refused(fn, word):
        with pytest.raises(pkg.LslamError) as e:
            fn()
        assert e.value.code == pkg.Status.ERR_INVALID and word in str(e.value), str(e.value)
    try:
        for c, s in scans[:3]:
            store.add(c, s)
        pts = _pad4(five["query"][:300])
        refused(lambda: store.vis_votes([0], poses[:1], pts), "lslam_vis_setup")  # before setup
        refused(lambda: store.vis_range_image(0), "lslam_vis_setup")
        refused(lambda: store.vis_filter([0], poses[:1], pts), "lslam_vis_setup")
        nan, inf = float("nan"), float("inf")
        for field, values in (("n_row", (0, 129)), ("n_col", (3, 4097)), ("fov_down_deg", (nan, -91.0, 16.0, 20.0)),
                              ("fov_up_deg", (nan, 91.0, -16.0, inf)), ("min_range", (0.0, -1.0, nan, inf)),
                              ("max_range", (1.0, 0.5, nan, inf)), ("window", (-1, 4)), ("abs_margin", (-0.1, nan, inf)),
                              ("rel_margin", (-0.1, nan, inf)), ("min_free_votes", (0, -3)), ("up_axis", (0, 3))):
            for v in values:
                word = "fov_up_deg" if (field, v) in (("fov_down_deg", 16.0), ("fov_down_deg", 20.0)) else field  # down < up is said of up
                refused(lambda: store.vis_setup(**{field: v}), word)
        assert not store.vis_info()["is_set"] and store.vis_info()["image_bytes"] == 0
        store.vis_setup(**p)
        good = store.vis_votes([0, 1, 2], poses[:3], pts)
        assert good.any()
        refused(lambda: store.vis_setup(n_row=200), "n_row")
        assert store.vis_info()["n_images"] == 3  # a refused setup drops nothing
        refused(lambda: store.vis_votes([3], poses[:1], pts), "out of range")
        refused(lambda: store.vis_votes([-1], poses[:1], pts), "out of range")
        refused(lambda: store.vis_range_image(3), "out of range")
        refused(lambda: store.vis_filter([0, 7], poses[:2], pts), "out of range")
        badT = poses[0].copy()
        badT[1, 3] = np.nan
        refused(lambda: store.vis_votes([0], [badT], pts), "not finite")
        lib, ip = store.lib, np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        Tp = poses[0].ctypes.data_as(C.POINTER(C.c_float))
        out = np.full(300, 0xA5A5A5A5, np.uint32)
        op = out.ctypes.data_as(C.POINTER(C.c_uint32))
        INVALID = int(pkg.Status.ERR_INVALID)
        assert lib.lslam_vis_votes(store.h, 1, None, Tp, pts.ctypes.data_as(C.c_void_p), 300, 16, op) == INVALID   # null ids
        assert lib.lslam_vis_votes(store.h, 1, ip, None, pts.ctypes.data_as(C.c_void_p), 300, 16, op) == INVALID   # null poses
        assert lib.lslam_vis_votes(store.h, 1, ip, Tp, None, 300, 16, op) == INVALID                               # null points
        assert lib.lslam_vis_votes(store.h, 1, ip, Tp, pts.ctypes.data_as(C.c_void_p), 300, 16, None) == INVALID   # null output
        assert lib.lslam_vis_votes(store.h, 1, ip, Tp, pts.ctypes.data_as(C.c_void_p), 300, 12, op) == INVALID     # stride
        assert lib.lslam_vis_votes(store.h, 65536, ip, Tp, pts.ctypes.data_as(C.c_void_p), 300, 16, op) == INVALID
        assert (out == 0xA5A5A5A5).all()
        assert lib.lslam_vis_range_image(store.h, 0, None) == INVALID and lib.lslam_vis_info(store.h, None) == INVALID
        kept = C.c_size_t(77)
        assert lib.lslam_vis_filter_device(store.h, 1, ip, Tp, None, 300, None, C.byref(kept)) == INVALID and kept.value == 77
        removed = (C.c_size_t * 2)(5, 6)
        assert lib.lslam_vis_add_to_fmap(store.h, 0, None, Tp, 1, ip, Tp, removed) == INVALID and tuple(removed) == (5, 6)
        fm = pkg.FeatureMap(ctx, 21, 11, 21)
        try:
            refused(lambda: store.vis_add_to_fmap(9, fm, poses[0], [0], poses[:1]), "out of range")
            refused(lambda: store.vis_add_to_fmap(0, fm, poses[0], [9], poses[:1]), "out of range")
            assert fm.info()["n_corner"] == 0 and fm.info()["n_surf"] == 0
        finally:
            fm.close()
        assert lib.lslam_debug_vis_votes(store.h, -1) == INVALID
        again = store.vis_votes([0, 1, 2], poses[:3], pts)
        assert np.array_equal(again, good)  # the store works as before
        assert lib.lslam_debug_vis_votes(store.h, 2) == 0  # the tap, in the shape of that call
        assert np.array_equal(store.vis_votes([0, 1, 2], poses[:3], pts), good)
        assert store.vis_info()["vote_launches"] == 3  # the tap's launches are not counted
    finally:
        store.close()
    own = pkg.Context(0)
    st = pkg.KeyframeStore(own, slab_points=1 << 14)
    st.add(_rand(rng, 100), _rand(rng, 200))
    st.vis_setup(**p)
    own.close()
    one = _pad4(five["query"][:4])
    for fn in (lambda: st.vis_setup(**p), lambda: st.vis_votes([0], poses[:1], one), lambda: st.vis_range_image(0),
               lambda: st.vis_info()):
        refused(fn, "its ctx was destroyed")
    st.close()


# ---- the scene: a box that is there for the first two of six keyframes -------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(synth):
    return V.scene(synth)


def _in_box(xyz, box):
    x0, x1, y0, y1, h = box
    return (xyz[:, 0] >= x0 - 0.1) & (xyz[:, 0] <= x1 + 0.1) & (xyz[:, 1] >= y0 - 0.1) & (xyz[:, 1] <= y1 + 0.1) & (xyz[:, 2] > 0.05) & \
        (xyz[:, 2] <= h + 0.1)


def test_scene_votes_remove_the_box_and_nothing_else(pkg, ctx, scene):
    p, poses = scene["params"], scene["poses"]
    # of the reference itself: no static point goes, at least half of the box does
    dyn = V.dynamic(scene["votes"], p)
    box = scene["is_box"]
    n_box, n_static = int(box.sum()), int((~box).sum())
    print("reference: %d of %d static points removed, %d of %d box points removed; %d of %d query points ambiguous" %
          ((dyn & ~box).sum(), n_static, (dyn & box).sum(), n_box, (~scene["keep"]).sum(), len(dyn)))
    assert n_box > 200 and (dyn & ~box).sum() == 0 and 2 * (dyn & box).sum() >= n_box
    assert (~scene["keep"]).sum() <= 0.01 * len(dyn)
    store = pkg.KeyframeStore(ctx)
    try:
        store.vis_setup(**p)
        ids = [store.add(c, s) for c, s in scene["clouds"]]
        for i, (c, s) in enumerate(scene["clouds"]):
            keep = V.unambiguous(c, None, p).all() and V.unambiguous(s, None, p).all()
            if keep:
                assert store.vis_range_image(i).tobytes() == scene["images"][i].tobytes(), i
        got = store.vis_votes(ids, poses, _pad4(scene["query"]))
        keep = scene["keep"]
        assert np.array_equal(got[keep], scene["votes"][keep])
        mask = pkg.visibility.dynamic_mask(got, p["min_free_votes"])
        assert np.array_equal(mask[keep], dyn[keep])
    finally:
        store.close()


def _scene_graph(pkg, ctx, scene, remove):
    g = pkg.Graph(ctx=ctx, resident=True, remove_dynamic=remove, dynamic_params=dict(up_axis=2) if remove else None)
    for T, (c, s) in zip(scene["poses"], scene["clouds"]):
        assert g.add_frame(T.astype(np.float64), c, s) is not None
    g.optimize()
    assert len(g.keyframes) == len(scene["poses"])
    return g


def test_graph_final_map_without_the_box(pkg, ctx, scene):
    """Graph(resident=True, remove_dynamic=True).get_final_feature_map(bootstrap=True) on the scene's keyframes: fewer map
    points inside the box than with it off; `removed` is, per keyframe, the reference's count at the pose the keyframe was added
    with (up to its ambiguous points), and sums to the difference of the points the two maps were given."""
    p = scene["params"]
    results = {}
    for remove in (False, True):
        g = _scene_graph(pkg, ctx, scene, remove)
        out = g.get_final_feature_map(ctx=ctx, cube_dims=(21, 11, 21), bootstrap=True)
        try:
            full = out["map"].get_full_map()
            results[remove] = dict(inside=int(_in_box(full[:, :3], scene["box"]).sum()), added=out["added"], poses=out["poses"],
                                   matched=out["matched"], removed=out.get("removed"), estimates=[np.array(k.estimate) for k in g.keyframes],
                                   counts=[g.store.counts(k.store_id) for k in g.keyframes])
        finally:
            out["map"].close()
            g.store.close()
    off, on = results[False], results[True]
    assert "removed" not in off or off["removed"] is None
    assert on["added"] == len(scene["poses"]) == len(on["removed"]) and off["added"] == on["added"]
    print("map points inside the box: %d without the filter, %d with it; removed per keyframe %s" % (off["inside"], on["inside"], on["removed"]))
    assert on["inside"] < off["inside"] and off["inside"] > 50
    given_off = sum(nc + ns for nc, ns in off["counts"])
    voters = [np.asarray(e, np.float64).astype(np.float32) for e in on["estimates"]]
    given_on = 0
    for k, (c, s) in enumerate(scene["clouds"]):
        for t, cloud in enumerate((c, s)):
            gpts = V.transform(on["poses"][k], cloud)
            keep = V.unambiguous(gpts, voters, p)
            dyn = V.dynamic(V.votes(scene["images"], voters, gpts, p), p)
            assert abs(on["removed"][k][t] - int((dyn & keep).sum())) <= int((~keep).sum()), (k, t)
            given_on += len(cloud) - on["removed"][k][t]
    assert sum(a + b for a, b in on["removed"]) == given_off - given_on
    assert sum(a + b for a, b in on["removed"][:2]) > 100


def test_graph_save_filters_both_maps(pkg, ctx, scene, tmp_path):
    """Graph.save with remove_dynamic: the unmatched map (graph/) and the matched one (graph2/) both hold fewer points inside
    the box than those of the same graph without the switch, and the result carries `removed`."""
    inside = {}
    for remove in (False, True):
        g = _scene_graph(pkg, ctx, scene, remove)
        d = tmp_path / ("on" if remove else "off")
        try:
            out = g.save(str(d), bootstrap=True)
            assert out["added"] == len(scene["poses"]) and ("removed" in out) == remove
            if remove:
                assert len(out["removed"]) == out["added"] and sum(a + b for a, b in out["removed"][:2]) > 100
            for sub in ("graph", "graph2"):
                fm = pkg.FeatureMap(ctx, 121, 111, 121)
                try:
                    assert fm.load_cloud_from_files(str(d / sub))
                    inside[(remove, sub)] = int(_in_box(fm.get_full_map()[:, :3], scene["box"]).sum())
                finally:
                    fm.close()
        finally:
            g.store.close()
    print("map points inside the box (graph, graph2): off %d %d, on %d %d" % (inside[(False, "graph")], inside[(False, "graph2")],
                                                                               inside[(True, "graph")], inside[(True, "graph2")]))
    # the box is in the unfiltered maps to begin with: its two visible faces (4 x 1.6 m and 2 x 1.6 m, 9.6 m^2) are 60 voxels of
    # the coarsest leaf used (0.4 m), and a 16-ring scan from 10 m (rings 0.35 m apart there) reaches at least a third of them
    for sub in ("graph", "graph2"):
        assert inside[(True, sub)] < inside[(False, sub)] and inside[(False, sub)] >= 20
