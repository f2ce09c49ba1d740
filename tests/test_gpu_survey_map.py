"""The survey-cloud feature map extractor on the device (lslam_survey_*, csrc/lslam_survey.hip) against the numpy restatement
tests/survey_map_ref.py: every stage through its tap, the whole extraction, the saved map through the localisation node.

Decisions (neighbour in radius, edge, boundary flag) are compared exactly: the taps receive the restatement's fp32 inputs, and
tests/test_survey_map_ref.py holds the scene's decision margins above 1e-5."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import localization_ref as lr
import survey_map_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def ulps(a, b):
    """Distance of two fp32 arrays in units in the last place (NaN against NaN: 0)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, np.where(np.isnan(a) | np.isnan(b), 1 << 40, d))


@pytest.fixture(scope="module")
def sm(pkg):
    return pkg.survey_map


@pytest.fixture(scope="module")
def scene():
    return R.scene_reference()


# ---- normals -----------------------------------------------------------------------------------------------------------------
def _patch(rng, n, spacing, origin, tilt=0.3):
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2) * spacing
    g = g + rng.uniform(-0.3 * spacing, 0.3 * spacing, g.shape)
    z = tilt * g[:, 0] - 0.2 * g[:, 1] + rng.normal(0, 0.0005, len(g))
    return (np.stack([g[:, 0], g[:, 1], z], 1) + np.asarray(origin)).astype(F)


def _normal_cases():
    rng = np.random.default_rng(3)
    r = 0.05
    cell = np.float64(F(r)) * R.GRID_CELL_PAD
    cases = {}
    # exactly 2 and exactly 3 neighbours (far from everything else), next to a well-populated patch
    patch = _patch(rng, 30, 0.01, (5.0, -3.0, 1.0))
    two = np.array([[7.0, 1.0, 2.0], [7.01, 1.0, 2.0]], F)
    three = np.array([[9.0, 1.0, 2.0], [9.01, 1.0, 2.0], [9.0, 1.013, 2.004]], F)
    surf = np.concatenate([patch, two, three], 0)
    q = np.concatenate([patch[::7], [[7.004, 1.001, 2.0]], [[9.004, 1.003, 2.001]], [[20.0, 20.0, 20.0]]], 0).astype(F)
    cases["two_and_three"] = (surf, q, r)
    # points and queries on cell walls of the search grid (cells of r * GRID_CELL_PAD from the surface minimum)
    patch = _patch(rng, 40, 0.008, (2.0, 2.0, 0.5), tilt=0.0)
    lo = patch.min(0).astype(np.float64)
    wall = patch.copy()
    wall[::5, 0] = (lo[0] + cell * (np.arange(len(wall[::5])) % 6)).astype(F)
    wall[1::9, 1] = (lo[1] + cell * (np.arange(len(wall[1::9])) % 6)).astype(F)
    cases["cell_wall"] = (wall, wall[::3].copy(), r)
    # more than 256 neighbours in radius
    dense = _patch(rng, 40, 0.002, (-4.0, 8.0, 3.0))
    cases["dense"] = (dense, dense[::40].copy(), r)
    # duplicate points
    patch = _patch(rng, 25, 0.012, (1.0, 1.0, 1.0))
    dup = np.concatenate([patch, patch[::3], patch[::3], patch[5:6].repeat(7, 0)], 0)
    cases["duplicates"] = (dup, patch[::2].copy(), r)
    return cases


@pytest.mark.parametrize("name", ["two_and_three", "cell_wall", "dense", "duplicates"])
def test_normals_tap(sm, ctx, name):
    surf, q, r = _normal_cases()[name]
    want, wcnt = R.normals(surf, q, r)
    got, gcnt = sm.debug_normals(ctx, surf, q, r)
    assert np.array_equal(gcnt, wcnt)
    if name == "two_and_three":
        assert sorted(wcnt[-3:]) == [0, 2, 3] and np.isnan(want[-3, 0]) and not np.isnan(want[-2, 0]) and np.isnan(want[-1, 0])
    if name == "dense":
        assert wcnt.max() > 256
    u = ulps(got, want)
    print(name, "queries", len(q), "neighbours", wcnt.min(), "..", wcnt.max(), "max ulp", u.max())
    assert u.max() <= 2


# ---- K nearest -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n37", "n61", "lattice", "scene"])
def test_knn_tap(sm, ctx, scene, name):
    rng = np.random.default_rng(5)
    if name == "n37":
        pts, cell = rng.uniform(-1, 1, (37, 3)).astype(F), 0.3
    elif name == "n61":
        pts, cell = rng.uniform(-1, 1, (61, 3)).astype(F), 0.0
    elif name == "lattice":  # distance ties everywhere: broken by index
        pts = (np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25).astype(F)
        pts, cell = pts[rng.permutation(len(pts))], 0.3
    else:
        pts, cell = scene[1]["blocks"][0]["pts"], 0.2
    want = R.knn_lists(pts, 60)
    got = sm.debug_knn(ctx, pts, 60, cell)
    if name == "n37":
        assert np.all(want[:, 37:] == -1) and np.all(want[:, :37] >= 0)
    assert np.array_equal(got, want)


# ---- region growing ----------------------------------------------------------------------------------------------------------
def _two_families(rng, n):
    """Unit normals of two directions 10 degrees apart (an edge exists inside a family only), random curvatures."""
    a = np.array([0.0, 0.0, 1.0])
    b = np.array([np.sin(np.radians(10)), 0.0, np.cos(np.radians(10))])
    fam = rng.integers(0, 2, n)
    nrm = np.where(fam[:, None] == 0, a, b)
    return np.concatenate([nrm, rng.uniform(0.0, 0.1, (n, 1))], 1).astype(F)


def _region_cases(scene):
    rng = np.random.default_rng(9)
    c = R.cos_threshold(R.DEFAULTS["smoothness_angle"])
    cases = {}
    b = scene[1]["blocks"][0]
    cases["scene"] = (b["normals"], b["lists"])
    # a dense clump beside a sparse line: the line's lists reach into the clump, the clump's never reach the line
    clump = rng.uniform(0, 0.05, (40, 3))
    line = np.stack([0.3 + 0.25 * np.arange(12), np.zeros(12), np.zeros(12)], 1)
    pts = np.concatenate([clump, line], 0).astype(F)
    lists = R.knn_lists(pts, 8)
    assert np.all(lists[:40] < 40) and np.any(lists[40:] < 40)
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (52, 1)), rng.uniform(0, 0.1, (52, 1))], 1).astype(F)
    nrm[40:, 3] = rng.uniform(0, 0.01, 12)  # the line's points rank first: seed order matters
    cases["clump_and_line"] = (nrm, lists)
    # a strip of 400 points with K = 4: the lowest rank is at one end and has 400 points to cross
    pts = np.stack([np.arange(400) * 1.0, np.zeros(400), np.zeros(400)], 1).astype(F)
    nrm = np.concatenate([np.tile([0.0, 1.0, 0.0], (400, 1)), (0.001 * (1 + np.arange(400)))[:, None]], 1).astype(F)
    cases["strip"] = (nrm, R.knn_lists(pts, 4))
    # clusters of exactly 49 and 50 points
    pts = np.concatenate([rng.uniform(0, 0.1, (49, 3)), rng.uniform(5, 5.1, (50, 3))], 0).astype(F)
    nrm = np.concatenate([np.tile([1.0, 0.0, 0.0], (99, 1)), rng.uniform(0, 0.1, (99, 1))], 1).astype(F)
    cases["sizes_49_50"] = (nrm, R.knn_lists(pts, 20))
    # equal curvatures: ranks by index alone
    pts = rng.uniform(0, 1, (300, 3)).astype(F)
    nrm = _two_families(rng, 300)
    nrm[:, 3] = F(0.02)
    cases["equal_curvatures"] = (nrm, R.knn_lists(pts, 10))
    return cases, c


@pytest.mark.parametrize("name", ["scene", "clump_and_line", "strip", "sizes_49_50", "equal_curvatures"])
def test_region_tap(sm, ctx, scene, name):
    cases, c = _region_cases(scene)
    nrm, lists = cases[name]
    want = R.region_sequential(nrm, lists, c)
    fix, rounds = R.region_fixpoint(nrm, lists, c)
    assert np.array_equal(want, fix)
    got, sweeps = sm.debug_region(ctx, nrm, lists, c)
    print(name, "points", len(nrm), "clusters", len(np.unique(want)), "synchronous rounds", rounds, "device sweeps", sweeps)
    assert np.array_equal(got, want)
    assert sweeps >= 1
    if name == "strip":
        assert rounds > 64 and len(np.unique(want)) == 1
    if name == "sizes_49_50":
        assert sorted(np.bincount(got)[np.unique(got)]) == [49, 50]


# ---- boundary ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene", "only_duplicates", "normal_along_z"])
def test_boundary_tap(sm, ctx, scene, name):
    rng = np.random.default_rng(13)
    thr, r = R.DEFAULTS["boundary_angle"], 0.1
    if name == "scene":
        b = scene[1]["blocks"][0]
        pts, nrm = b["pts"], b["normals"]
    elif name == "only_duplicates":
        patch = _patch(rng, 12, 0.03, (0.0, 0.0, 0.0), tilt=0.0)
        lone = np.tile(np.array([[3.0, 3.0, 3.0]], F), (4, 1))  # four copies of one point, nothing else within the radius
        pts = np.concatenate([patch, lone], 0)
        nrm = np.tile(np.array([[0.0, 0.0, 1.0]], F), (len(pts), 1))
    else:
        pts = _patch(rng, 15, 0.03, (1.0, -2.0, 0.7), tilt=0.0)
        nrm = np.tile(np.array([[0.0, 0.0, 1.0]], F), (len(pts), 1))
        nrm[::2] = np.array([0.0, 0.0, -1.0], F)
        nrm[1::4] = np.array([3e-6, -2e-6, 1.0], F)  # below Eigen's 1e-5: still the second branch
    wflag, wgap = R.boundary(pts, nrm, r, thr)
    gflag, ggap = sm.debug_boundary(ctx, pts, nrm, r, thr)
    print(name, "points", len(pts), "boundary", int(wflag.sum()), "max gap difference", np.abs(ggap - wgap).max())
    if name == "only_duplicates":
        assert not wflag[-4:].any() and np.all(wgap[-4:] == 0.0)
    assert np.array_equal(gflag, wflag)
    assert np.abs(ggap - wgap).max() <= 1e-9


# ---- the filter with a minimum count ---------------------------------------------------------------------------------------
def test_voxel_grid_min(pkg, sm, ctx):
    rng = np.random.default_rng(17)
    # voxels of leaf 1 with exactly 1, 2, 3 and 4 points
    pts = []
    for v, k in enumerate((1, 2, 3, 4, 2, 3)):
        pts.append(np.concatenate([rng.uniform(0.1, 0.9, (k, 3)) + [2.0 * v, 0.0, 0.0], rng.uniform(0, 9, (k, 1))], 1))
    cloud = np.concatenate(pts, 0).astype(F)
    cloud = cloud[rng.permutation(len(cloud))]
    got = sm.voxel_grid_min(ctx, cloud, 1.0, 3)
    want = R.voxel_filter_min(cloud, 1.0, 3)
    assert len(want) == 3 and np.array_equal(bits(got), bits(want))
    big = np.concatenate([rng.uniform(-20, 20, (30000, 3)), rng.uniform(0, 64, (30000, 1))], 1).astype(F)
    for leaf in (0.4, 1.0):
        one = sm.voxel_grid_min(ctx, big, leaf, 1)
        assert np.array_equal(bits(one), bits(pkg.voxel_grid(ctx, big, leaf)))  # bit for bit lslam_voxel_grid
        three = sm.voxel_grid_min(ctx, big, leaf, 3)
        assert np.array_equal(bits(three), bits(R.voxel_filter_min(big, leaf, 3))) and 0 < len(three) < len(one)
    far = np.array([[0, 0, 0, 1], [5000, 5000, 5000, 2], [1, 1, 1, 3]], F)  # the "leaf too small" guard: the input comes back
    assert np.array_equal(sm.voxel_grid_min(ctx, far, 0.01, 3), far)


# ---- the whole extraction ----------------------------------------------------------------------------------------------------
def _rows(a):
    return sorted(map(bytes, np.ascontiguousarray(a[:, :3], F)))


def _rows4(a):
    return sorted(map(bytes, np.ascontiguousarray(a[:, :4], F)))


@pytest.fixture(scope="module")
def extracted(sm, _session_ctx, scene, tmp_path_factory):
    cloud, ref = scene
    m = sm.extract(_session_ctx, cloud, **R.SCENE_PARAMS)
    d = tmp_path_factory.mktemp("survey_gpu")
    m.save(d)
    yield m, d
    m.close()


def test_extract_end_to_end(sm, ctx, scene, extracted, tmp_path):
    cloud, ref = scene
    m, d = extracted
    st = m.info()
    print("device stats", st)
    c, s = m.clouds()
    assert _rows(c) == _rows(ref["corner"]) and _rows(s) == _rows(ref["surf"])
    assert np.all(c[:, 3] == 0) and np.all(s[:, 3] == 0)
    for k, v in ref["stats"].items():
        assert st[k] == v, k
    assert st["label_sweeps"] >= 2
    assert st["blocks_kept"] == 2 and st["blocks_dropped"] == 1  # the second block; the detached patch
    # the saved map: the same files, the same order inside every cube
    R.save(ref, str(tmp_path))
    assert open(os.path.join(d, "index.txt")).read() == open(os.path.join(tmp_path, "index.txt")).read()
    n_files = len(open(os.path.join(d, "index.txt")).read().splitlines())
    assert n_files == 4  # two cubes, corner and surf each
    for k in range(n_files):
        assert np.array_equal(bits(lr.read_pcd_xyzi(os.path.join(d, "%d.pcd" % k))), bits(lr.read_pcd_xyzi(os.path.join(tmp_path, "%d.pcd" % k))))


def test_extract_empty_results(sm, ctx, scene):
    for cloud in (np.zeros((0, 3), F), R.make_scene()[20000:20300], np.full((5, 3), np.nan, F)):
        m = sm.extract(ctx, cloud, **R.SCENE_PARAMS)
        st = m.info()
        assert (st["n_corner"], st["n_surf"], st["blocks_kept"]) == (0, 0, 0)
        c, s = m.clouds()
        assert c.shape == (0, 4) and s.shape == (0, 4)
        m.close()
    with pytest.raises(sm.LslamError):
        sm.extract(ctx, scene[0][:10], knn_k=65)
    with pytest.raises(sm.LslamError):
        sm.extract(ctx, scene[0][:10], curvature_threshold=0.1)


def test_saved_map_round_trip_through_the_localisation_node(pkg, ctx, oracle, scene, extracted, tmp_path):
    """lslam_survey_save -> lslam_loc_load: the node's map and surround equal localization_ref's load of the restatement's
    clouds, bit for bit; after lslam_index_convert the paged node opens the directory too."""
    cloud, ref = scene
    m, d = extracted
    P = ref["params"]
    R.save(ref, str(tmp_path))
    want = lr.RefLocalization(oracle, P["cube_dims"], P["cube_size"], P["cube_origin"], map_filter_corner=0.4, map_filter_surf=0.8)
    want.load_map(str(tmp_path))
    node = pkg.LaserLocalization(ctx, *P["cube_dims"], map_filter_corner=0.4, map_filter_surf=0.8, cube_size=P["cube_size"],
                                 world_origin=P["cube_origin"], lidar_valid_distance=150.0)
    node.load_map(d)
    info = node.info()
    assert info["n_points"] == (len(want.map[0]), len(want.map[1])) and min(info["n_points"]) > 0
    assert info["cubes_loaded"] == (len(want.cubes[0]), len(want.cubes[1])) == (2, 2)
    gc, gs = node.get_surround()
    assert gc.shape == want.map[0].shape and gs.shape == want.map[1].shape
    assert _rows4(gc) == _rows4(want.map[0]) and _rows4(gs) == _rows4(want.map[1])  # every point, all four words, bit for bit
    node.close()
    lib = pkg.load_library()
    assert lib.lslam_index_convert(os.path.join(str(d), "index.txt").encode(), *[int(v) for v in P["cube_origin"]],
                                   os.path.join(str(d), "index2.txt").encode()) == 0
    paged = pkg.LaserLocalization(ctx, 7, 7, 7, map_filter_corner=0.4, map_filter_surf=0.8, cube_size=P["cube_size"],
                                  lidar_valid_distance=150.0, dynamic_mode=True, files_directory=d)
    paged.update((0.0, 0.0, 0.0))
    pc, ps = paged.get_window_surround()
    assert _rows4(pc) == _rows4(want.map[0]) and _rows4(ps) == _rows4(want.map[1])
    paged.close()


def test_extract_file_reads_a_pcd(sm, ctx, scene, tmp_path):
    cloud = scene[0][:20000]
    path = tmp_path / "survey.pcd"
    with open(path, "wb") as f:
        f.write(("VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH %d\nHEIGHT 1\nPOINTS %d\nDATA binary\n"
                 % (len(cloud), len(cloud))).encode())
        f.write(cloud.tobytes())
    a = sm.extract_file(ctx, path, **R.SCENE_PARAMS)
    b = sm.extract(ctx, cloud, **R.SCENE_PARAMS)
    assert a.info()["n_surf"] > 0
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a.clouds(), b.clouds()))
    a.close()
    b.close()
    (tmp_path / "c.pcd").write_bytes(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 1\nHEIGHT 1\nPOINTS 1\nDATA binary_compressed\n")
    with pytest.raises(sm.LslamError) as e:
        sm.extract_file(ctx, tmp_path / "c.pcd")
    assert "binary_compressed" in str(e.value)


def test_handles_own_their_buffers(pkg, sm, scene):
    """Two extractions alive on one context, destroyed in either order, eight times over: the device's free memory (what
    tests/test_gpu_ctx_lifetime.py observes) does not go down.  A block of the scene is 20 000 points: the smallest buffer a call
    makes per block is 320 kB, so sixteen calls that each left one behind would hold 5 MiB; 2 MiB is the allocation granule."""
    import torch
    cloud = scene[0]
    c = pkg.Context(0)
    for _ in range(2):  # settles what the runtime keeps per process and queue
        sm.extract(c, cloud, **R.SCENE_PARAMS).close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for k in range(8):
        maps = [sm.extract(c, cloud, **R.SCENE_PARAMS) for _ in range(2)]
        assert all(m.info()["n_surf"] > 0 for m in maps)
        for i in ((0, 1), (1, 0))[k % 2]:
            maps[i].close()
    lost = free0 - torch.cuda.mem_get_info()[0]
    print("free memory lost over sixteen extractions: %d bytes" % lost)
    assert lost <= 2 << 20
    c.close()


def test_cpp_mirror_end_to_end(pkg, scene, tmp_path):
    """tests/cpp/survey_map_end_to_end.cpp: extract -> save -> LaserLocalization::loadMap through the C++ mirrors."""
    exe = tmp_path / "survey_map_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "survey_map_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    cloud, ref = scene
    (tmp_path / "cloud.bin").write_bytes(np.ascontiguousarray(cloud[:, :3], F).tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "cloud.bin"), str(tmp_path), "4.0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    words = [l.split() for l in out.stdout.splitlines() if l.startswith("OK ")]
    got = {w[1]: [int(v) for v in w[2:]] for w in words}
    assert got["extract"] == [ref["stats"]["n_corner"], ref["stats"]["n_surf"], 2, 1]
    assert got["loaded"][0] > 0 and got["loaded"][1] > 0
