"""CPU checks of the re-localisation stage: its numpy restatement (tests/relocalization_ref.py) on hand-made cases and on the
scene of tests/localization_ref.py, the host half of the library's selection (lslam_reloc_nms) against the restatement, the two
device-free helpers of the Python mirror, and the new entry points' declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import localization_ref as lr
import relocalization_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
RELOC = ["lslam_reloc_relocalize", "lslam_reloc_scores", "lslam_reloc_nms", "lslam_reloc_occupied", "lslam_reloc_info"]


class TinyRef:
    """The part of RefLocalization the restatement reads, over a hand-made map and with no scan filter."""
    cube_size, origin, dims = 50.0, (10, 10, 10), (21, 21, 21)

    def __init__(self, corner, surf):
        self.map = [np.asarray(corner, F).reshape(-1, 4), np.asarray(surf, F).reshape(-1, 4)]

    def prepare_frame(self, c, s):
        return np.asarray(c, F).reshape(-1, 4), np.asarray(s, F).reshape(-1, 4)


def _capi():
    from importlib import import_module
    return import_module("the-cooper-mapper_amd.capi")


def _loc():
    from importlib import import_module
    return import_module("the-cooper-mapper_amd.laser_localization")


def test_voxel_index_is_floor_not_truncation():
    inv = rr.inv_of(2.0)
    pts = np.array([[-0.5, 0.5, 0.0], [-2.0, 2.0, -2.0000002], [1.9999999, -1.9999999, 4.0], [np.nan, 0, 0], [0, np.inf, 0],
                    [0, 0, -np.inf], [3e6, 0, 0], [-2097152.0, 0, 0], [-2097153.0, 0, 0], [2097151.9, 0, 0]], F)
    k, ok = rr.voxel_keys(pts, inv)
    idx = np.stack([(k >> 42) & 0x1fffff, (k >> 21) & 0x1fffff, k & 0x1fffff], 1) - rr.IDX_LIM
    assert ok.tolist() == [True, True, True, False, False, False, False, True, False, True]
    assert idx[0].tolist() == [-1, 0, 0]        # truncation would give 0 for -0.25
    assert idx[1].tolist() == [-1, 1, -2]       # exactly on a face: the face belongs to the voxel above it
    assert idx[2].tolist() == [0, -1, 2]
    assert idx[7].tolist() == [-rr.IDX_LIM, 0, 0] and idx[9].tolist() == [rr.IDX_LIM - 1, 0, 0]
    assert rr.inv_of(0) == F(0.5)               # voxel 0 means 2.0


def test_score_counts_hits_per_type_and_skips_points_without_a_voxel():
    corner_map = [[-0.5, -0.5, -0.5, 0], [10.5, 0.5, 0.5, 0]]
    surf_map = [[0.5, 0.5, 0.5, 0], [-3.0, -3.0, -3.0, 0]]
    ref = TinyRef(corner_map, surf_map)
    sets = rr.occupancy_sets(ref, 2.0)
    assert len(sets[0]) == 2 and len(sets[1]) == 2
    corner = np.array([[-1.0, -1.0, -1.0, 0], [0.5, 0.5, 0.5, 0], [np.nan, 0, 0, 0]], F)  # hit, surf's voxel (no corner there), no voxel
    surf = np.array([[1.0, 1.0, 1.0, 0], [-2.0, -2.0, -2.0, 0], [-4.0, -4.0, -4.0, 0]], F)  # hit, on a face: voxel -1 (no surf), hit
    I = np.eye(3, dtype=F)[None]
    pos = np.array([[0, 0, 0], [10, 0, 0], [0.5, 0.5, 0.5], [1000.0, 0, 0]], F)
    sc, n = rr.scores(ref, corner, surf, I, pos, 2.0)
    assert n == (3, 3)
    # at (10, 0, 0): corner (0.5, .5, .5) -> (10.5, .5, .5) hits; at (.5, .5, .5): corner 1 -> (-.5, ...) hits voxel -1; surf 2
    # (-2 -> -1.5) stays in voxel -1 (no surf there), surf 3 (-4 -> -3.5) stays in voxel -2 (hit), surf 1 stays in voxel 0 (hit)
    assert sc.tolist() == [[3, 1, 3, -1]]  # x = 1000 is cube 30 of 21: refused
    Rz = np.array([[[0, -1, 0], [1, 0, 0], [0, 0, 1]]], F)  # a quarter turn: (x, y) -> (-y, x)
    sc2, _ = rr.scores(ref, np.array([[0.5, -10.5, 0.5, 0]], F), np.zeros((0, 4), F), Rz, pos[:1], 2.0)
    assert sc2.tolist() == [[1]]
    assert rr.occupied(sets, 0, [[-1.9, -0.1, -2.0]], 2.0).tolist() == [1] and rr.occupied(sets, 1, [[-1.9, -0.1, -2.0]], 2.0).tolist() == [0]
    assert rr.subsample(np.arange(10), 4).tolist() == [0, 3, 6, 9] and rr.subsample(np.arange(10), 10).tolist() == list(range(10))
    assert rr.subsample(np.arange(9), 4).tolist() == [0, 3, 6]


def test_top_m_order_under_ties():
    sc = np.array([[5, 7, 7, -1], [7, 0, 5, 9]], np.int32)
    idx, val = rr.top_m(sc, 4)
    assert idx.tolist() == [7, 1, 2, 4] and val.tolist() == [9, 7, 7, 7]
    idx, val = rr.top_m(sc, 100)  # top_m > H: everything but the refused one
    assert idx.tolist() == [7, 1, 2, 4, 0, 6, 5] and val.tolist() == [9, 7, 7, 7, 5, 5, 0]
    run = np.full(5000, 3, np.int32)  # a long run of equal scores: the lowest indices win
    run[4321] = 4
    idx, val = rr.top_m(run, 300)
    assert idx.tolist() == [4321] + list(range(299)) and val.tolist() == [4] + [3] * 299
    assert len(rr.top_m(np.full(10, -1), 4)[0]) == 0


def _nms_case():
    pos = np.array([[x, y, 0.0] for x in range(6) for y in range(2)], F)  # 12 positions, 1 m apart
    n_rot = 8
    # (rotation, position): neighbours in position and rotation, across the wrap, and far ones
    hyp = [(0, 0), (1, 1), (7, 2), (3, 0), (0, 6), (6, 3), (4, 11), (0, 0 + 1)]
    return pos, n_rot, np.array([r * len(pos) + j for r, j in hyp], np.int32)


def test_nms_cyclic_and_not():
    pos, n_rot, top = _nms_case()
    keep = rr.nms(top, pos, n_rot, nms_m=1.0, nms_rot=1, cyclic=False, max_candidates=8)
    # (1,1) is next to (0,0) in both; (7,2) is 1 m away but 7 rotations apart without the wrap, and it then suppresses (6,3)
    assert keep.tolist() == [0, 2, 3, 4, 6]
    keep = rr.nms(top, pos, n_rot, nms_m=1.0, nms_rot=1, cyclic=True, max_candidates=8)
    assert keep.tolist() == [0, 3, 4, 5, 6]      # with the wrap rotation 7 is next to rotation 0
    assert rr.nms(top, pos, n_rot, 1.0, 1, True, 2).tolist() == [0, 3]
    assert rr.nms(top, pos, n_rot, 100.0, 0, True, 8).tolist() == [0, 1, 2, 3, 5, 6]  # the same rotation only


def test_library_nms_equals_the_restatement(pkg):
    """The host half of the device stage's selection, which needs no GPU."""
    capi = _capi()
    lib = capi.load_library()
    rng = np.random.default_rng(5)
    pos, n_rot, top = _nms_case()
    cases = [(pos, n_rot, top, dict(nms_m=1.0, nms_rot=1, rot_cyclic=0, max_candidates=8)),
             (pos, n_rot, top, dict(nms_m=1.0, nms_rot=1, rot_cyclic=1, max_candidates=8)),
             (pos, n_rot, top, dict(nms_m=100.0, nms_rot=-1, rot_cyclic=1, max_candidates=8)),
             (pos, n_rot, top, dict(nms_m=1.0, nms_rot=1, rot_cyclic=1, max_candidates=2))]
    big_pos = rng.uniform(-8, 8, (400, 3)).astype(F)
    big_top = rng.permutation(400 * 90)[:1024].astype(np.int32)
    cases.append((big_pos, 90, big_top, dict(nms_m=2.0, nms_rot=3, rot_cyclic=1, max_candidates=64)))
    cases.append((big_pos, 90, big_top, dict()))  # the defaults: 2 m, 2 indices, not cyclic, 8 candidates
    for p, nr, t, kw in cases:
        o = capi.LslamRelocOpts(**kw)
        keep = np.zeros(64, np.int32)
        n = lib.lslam_reloc_nms(t.ctypes.data_as(capi.c_int32_p), len(t), p.ctypes.data_as(C.POINTER(C.c_float)), nr, len(p), C.byref(o),
                                keep.ctypes.data_as(capi.c_int32_p))
        want = rr.nms(t, p, nr, kw.get("nms_m", 2.0) or 2.0, {0: 2, -1: 0}.get(kw.get("nms_rot", 0), kw.get("nms_rot", 0)),
                      bool(kw.get("rot_cyclic", 0)), kw.get("max_candidates", 8) or 8)
        assert n == len(want) and keep[:n].tolist() == want.tolist(), kw
    bad = capi.LslamRelocOpts(top_m=1025)
    keep = np.zeros(64, np.int32)
    assert lib.lslam_reloc_nms(top.ctypes.data_as(capi.c_int32_p), len(top), pos.ctypes.data_as(C.POINTER(C.c_float)), n_rot, len(pos),
                               C.byref(bad), keep.ctypes.data_as(capi.c_int32_p)) == pkg.Status.ERR_INVALID


def test_yaw_sweep_and_grid_positions():
    loc = _loc()
    y = loc.yaw_sweep(4.0, 2)
    assert y.shape == (90, 3) and y.dtype == np.float32 and y.rot_cyclic
    assert np.all(y[:, :2] == 0) and y[0, 2] == 0 and np.allclose(np.diff(y[:, 2]), np.deg2rad(4.0), atol=1e-6)
    y = loc.yaw_sweep(90.0, 1, tilt=(0.1, -0.2))
    assert np.allclose(y[:, 1], [0, np.pi / 2, np.pi, 3 * np.pi / 2]) and np.all(y[:, 0] == F(0.1)) and np.all(y[:, 2] == F(-0.2))
    with pytest.raises(ValueError):
        loc.yaw_sweep(7.0, 2)
    g = loc.grid_positions((1.0, -2.0), 1.0, 0.5, 1.8)
    assert g.shape == (25, 3) and g.dtype == np.float32 and np.all(g[:, 2] == F(1.8))
    assert g[0].tolist() == [0.0, -3.0, F(1.8)] and g[1].tolist() == [0.0, -2.5, F(1.8)] and g[-1].tolist() == [2.0, -1.0, F(1.8)]
    assert loc.RELOC_POS_TILE == 32 and loc.RELOC_CHUNK == 1024


def test_reloc_entry_points_are_declared_exported_and_refuse_a_null_handle(pkg):
    capi = _capi()
    txt = open(os.path.join(ROOT, "include", "lslam_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert set(re.findall(r"\b(lslam_reloc_[a-z0-9_]+)\s*\(", code)) == set(RELOC)
    lib = capi.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(lslam_reloc_[a-z0-9_]+)\b", exported)) == set(RELOC)
    for name in RELOC:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert "#define LSLAM_ABI_VERSION 7" in txt and "#define LSLAM_RELOC_POS_TILE 32" in txt and "#define LSLAM_RELOC_CHUNK 1024" in txt
    # the structs as the C compiler lays them out (natural alignment, LP64)
    assert C.sizeof(capi.LslamRelocOpts) == 40 and C.sizeof(capi.LslamRelocCandidate) == 44
    assert C.sizeof(capi.LslamRelocResult) == 136 + 64 * 44 + 8 and C.sizeof(capi.LslamRelocMapStats) == 40
    fp = C.POINTER(C.c_float)
    pts = np.zeros((3, 4), F)
    vp = pts.ctypes.data_as(C.c_void_p)
    rot, pos = np.zeros(3, F), np.zeros(3, F)
    res = capi.LslamRelocResult()
    res.n_candidates = 7
    info = capi.LslamRelocMapStats()
    info.builds = 7
    sc, out = np.zeros(1, np.int32), np.zeros(3, np.uint8)
    calls = {
        "lslam_reloc_relocalize": lambda: lib.lslam_reloc_relocalize(None, vp, 3, vp, 3, 16, rot.ctypes.data_as(fp), 1, pos.ctypes.data_as(fp),
                                                                     1, None, C.byref(res)),
        "lslam_reloc_scores": lambda: lib.lslam_reloc_scores(None, vp, 3, vp, 3, 16, rot.ctypes.data_as(fp), 1, pos.ctypes.data_as(fp), 1, None,
                                                             sc.ctypes.data_as(capi.c_int32_p), None, None, None, None),
        "lslam_reloc_occupied": lambda: lib.lslam_reloc_occupied(None, 0, 2.0, vp, 3, 16, out.ctypes.data_as(capi.c_uint8_p)),
        "lslam_reloc_info": lambda: lib.lslam_reloc_info(None, C.byref(info)),
    }
    for name, call in calls.items():
        assert call() == pkg.Status.ERR_INVALID, name
        msg = lib.lslam_last_error().decode()
        assert msg.split(":")[0] == name and "null localisation node" in msg, (name, msg)
    assert res.n_candidates == 0 and res.winner == -1 and info.builds == 0
    assert pkg.yaw_sweep is not None and pkg.grid_positions is not None and "RelocResult" in pkg.__all__


def test_cpp_relocalization_mirror_compiles(pkg, tmp_path):
    """include/lslam_pipeline.hpp with LaserLocalization::relocalize builds with g++ -std=c++11 -Wall -Werror; without a GPU the
    example reports the missing backend and exits 1."""
    import torch
    exe = tmp_path / "relocalization_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "relocalization_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    if not torch.cuda.is_available():
        (tmp_path / "none.bin").write_bytes(b"")
        out = subprocess.run([str(exe), str(tmp_path / "none.bin")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "backend unavailable" in out.stderr


@pytest.fixture(scope="module")
def scene(synth):
    return lr.make_scene(synth, n_sweeps=1)


def test_score_is_discriminative_on_the_scene(scene, oracle):
    """Sweep 0 (ground truth (3.0, -2.0, 1.8), yaw 0.3 rad), scan filters 1.0 / 1.0, voxel 2.0, positions at 1 m over +-4 m offset
    (0.37, -0.41) from the truth, yaw on the 4 degree lattice around the truth and around its three quarter-turn aliases (the
    world is square): the top hypothesis is the truth's cell, and the best hypothesis beyond nms_m = 2 m scores strictly less."""
    ref = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
    ref.set_map(scene["map_corner"], scene["map_surf"], filter=False)
    c, s = scene["sweeps"][0]
    gt = np.asarray(scene["poses"][0], np.float64)
    fc, fs = ref.prepare_frame(c, s)
    assert len(fc) + len(fs) == 3274
    step, ystep = 1.0, 4.0
    off = np.arange(-4, 5) * step
    pos = np.array([[gt[3] + 0.37 + dx, gt[4] - 0.41 + dy, gt[5]] for dx in off for dy in off], F)
    lattice = np.arange(90) * ystep
    near = lambda a, b: abs((a - b + 180.0) % 360.0 - 180.0)
    yaws = np.array([a for a in lattice if any(near(a, np.rad2deg(gt[2]) + q) <= 3 * ystep for q in (0, 90, 180, 270))])
    assert len(yaws) == 24
    Rs = np.stack([ref.pose_to_isometry(np.array([0, 0, np.deg2rad(a), 0, 0, 0], F))[:3, :3] for a in yaws])
    sc, n = rr.scores(ref, c, s, Rs, pos, 2.0)
    idx, val = rr.top_m(sc, sc.size)
    best = int(idx[0])
    bp, by = pos[best % len(pos)], yaws[best // len(pos)]
    dpos, dyaw = np.abs(bp[:2] - gt[3:5]), near(by, np.rad2deg(gt[2]))
    far = np.abs(pos[idx % len(pos)][:, :2] - bp[None, :2]).max(1) > 2.0
    print("best: score %d of %d at %.2f m, %.1f deg from the truth; best beyond 2 m: %d (yaw %.0f deg)" %
          (val[0], sum(n), np.hypot(*dpos), dyaw, val[far][0], yaws[idx[far][0] // len(pos)]))
    assert dpos.max() <= step and dyaw <= ystep
    assert val[far][0] < val[0]
