"""tests/cpp/map_quality_end_to_end.cpp: the C++ mirrors of the map-quality feature (Graph::mapQuality, KeyframeStore::mapQuality,
FeatureMap::quality, trajectoryEval) on the displaced-keyframe scene of tests/map_quality_ref.py, against the Python mirrors on
the same numbers: the integers are equal and so are the means."""
import subprocess

import numpy as np
import pytest

import map_quality_ref as ref
from test_abi import _build_cpp

KEYS = ("n_query", "n_defined", "n_sparse", "sum_entropy_q32", "sum_plane_var_q30", "sum_neighbors", "max_neighbors")
MEANS = ("mean_entropy", "mean_plane_variance", "mean_neighbors")


def _scene():
    clouds, poses, moved = ref.keyframe_scene()
    rng = np.random.default_rng(31)
    corners = [rng.uniform(-1, 1, (60 + 5 * k, 4)).astype(np.float32) for k in range(len(clouds))]
    return corners, clouds, poses, moved


def _write_scene(path, corners, clouds, odoms, estimates):
    with open(path, "wb") as f:
        f.write(np.uint32(len(clouds)).tobytes())
        for c, s, O, E in zip(corners, clouds, odoms, estimates):
            f.write(np.asarray(O, np.float64).tobytes())
            f.write(np.asarray(E, np.float64).tobytes())
            for cloud in (c, s):
                f.write(np.uint32(len(cloud)).tobytes())
                f.write(np.ascontiguousarray(cloud, np.float32).tobytes())


def test_cpp_program_compiles_and_needs_the_backend(pkg, tmp_path):
    """g++ -std=c++11 -Wall -Werror; without a GPU the program reports the missing backend."""
    import torch
    exe = _build_cpp(pkg, tmp_path, "map_quality_end_to_end")
    if not torch.cuda.is_available():  # (with a GPU the gpu-marked test below runs the program)
        (tmp_path / "s.bin").write_bytes(np.uint32(0).tobytes())
        out = subprocess.run([str(exe), str(tmp_path / "s.bin")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "backend unavailable" in out.stderr and "no CPU fallback" in out.stderr


@pytest.mark.gpu
def test_cpp_mirrors_equal_the_python_mirrors(pkg, ctx, tmp_path):
    corners, clouds, poses, moved = _scene()
    want = {}
    graphs = []
    for tag, resident in (("RES", True), ("HOST", False)):
        g = pkg.Graph(device=ctx.device, ctx=ctx, resident=resident)
        graphs.append(g)
        kfs = [g.add_frame(moved[k], corners[k], clouds[k]) for k in range(len(clouds))]
        for kf, T in zip(kfs, poses):
            kf.estimate = T.copy()
        want[tag + "_EST"] = g.map_quality("estimate", "surf", keyframes=kfs)
        want[tag + "_ODOM"] = g.map_quality("odom", "surf", keyframes=kfs)
        if resident:
            want["STORE_CORNER"] = g.store.map_quality([kf.store_id for kf in kfs], poses, "corner", radius=0.5, min_neighbors=3)
    fm = pkg.FeatureMap(ctx)
    fm.update(np.zeros(3, np.float32))
    fm.add_feature_cloud(corners[0], clouds[0], np.asarray(poses[0], np.float64).astype(np.float32))
    want["FMAP_CORNER"] = fm.quality("corner", radius=0.5, min_neighbors=3)
    want["FMAP_SURF"] = fm.quality("surf")
    fm.close()
    stamps = np.arange(len(poses), dtype=np.float64)
    traj = pkg.trajectory_eval(stamps, [T[:3, 3] for T in poses], stamps, [T[:3, 3] for T in moved], align=True)
    graphs[0].store.close()

    _write_scene(tmp_path / "scene.bin", corners, clouds, moved, poses)
    exe = _build_cpp(pkg, tmp_path, "map_quality_end_to_end")
    run = subprocess.run([str(exe), str(tmp_path / "scene.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [l.split() for l in run.stdout.splitlines() if l.split()]
    got = {r[1]: r[2:] for r in rows if r[0] == "Q"}
    assert sorted(got) == sorted(want)
    for tag, st in want.items():
        assert [int(v) for v in got[tag][:7]] == [st[k] for k in KEYS], tag
        for v, k in zip(got[tag][7:], MEANS):
            assert float.fromhex(v) == st[k], (tag, k)
    assert want["RES_EST"]["mean_plane_variance"] <= 0.1 * want["RES_ODOM"]["mean_plane_variance"]
    assert want["FMAP_SURF"]["n_query"] > 100 and want["STORE_CORNER"]["n_query"] == sum(len(c) for c in corners)
    t = next(r for r in rows if r[0] == "TRAJ")
    assert (int(t[1]), int(t[2]), int(t[5])) == (traj["n_used"], traj["n_gated"], int(traj["aligned"])) and traj["n_used"] == 4
    assert float.fromhex(t[3]) == traj["mean"][3] and float.fromhex(t[4]) == traj["max"][3] and float.fromhex(t[6]) == traj["ate_rmse"]
    assert ["MOVED", "0"] in rows
