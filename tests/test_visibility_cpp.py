"""tests/cpp/visibility_end_to_end.cpp: pose_graph::Graph with remove_dynamic and KeyframeStore's vis_* members (the C++ mirror,
include/lslam_loop_closure.hpp) on the scene of a box that is there for two keyframes of six, against the Python mirror on
the same numbers."""
import subprocess

import numpy as np
import pytest

from test_abi import _build_cpp


def _write_scene(path, scene):
    with open(path, "wb") as f:
        f.write(np.uint32(len(scene["poses"])).tobytes())
        for T, (c, s) in zip(scene["poses"], scene["clouds"]):
            f.write(np.asarray(T, np.float64).tobytes())
            for cloud in (c, s):
                f.write(np.uint32(len(cloud)).tobytes())
                f.write(np.ascontiguousarray(cloud, np.float32).tobytes())


def test_cpp_program_compiles_and_needs_the_backend(pkg, tmp_path):
    """g++ -std=c++11 -Wall -Werror; without a GPU the program reports the missing backend."""
    import torch
    exe = _build_cpp(pkg, tmp_path, "visibility_end_to_end")
    if not torch.cuda.is_available():  # (with a GPU the gpu-marked test below runs the program)
        (tmp_path / "s.bin").write_bytes(np.uint32(0).tobytes())
        out = subprocess.run([str(exe), str(tmp_path / "s.bin"), "2"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "no CPU fallback" in out.stderr


@pytest.mark.gpu
def test_cpp_graph_removes_what_the_python_graph_removes(pkg, ctx, synth, tmp_path):
    """The two mirrors issue the same C-ABI calls on the same bits (the odometry poses are float32 values, the graph has no
    loops, so the estimates are the odometry poses): the keyframes added, the points left out per keyframe and the votes of
    KeyframeStore::vis_votes are equal; no cloud crosses PCIe for the filter."""
    import visibility_ref as V
    scene = V.scene(synth)
    p = scene["params"]
    g = pkg.Graph(ctx=ctx, resident=True, remove_dynamic=True, dynamic_params=dict(up_axis=2))
    try:
        for T, (c, s) in zip(scene["poses"], scene["clouds"]):
            assert g.add_frame(T.astype(np.float64), c, s) is not None
        g.optimize()
        out = g.get_final_feature_map(ctx=ctx, cube_dims=(21, 11, 21), bootstrap=True)
        out["map"].close()
        ids = [kf.store_id for kf in g.keyframes]
        poses = [kf.estimate for kf in g.keyframes]
        py_votes, py_pix = [], []
        for kf in g.keyframes:
            w = g.store.vis_votes(ids, poses, g.store.get(kf.store_id, 1))
            nf, nh = pkg.visibility.split_votes(w)
            py_votes.append([int((nf > 0).sum()), int((nh > 0).sum()), int(pkg.visibility.dynamic_mask(w, p["min_free_votes"]).sum())])
            py_pix.append(int(np.isfinite(g.store.vis_range_image(kf.store_id)).sum()))
    finally:
        g.store.close()
    _write_scene(tmp_path / "scene.bin", scene)
    exe = _build_cpp(pkg, tmp_path, "visibility_end_to_end")
    run = subprocess.run([str(exe), str(tmp_path / "scene.bin"), "2"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [l.split() for l in run.stdout.splitlines() if l.split()]
    removed = [(int(r[2]), int(r[3])) for r in rows if r[0] == "REMOVED"]
    votes = [[int(v) for v in r[2:5]] for r in rows if r[0] == "VOTES"]
    pix = [int(r[2]) for r in rows if r[0] == "IMAGE"]
    print("removed per keyframe", removed, "votes (free, hit, dynamic)", votes)
    assert ["ADDED", str(out["added"]), str(len(scene["poses"]))] in rows and out["added"] == len(scene["poses"])
    assert removed == [tuple(r) for r in out["removed"]] and sum(a + b for a, b in removed) > 100
    assert votes == py_votes and pix == py_pix
    assert ["MOVED", "0"] in rows and ["OFF", "1"] in rows
