"""tests/cpp/edge_information_end_to_end.cpp: the C++ Graph with edge_information = "hessian" builds with g++ -std=c++11 -Wall
-Werror over the C ABI; on the GPU its information matrices equal the Python mirror's to the last bit for the same keyframes
(six keyframes of tests/test_gpu_edge_information.py's corridor, one loop measured 1 m wrong along the axis)."""
import subprocess

import numpy as np
import pytest


def test_cpp_program_compiles_and_needs_the_backend(pkg, tmp_path):
    import torch
    from test_abi import _build_cpp
    exe = _build_cpp(pkg, tmp_path, "edge_information_end_to_end")
    if not torch.cuda.is_available():  # (with a GPU the gpu-marked test below runs the program)
        (tmp_path / "none.txt").write_text("0 0.02\n0\n")
        out = subprocess.run([str(exe), str(tmp_path / "none.txt")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "no CPU fallback" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_cpp_graph_matches_the_python_mirror_bit_for_bit(ctx, pkg, tmp_path):
    from test_abi import _build_cpp
    import test_gpu_edge_information as G
    zs = [0.0, 8.0, 16.0, 17.0, 8.0, 0.3]
    rng = np.random.default_rng(41)
    clouds = [G.keyframe_clouds(rng, z, k) for k, z in enumerate(zs)]
    sigma = 0.02
    saved = G.GRAPH_Z
    G.GRAPH_Z = zs  # run_graph drives the keyframes of GRAPH_Z
    try:
        g, est, _ = G.run_graph(ctx, pkg, clouds, edge_information="hessian", range_sigma=sigma)
    finally:
        G.GRAPH_Z = saved
    try:
        omega = np.stack(g.solver._info)
        n_rows = [ei.n_rows for ei in g.edge_informations()]
        pos = np.stack([kf.estimate[:3, 3] for kf in g.keyframes])
        loop = g.loops[0]
    finally:
        g.store.close()
    assert len(omega) == len(zs) and min(n_rows) >= 50
    with open(tmp_path / "keyframes.txt", "w") as f:
        f.write("%d %.17g\n" % (len(zs), sigma))
        for z, (corner, surf) in zip(zs, clouds):
            odom = np.eye(4)
            odom[2, 3] = z
            f.write(" ".join("%.17g" % v for v in odom.reshape(-1)) + "\n")
            for c in (corner, surf):
                f.write("%d\n" % len(c))
                f.write("\n".join(" ".join("%.9g" % v for v in p) for p in c.tolist()) + "\n")
        f.write("1\n0 %d\n" % (len(zs) - 1))
        f.write(" ".join("%.17g" % v for v in loop.relative_pose.astype(np.float64).reshape(-1)) + "\n")
    exe = _build_cpp(pkg, tmp_path, "edge_information_end_to_end")
    out = subprocess.run([str(exe), str(tmp_path / "keyframes.txt")], capture_output=True, text=True, timeout=120)
    print(out.stdout[:200], "...", out.stderr[-1500:])
    assert out.returncode == 0
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.split()]
    assert ["REFUSED", "1"] in rows and ["EDGES", str(len(zs))] in rows
    info = [r for r in rows if r[0] == "INFO"]
    assert [int(r[1]) for r in info] == list(range(len(zs))) and [int(r[2]) for r in info] == n_rows
    c_omega = np.array([[float.fromhex(v) for v in r[3:]] for r in info]).reshape(len(zs), 6, 6)
    assert np.array_equal(c_omega.view(np.uint64), omega.view(np.uint64))
    assert not np.array_equal(c_omega[0], c_omega[1])  # ... and they are the data's, not the constants
    cpos = np.array([[float(v) for v in r[2:5]] for r in rows if r[0] == "POS"])
    print("C++ Graph against Python Graph: positions %.3e" % np.abs(cpos - pos).max())
    assert cpos.shape == pos.shape and np.abs(cpos - pos).max() <= 1e-9  # the same system through the same solver
