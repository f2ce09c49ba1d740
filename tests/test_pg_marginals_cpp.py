"""tests/cpp/pg_marginals_end_to_end.cpp: SolverG2OT::marginals / relativeCovariances / marginalStats build with g++ -std=c++11
-Wall -Werror over the C ABI; on the GPU they give what the Python mirror gives on the same numbers."""
import subprocess

import numpy as np
import pytest

import marginals_ref as mr


def test_cpp_program_compiles_and_needs_the_backend(pkg, tmp_path):
    import torch
    from test_abi import _build_cpp
    exe = _build_cpp(pkg, tmp_path, "pg_marginals_end_to_end")
    if not torch.cuda.is_available():  # (with a GPU the gpu-marked test below runs the program)
        (tmp_path / "none.txt").write_text("0 0 0 0\n")
        out = subprocess.run([str(exe), str(tmp_path / "none.txt")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "no CPU fallback" in (out.stderr + out.stdout)


def _row(a):
    return " ".join("%.17g" % v for v in np.asarray(a, np.float64).reshape(-1))


@pytest.mark.gpu
def test_cpp_marginals_match_the_python_mirror(pkg, tmp_path):
    """A 22-vertex chain with three loop edges; both mirrors are handed the same 4x4 matrices and run the same library.  The only
    difference is the host-side matrix -> quaternion conversion, written twice: the poses agree to a few ulp, but two PCG runs
    on systems that differ in the last bit need not stop at the same iterate -- each is inside the reference bound of
    tests/marginals_ref.py (sqrt(6) column bounds per block, relative_bound per relative covariance), so they differ by at
    most twice that."""
    from importlib import import_module
    from test_abi import _build_cpp
    pgm = import_module("the-cooper-mapper_amd.pose_graph")
    g = mr.make_chain(22, 5, n_loops=3, box=2.0)
    mats = [pgm.pose7_to_mat(p) for p in g["init"]]
    rels = [pgm.pose7_to_mat(m) for m in g["meas"]]
    q, ref, max_iters = [3, 0, 21, 3, 12], 12, 4000
    pg = pkg.PoseGraph(0)
    for T in mats:
        pg.add_se3_node(T)
    for (i, j), Z, w in zip(g["ij"].tolist(), rels, g["info"]):
        pg.add_se3_edge(i, j, Z, w)
    H, S = mr.covariance(pg.linearize(), 0)
    cov, cross = pg.marginals(q, cross=True, max_iters=max_iters)
    rel = pg.relative_covariances(ref, q, max_iters=max_iters)
    st = pg.marginal_stats
    _, J = mr.relative_covariance(S, pg.poses(), ref, q)
    pg.close()
    with open(tmp_path / "graph.txt", "w") as f:
        f.write("%d %d %d %d\n" % (len(mats), len(g["ij"]), ref, max_iters))
        for T in mats:
            f.write(_row(T) + "\n")
        for (i, j), Z, w in zip(g["ij"].tolist(), rels, g["info"]):
            f.write("%d %d\n%s\n%s\n" % (i, j, _row(w), _row(Z)))
        f.write("%d\n%s\n" % (len(q), " ".join(str(v) for v in q)))
    exe = _build_cpp(pkg, tmp_path, "pg_marginals_end_to_end")
    out = subprocess.run([str(exe), str(tmp_path / "graph.txt")], capture_output=True, text=True, timeout=120)
    print(out.stdout[-300:], "...", out.stderr[-1500:])
    assert out.returncode == 0
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.split()]
    c_cov = np.array([[float(v) for v in r[2:]] for r in rows if r[0] == "COV"]).reshape(len(q), 6, 6)
    c_cross = np.array([[float(v) for v in r[3:]] for r in rows if r[0] == "CROSS"]).reshape(len(q), len(q), 6, 6)
    c_rel = np.array([[float(v) for v in r[2:]] for r in rows if r[0] == "REL"]).reshape(len(q), 6, 6)
    bound = 2 * np.sqrt(6) * mr.column_bound(H, S, 1e-8)
    d_cov = max(np.linalg.norm(c_cov[k] - cov[k]) for k in range(len(q)))
    d_cross = max(np.linalg.norm(c_cross[a, b] - cross[a, b]) for a in range(len(q)) for b in range(len(q)))
    d_rel = max(np.linalg.norm(c_rel[k] - rel[k]) / (2 * mr.relative_bound(H, S, J[k], 1e-8)) for k in range(len(q)))
    print("C++ against Python: cov %.3e cross %.3e (bound %.3e), rel / its bound %.3e" % (d_cov, d_cross, bound, d_rel))
    assert d_cov <= bound and d_cross <= bound and d_rel <= 1.0
    assert not c_cov[1].any() and not c_rel[4].any() and np.array_equal(c_cov[0], c_cov[3])
    assert ["REFUSED", "1"] in rows
    c_st = [r for r in rows if r[0] == "STATS"][0]
    assert int(c_st[1]) == st.columns == 24 and int(c_st[2]) == st.panels == 1 and int(c_st[4]) == st.coarse_used
