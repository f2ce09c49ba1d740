"""oracle/posegraph_oracle.c (compiled LM: analytic Jacobians, RCM-ordered envelope block Cholesky -- the CPU baseline of the
pose-graph leg) against oracle/posegraph_oracle.py (numpy: numeric Jacobians, SuperLU).  CPU only.  Parity of both with the
reference is unpinned: g2o (pose_graph/solver_g2o.cpp:16,79-95) is not available; they restate its published conventions
independently of each other -- different Jacobians, different linear solver."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import posegraph_oracle as po  # noqa: E402
import posegraph_oracle_c as pc  # noqa: E402


def _graph(**kw):
    return po.make_graph(**kw)


def test_linearisation_matches_the_numpy_oracle():
    """Measured on this graph: H 1.5e-9 max|H|, b 1.7e-9 max|b| (the central differences' error at positions of 40 m; the bound
    was 1e-6), chi2 1.1e-15; asserted at 3e-9 and 1e-13."""
    g = _graph(n_kf=120, n_loop=400)
    H, b, c2 = po.linearize(g["init"], g["ij"], g["meas"], g["info"])
    diag, bc, c2c = pc.linearize(g["init"], g["ij"], g["meas"], g["info"], fixed=0)
    assert abs(c2 - c2c) <= 1e-13 * c2
    Hd = H.toarray()
    scale = np.abs(Hd).max()
    for v in range(1, 120):  # vertex 0 is fixed: identity row in the C oracle
        assert np.abs(diag[v] - Hd[6 * v:6 * v + 6, 6 * v:6 * v + 6]).max() <= 3e-9 * scale, v  # numeric Jacobians: h = 1e-6
    assert np.array_equal(diag[0], np.eye(6)) and not bc[:6].any()
    assert np.abs(bc[6:] - b[6:]).max() <= 3e-9 * np.abs(b).max()


def test_damped_solve_matches_superlu():
    g = _graph(n_kf=150, n_loop=500, seed=3)
    H, b, c2 = po.linearize(g["init"], g["ij"], g["meas"], g["info"])
    for lam in (1e-6 * H.diagonal().max(), 1e-2 * H.diagonal().max()):
        dx = pc.solve(g["init"], g["ij"], g["meas"], g["info"], lam, fixed=0)
        ref = po.solve_damped(H, b, lam, 0)
        assert not dx[:6].any()
        assert np.abs(dx - ref).max() <= 1e-5 * np.abs(ref).max()  # Jacobians differ by the finite-difference error


def test_lm_run_matches_the_numpy_oracle():
    g = _graph(n_kf=200, n_loop=700, seed=11)
    ref, hist = po.optimize(g["init"], g["ij"], g["meas"], g["info"], fixed=0, max_iters=12)
    out, st = pc.optimize(g["init"], g["ij"], g["meas"], g["info"], fixed=0, max_iters=12)
    assert st.status == 0 and st.iterations == len(hist) and st.trials == sum(h["trials"] for h in hist)
    assert abs(st.chi2_final - hist[-1]["chi2"]) <= 1e-6 * hist[-1]["chi2"]
    assert np.abs(out[:, :3] - ref[:, :3]).max() <= 1e-5  # twelve iterations apart through different Jacobians (central differences, h = 1e-6)
    assert st.chi2_final < 1e-3 * st.chi2_initial  # it optimised something


def test_envelope_order_is_a_permutation_and_small():
    """RCM on a chain with loop closures: the envelope is far smaller than the dense lower triangle; disconnected parts and a
    fixed vertex in the middle are handled."""
    g = _graph(n_kf=300, n_loop=1200)
    out, st = pc.optimize(g["init"], g["ij"], g["meas"], g["info"], fixed=0, max_iters=1)
    assert st.env_blocks < 0.35 * 300 * 301 / 2 and st.bandwidth < 300
    # two components: the second one floats (singular without damping) but LM's lambda keeps the factorisation definite
    ij2 = np.concatenate([g["ij"], g["ij"] + 300]).astype(np.int32)
    poses2 = np.concatenate([g["init"], g["init"]])
    out2, st2 = pc.optimize(poses2, ij2, np.concatenate([g["meas"]] * 2), np.concatenate([g["info"]] * 2), fixed=150, max_iters=3)
    assert st2.status == 0 and st2.iterations == 3 and np.array_equal(out2[150], poses2[150])


# ---------------------------------------------------------------------------------------------------------------------------
# general SE(3) graphs (posegraph_oracle.make_graph_se3): the two references pinned to each other, and the floors that the
# tolerances of tests/test_gpu_posegraph_se3.py are ten times of (figures: tests/posegraph_se3.py)
# ---------------------------------------------------------------------------------------------------------------------------
import pytest  # noqa: E402

import posegraph_se3 as se3  # noqa: E402


@pytest.mark.parametrize("case", se3.LIN_CASES, ids=lambda c: "n%d_seed%d_fixed%d%s" % (c[0], c[2], c[3], "_iso" if c[4] else ""))
def test_se3_linearisation_of_the_two_oracles_agrees(case):
    """Analytic Jacobians + envelope assembly against central differences + scipy assembly on random rotations, reversed and
    duplicated edges, both quaternion hemispheres, dense information matrices and fixed in {0, middle, last}.  Measured over
    these cases: H 1.8e-10 max|H|, b 3.1e-10 max|b|, chi2 6.6e-15; asserted at the recorded O2O_* (the finite-difference
    error of the numpy oracle, see test_se3_finite_difference_floor)."""
    g = se3.graph(case)
    d = se3.differences(se3.c_system(g), se3.np_system(g))
    print(case, d)
    assert d["h"] <= se3.O2O_H and d["b"] <= se3.O2O_B and d["chi2"] <= se3.O2O_CHI2, d
    c = se3.c_system(g)
    f = g["fixed"]
    assert np.array_equal(c["diag"][f], np.eye(6)) and not c["b"][6 * f:6 * f + 6].any()
    assert not c["off"][(c["off_ij"] == f).any(1)].any()
    if g["isolated"] is not None:
        assert not c["diag"][g["isolated"]].any() and not (g["ij"] == g["isolated"]).any()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("fixed", [0, 32, 63])
def test_se3_damped_solve_of_the_two_oracles_agrees(seed, fixed):
    """Envelope Cholesky against SuperLU at a small and a large lambda.  Measured: at most 1.3e-8 |dx| (lambda = 1e-6 max
    diag H, condition 1e6) and 7.8e-10 |dx| (lambda = 1e-2 max diag H) in the 2-norm -- the Jacobians' 3e-10 through the
    condition number; asserted at 5e-8 / 5e-9."""
    g = po.make_graph_se3(64, 100, seed, fixed=fixed)
    H, b, c2 = po.linearize(g["init"], g["ij"], g["meas"], g["info"])
    for rel_lam, bound in ((1e-6, 5e-8), (1e-2, 5e-9)):
        lam = rel_lam * H.diagonal().max()
        dx = pc.solve(g["init"], g["ij"], g["meas"], g["info"], lam, fixed=fixed)
        ref = po.solve_damped(H, b, lam, fixed)
        assert not dx[6 * fixed:6 * fixed + 6].any()
        assert np.linalg.norm(dx - ref) <= bound * np.linalg.norm(ref)


@pytest.mark.parametrize("lm", se3.LM_CASES, ids=lambda c: "%s_seed%d_fixed%d" % c[:3])
def test_se3_lm_runs_of_the_two_oracles_agree(lm):
    """The LM runs that the GPU is compared with: both oracles take the same trials in every iteration of the prefix, chi2
    falls by more than 1e-9 of itself in each, and the sequence survives damped solves that stop at the PCG's residual.
    Measured between the oracles: poses within 2.1e-9 (mild: 1.3e-9), chi2 within 1.6e-14 relative."""
    start, seed, fixed, iters = lm
    g = se3.lm_graph(start, seed, fixed)
    r = se3.lm_references(g, iters)
    print(lm, r["np_trials"], r["clamped"], np.abs(r["np_poses"] - r["c_poses"]).max(), r["pcg_spread"], r["path"])
    assert r["np_trials"] == r["c_trials"] and r["pcg_same_trials"]
    assert all(r["chi2"][k] - r["chi2"][k + 1] > 1e-9 * r["chi2"][k] for k in range(iters))
    assert r["c_stats"].status == 0 and r["c_stats"].iterations == iters
    assert np.abs(r["np_poses"] - r["c_poses"]).max() <= 1e-8
    assert abs(r["c_stats"].chi2_final - r["chi2"][-1]) <= 1e-12 * r["chi2"][-1]
    assert np.array_equal(r["c_poses"][fixed], g["init"][fixed])
    if start == "gross":
        assert r["clamped"] > 0  # the |dq| > 1 -> identity branch of fromVectorMQT ran


def test_se3_lm_cases_contain_rejected_trials():
    r = se3.lm_references(se3.lm_graph("gross", 1, 20), 16)
    assert r["np_trials"] == [1] * 9 + [4] + [1] * 6 and r["clamped"] > 0


def test_se3_finite_difference_floor():
    """numeric_jacobians at h = 1e-6 against h / 2: measured 3.4e-10 of the largest Jacobian entry (1.5e-8 absolute at a
    scale of 44) -- the numpy oracle's own error, which the oracle-to-oracle figures above are made of."""
    g = po.make_graph_se3(80, 127, 0)
    Ja, Jb = po.numeric_jacobians(g["init"], g["ij"], g["meas"], h=1e-6)
    Jc, Jd = po.numeric_jacobians(g["init"], g["ij"], g["meas"], h=0.5e-6)
    scale = max(np.abs(Ja).max(), np.abs(Jb).max())
    err = max(np.abs(Ja - Jc).max(), np.abs(Jb - Jd).max()) / scale
    print("finite-difference floor", err, "scale", scale)
    assert err <= se3.FD_REL


@pytest.mark.parametrize("case", [c for c in se3.LIN_CASES if c[3] == c[0] // 2],
                         ids=lambda c: "n%d_seed%d" % (c[0], c[2]))
def test_se3_summation_order_floor(case):
    """The C oracle against itself with its edges permuted (eight permutations): the fp64 rounding spread of the reference
    alone.  Measured: diag 4.1e-16, off 2.2e-16, b 4.2e-16, chi2 3.2e-15 (relative to max|diag|, max|off|, max|b|, chi2);
    asserted at the recorded SPREAD_*, which the GPU comparison takes ten times."""
    g = se3.graph(case)
    ref = se3.c_system(g)
    rng = np.random.default_rng(100 + case[2])
    for _ in range(8):
        d = se3.differences(se3.c_system(g, order=rng.permutation(len(g["ij"]))), ref)
        print(case, d)
        assert d["diag"] <= se3.SPREAD_H and d["off"] <= se3.SPREAD_H and d["b"] <= se3.SPREAD_B and d["chi2"] <= se3.SPREAD_CHI2, d


@pytest.mark.parametrize("case", [c for c in se3.LIN_CASES if c[0] >= 64], ids=lambda c: "n%d_seed%d_fixed%d" % (c[0], c[2], c[3]))
def test_se3_generator_covers_what_the_planar_family_never_does(case):
    g = se3.graph(case)
    ij, n = g["ij"], case[0]
    assert set(g) >= set(po.make_graph(n_kf=20, n_loop=5)) and g["fixed"] == case[3]
    rev = int((ij[:, 0] > ij[:, 1]).sum())
    assert 0.3 * len(ij) < rev < 0.7 * len(ij)                     # i > j edges
    w = se3.raw_edge_quaternion_w(g)
    assert 0.2 * len(ij) < int((w < 0).sum()) < 0.8 * len(ij)      # sgn = -1 in edge_error
    assert (g["init"][:, 6] < 0).any() and (g["meas"][:, 6] < 0).any()
    directed = {}
    for a, b in ij.tolist():
        directed[(a, b)] = directed.get((a, b), 0) + 1
    assert any(c > 1 for c in directed.values())                    # parallel duplicate
    assert any((b, a) in directed for (a, b) in directed)           # antiparallel pair
    assert len(se3.pairs_of(ij)) < len(ij)
    assert int((ij[g["n_odo"]:] == g["fixed"]).any(1).sum()) >= 1  # an extra edge at the fixed vertex
    e = po.edge_error(g["init"], ij, g["meas"])
    assert np.linalg.norm(e[:, 3:], axis=1).max() > 0.1             # rotation errors far from the identity
    info = g["info"]
    assert np.array_equal(info, np.transpose(info, (0, 2, 1)))      # exactly symmetric,
    assert np.abs(info - info * np.eye(6)).max() > 1.0              # dense,
    assert np.linalg.eigvalsh(info).min() > 0.4                     # positive definite
    assert np.abs(np.linalg.norm(g["init"][:, 3:], axis=1) - 1).max() < 1e-15
    if case[4]:
        assert g["isolated"] is not None and g["isolated"] != g["fixed"] and not (ij == g["isolated"]).any()


def test_load_honours_the_fix_vertex_of_the_file(pkg, tmp_path):
    """A .g2o file that fixes a vertex other than the first: PoseGraph.load() must pass that vertex to lslam_pg_create
    (it used to read the file's FIX and pin vertex 0 regardless).  A file without FIX keeps the first vertex."""
    edge = " 1 0 0 0 0 0 1 " + " ".join("1" if k in (0, 6, 11, 15, 18, 20) else "0" for k in range(21)) + "\n"
    txt = "".join("VERTEX_SE3:QUAT %d %d 0 0 0 0 0 1\n" % (10 + k, k) for k in range(4))
    txt += "".join("EDGE_SE3:QUAT %d %d" % (10 + k, 11 + k) + edge for k in range(3))
    f = tmp_path / "fix2.g2o"
    f.write_text(txt + "FIX 12\n")
    pg = pkg.PoseGraph(0)
    g = pg.load(f)
    assert g["fixed"] == 2 and pg.fixed == 2
    f0 = tmp_path / "nofix.g2o"
    f0.write_text(txt)
    g0 = pg.load(f0)
    assert g0["fixed"] == -1 and pg.fixed == 0
    pg.set_graph(g["poses"], g["ij"], g["meas"], g["info"], fixed=3)
    assert pg.fixed == 3
    pg.set_graph(g["poses"], g["ij"], g["meas"], g["info"])
    assert pg.fixed == 0
    with pytest.raises(ValueError):
        pg.set_graph(g["poses"], g["ij"], g["meas"], g["info"], fixed=4)
