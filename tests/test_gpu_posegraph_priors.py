"""csrc/lslam_posegraph.hip's unary constraints (lslam_pg_set_priors: GPS position and absolute-pose priors) against the CPU
reference tests/posegraph_prior_ref.py.  Parity with the reference stays unpinned (neither g2o nor hdl_graph_slam is
available); the semantics are their published ones, as the reference module restates them.

Every tolerance is ten times a floor of the references themselves, measured on the CPU by tests/test_posegraph_prior_ref.py
(and the earlier CPU suites) and recorded in tests/posegraph_prior_ref.py, posegraph_se3.py and robust_posegraph_ref.py; none
was calibrated against what the kernels return.  Each test prints its figures before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest

import posegraph_prior_ref as ppr
import posegraph_se3 as se3
import robust_posegraph_ref as rr

po, pc = se3.po, se3.pc
INVALID = -1  # LSLAM_ERR_INVALID
SHARD_CASE = (65, 100, 5, 32, True)  # tests/test_gpu_posegraph_se3.py's


def _graph(pkg, g, pr=None, fixed=None):
    pg = pkg.PoseGraph(0)
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"], fixed=g["fixed"] if fixed is None else fixed, priors=pr)
    return pg


def _in_pair_order(s):
    o = np.lexsort((s["off_ij"][:, 1], s["off_ij"][:, 0]))
    return dict(diag=s["diag"], off=s["off"][o], off_ij=s["off_ij"][o].astype(np.int32).reshape(-1, 2), b=s["b"], chi2=s["chi2"])


def _bits(s):
    return tuple(np.ascontiguousarray(s[k]).view(np.int64).tobytes() for k in ("diag", "off", "b")) + (np.float64(s["chi2"]).tobytes(),)


def _assert_system(got, g, pr, fixed):
    """against both references: 10 x SPREAD_* (C oracle) and 10 x O2O_* (numpy oracle) -- the weighted system too: its measured
    floor, (e) of posegraph_prior_ref's docstring, is inside the plain one's"""
    sc, sn = ppr.prior_system(g, pr, oracle="c", fixed=fixed), ppr.prior_system(g, pr, oracle="np", fixed=fixed)
    dc, dn = ppr.differences(got, sc), ppr.differences(got, sn)
    print("against C", dc, "against numpy", dn)
    assert dc["diag"] <= 10 * se3.SPREAD_H and dc["off"] <= 10 * se3.SPREAD_H, dc
    assert dc["b"] <= 10 * se3.SPREAD_B and dc["chi2"] <= 10 * se3.SPREAD_CHI2, dc
    assert dn["h"] <= 10 * se3.O2O_H and dn["b"] <= 10 * se3.O2O_B and dn["chi2"] <= 10 * se3.O2O_CHI2, dn
    return sc


# ---- linearisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ppr.LIN_PRIOR_CASES)
def test_prior_linearize_matches_both_references(pkg, name):
    """diag, off, b and chi2 of graphs with priors (sizes 1, 2, 7, 65, 400; XYZ, POSE, mixed, up to three priors on a vertex, a
    prior on the fixed vertex, fixed = -1, orientation-only information, both hemispheres of q_e, 300 priors = three blocks of
    pg_prior_kernel).  The C reference holds the POSE priors as edges of the augmented graph."""
    g, pr, fixed = ppr.lin_case(name)
    pg = _graph(pkg, g, pr, fixed)
    assert pg.num_priors == len(pr["vertex"])
    got = _in_pair_order(pg.linearize())
    plain_chi2 = pg.robust_info()["chi2_plain"]  # keeps its meaning: edges only
    pg.close()
    _assert_system(got, g, pr, fixed)
    if fixed >= 0:  # identity block, zero right-hand side -- whatever sits on the fixed vertex
        assert np.array_equal(got["diag"][fixed], np.eye(6)) and not got["b"][6 * fixed:6 * fixed + 6].any()
    edges_chi2 = po.chi2(g["init"], g["ij"], g["meas"], g["info"]) if len(g["ij"]) else 0.0
    assert abs(plain_chi2 - edges_chi2) <= 10 * se3.O2O_CHI2 * max(edges_chi2, 1e-300)
    if len(g["ij"]) == 0:  # n = 1: the system IS the prior's record
        assert np.abs(got["diag"][0]).max() > 0 and not got["diag"][0][3:].any() and not got["diag"][0][:, 3:].any()


@pytest.mark.gpu
def test_prior_on_the_fixed_vertex_adds_only_to_chi2(pkg):
    g, pr, fixed = ppr.lin_case("n7_pose_fixed")
    on_fixed = pr["vertex"] == fixed
    assert on_fixed.any()
    with_all, without = _graph(pkg, g, pr, fixed), _graph(pkg, g, ppr.permuted(pr, np.nonzero(~on_fixed)[0]), fixed)
    a, b = with_all.linearize(), without.linearize()
    with_all.close()
    without.close()
    e2 = ppr.prior_e2(g["init"], pr)[on_fixed].sum()
    print("chi2 with %.17g without %.17g reference e2 of the prior on the fixed vertex %.17g" % (a["chi2"], b["chi2"], e2))
    assert np.array_equal(a["diag"], b["diag"]) and np.array_equal(a["b"], b["b"]) and np.array_equal(a["off"], b["off"])
    assert abs((a["chi2"] - b["chi2"]) - e2) <= 10 * se3.SPREAD_CHI2 * a["chi2"]


# ---- robust kernels on priors ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n65_mixed", "n65_free_pose", "n400_many"])
def test_prior_robust_values_and_weighted_system(pkg, name):
    """lslam_pg_prior_robust (e2, rho0, rho1) against robust_posegraph_ref.rho on the reference's e2 for every kernel, priors on
    both sides of each threshold (asserted on the reference alone), and the weighted system.  Per prior 10 x W_EDGE_*."""
    g, pr, fixed = ppr.lin_case(name)
    q = ppr.prior_kernel_mix(g, pr)
    e2, r0, r1 = ppr.prior_rho(g["init"], q)
    sides = rr.sides(q["kernels"], q["deltas"], e2)
    assert all(a > 0 and b > 0 for a, b in sides.values()), sides
    pg = _graph(pkg, g, q, fixed)
    tap = pg.prior_robust()
    at = pg.prior_robust(g["gt"])  # at caller-supplied poses
    got = _in_pair_order(pg.linearize())
    pg.close()
    de, dr, dw = (np.abs(tap["e2"] - e2) / e2).max(), (np.abs(tap["rho"] - r0) / r0).max(), (np.abs(tap["weight"] - r1) / r1).max()
    e2g, r0g, r1g = ppr.prior_rho(g["gt"], q)
    de_g = (np.abs(at["e2"] - e2g) / e2g).max()
    print(name, "sides", sides, "e2 %.3e rho0 %.3e weight %.3e; at gt e2 %.3e" % (de, dr, dw, de_g))
    assert de <= 10 * rr.W_EDGE_E2 and dr <= 10 * rr.W_EDGE_RHO and dw <= 10 * rr.W_EDGE_WEIGHT
    assert de_g <= 10 * rr.W_EDGE_E2 and (np.abs(at["weight"] - r1g) / r1g).max() <= 10 * rr.W_EDGE_WEIGHT
    assert (tap["weight"][q["kernels"] == rr.NONE] == 1.0).all() and (tap["weight"] < 1.0).any()
    _assert_system(got, g, q, fixed)


# ---- LM ----------------------------------------------------------------------------------------------------------------------
def _lm_bound(r, cpu_cpu):
    """the construction of test_se3_lm_trajectory_matches_both_oracles"""
    return max(10 * cpu_cpu, 10 * r["pcg_spread"], se3.PCG_TOL * r["path"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ppr.LM_POSE_CASES, ids=lambda c: "%s_seed%d" % c[:2])
def test_lm_with_pose_priors_follows_the_c_oracle_on_the_augmented_graph(pkg, case):
    """40 vertices, fixed = -1, POSE priors on three vertices: iteration count, per-iteration trial counts (through the totals of
    runs of 1 .. k iterations), chi2 and poses against posegraph_oracle.c's LM on the augmented graph (its extra vertex fixed)
    and the numpy LM.  Pose bound: max(10 x the two references' disagreement, 10 x the numpy LM's spread under solves that stop
    at the PCG's residual, 1e-8 x path length)."""
    start, seed, iters = case
    g, pr = ppr.lm_case(start, seed, ppr.POSE)
    r = ppr.lm_run(g, pr, -1, iters)
    cp, ct, cst = ppr.c_lm_augmented(g, pr, iters)
    assert r["trials"] == ct and r["pcg_same_trials"], "inputs unusable: the references disagree"
    cum = []
    for k in range(1, iters + 1):
        pg = _graph(pkg, g, pr, -1)
        its = pg.optimize(k)
        cum.append(pg.last_stats.lm_trials)
        if k < iters:
            pg.close()
    st, got = pg.last_stats, pg.poses()
    pg.close()
    gpu_trials = list(np.diff([0] + cum))
    cpu_cpu = float(np.abs(cp - r["poses"]).max())
    tol = _lm_bound(r, cpu_cpu)
    tol_chi = 10 * max(abs(cst.chi2_final - r["chi2"][-1]) / r["chi2"][-1], r["pcg_chi2_spread"], se3.SPREAD_CHI2)
    err_c, err_n = float(np.abs(got - cp).max()), float(np.abs(got - r["poses"]).max())
    print(case, "trials gpu", gpu_trials, "reference", ct, "pose error C %.3e numpy %.3e bound %.3e (cpu-cpu %.3e pcg %.3e path %.3e)" % (
        err_c, err_n, tol, cpu_cpu, r["pcg_spread"], r["path"]), "chi2 %.17g / %.17g bound %.3e" % (st.chi2_final, cst.chi2_final, tol_chi))
    assert its == iters == cst.iterations and gpu_trials == ct
    assert abs(st.chi2_initial - cst.chi2_initial) <= 10 * se3.SPREAD_CHI2 * cst.chi2_initial
    assert abs(st.chi2_final - cst.chi2_final) <= tol_chi * cst.chi2_final
    assert err_c <= tol and err_n <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("case", ppr.LM_XYZ_CASES, ids=lambda c: "%s_seed%d" % c[:2])
def test_lm_with_xyz_priors_follows_the_numpy_lm(pkg, case):
    """The same graphs with five XYZ priors and no fixed vertex against the numpy reference LM (the prefix was chosen on the CPU:
    tests/test_posegraph_prior_ref.py).  Only one reference exists here, so the pose bound is max(10 x its spread under solves
    that stop at the PCG's residual, 1e-8 x path length)."""
    start, seed, iters = case
    g, pr = ppr.lm_case(start, seed, ppr.XYZ)
    r = ppr.lm_run(g, pr, -1, iters)
    assert r["pcg_same_trials"]
    pg = _graph(pkg, g, pr, -1)
    its = pg.optimize(iters)
    st, got = pg.last_stats, pg.poses()
    pg.close()
    tol = _lm_bound(r, 0.0)
    tol_chi = 10 * max(r["pcg_chi2_spread"], se3.O2O_CHI2)
    err = float(np.abs(got - r["poses"]).max())
    print(case, "trials gpu", st.lm_trials, "reference", r["trials"], "pose error %.3e bound %.3e" % (err, tol),
          "chi2 %.17g / %.17g bound %.3e" % (st.chi2_final, r["chi2"][-1], tol_chi))
    assert its == iters and st.lm_trials == sum(r["trials"])
    assert abs(st.chi2_initial - r["chi2"][0]) <= 10 * se3.O2O_CHI2 * r["chi2"][0]
    assert abs(st.chi2_final - r["chi2"][-1]) <= tol_chi * r["chi2"][-1]
    assert err <= tol


@pytest.mark.gpu
def test_gps_outlier_is_rejected_by_cauchy_and_pulls_without(pkg):
    """Odometry-only lap, a fix on every third keyframe, one displaced by 50 sigma.  The statements are asserted on the
    reference first, then on the solver: with Cauchy the outlier's weight falls below 0.1 and the others stay above 0.9; with
    no kernel the trajectory is pulled (largest position error more than twice the robust run's)."""
    ref_p, ref_c = ppr.gps_reference(None), ppr.gps_reference("cauchy")
    assert ref_c["weights"][ppr.GPS_OUTLIER] < 0.1 and np.delete(ref_c["weights"], ppr.GPS_OUTLIER).min() > 0.9
    assert ref_p["err"] > 2 * ref_c["err"]
    out = {}
    for kernel in (None, "cauchy"):
        g, pr = ppr.gps_scenario(kernel)
        pg = _graph(pkg, g, pr, -1)
        pg.optimize(ppr.GPS_ITERS)
        P = pg.poses()
        out[kernel] = dict(err=float(np.linalg.norm(P[:, :3] - g["gt"][:, :3], axis=1).max()), w=pg.prior_robust()["weight"])
        pg.close()
    w = out["cauchy"]["w"]
    print("gpu: outlier weight %.3e others min %.4f; position error plain %.3f m (reference %.3f) Cauchy %.3f m (reference %.3f)" % (
        w[ppr.GPS_OUTLIER], np.delete(w, ppr.GPS_OUTLIER).min(), out[None]["err"], ref_p["err"], out["cauchy"]["err"], ref_c["err"]))
    assert w[ppr.GPS_OUTLIER] < 0.1 and np.delete(w, ppr.GPS_OUTLIER).min() > 0.9
    assert (out[None]["w"] == 1.0).all()
    assert out[None]["err"] > 2 * out["cauchy"]["err"]


# ---- sharding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_edge_shards_count_every_prior_once(pkg):
    """SHARD_CASE with priors, shards (0, cut) and (cut, ne), no all-reduce (each shard's raw contribution): the host sum equals
    the full system within the existing sharded bounds (10 x SPREAD_*), and the second shard -- which carries no prior --
    gives the diagonal blocks, b and chi2 of the same shard on a graph without priors BIT FOR BIT."""
    g = se3.graph(SHARD_CASE)
    _, pr, _ = ppr.lin_case("n65_mixed")  # the same graph
    ne = len(g["ij"])
    cut = ne // 2

    def system(priors, shard=None):
        pg = _graph(pkg, g, priors)
        if shard is not None:
            pg.set_shard(*shard)
        s = pg.linearize()
        pg.close()
        return s
    full = system(pr)
    lo, hi, hi_plain = system(pr, (0, cut)), system(pr, (cut, ne)), system(None, (cut, ne))
    d = lo["diag"] + hi["diag"]
    d[g["fixed"]] = np.eye(6)
    summed = dict(diag=d, off=lo["off"] + hi["off"], off_ij=full["off_ij"], b=lo["b"] + hi["b"], chi2=lo["chi2"] + hi["chi2"])
    diff = ppr.differences(summed, full)
    print("sharded against full", diff)
    assert diff["diag"] <= 10 * se3.SPREAD_H and diff["off"] <= 10 * se3.SPREAD_H
    assert diff["b"] <= 10 * se3.SPREAD_B and diff["chi2"] <= 10 * se3.SPREAD_CHI2
    assert _bits(hi) == _bits(hi_plain)
    assert lo["chi2"] > system(None, (0, cut))["chi2"]  # ... and the first shard does carry them


# ---- no priors, no change ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_graph_without_priors_is_bit_identical(pkg):
    """linearize and optimize of a graph with no priors: before and after set_priors(n > 0) followed by set_priors(0), and
    against a fresh graph."""
    g, pr, fixed = ppr.lin_case("n65_mixed")
    pg = _graph(pkg, g)
    before = pg.linearize()
    pg.set_priors(pr)
    assert pg.num_priors == len(pr["vertex"]) and _bits(pg.linearize()) != _bits(before)
    pg.set_priors(None)
    assert pg.num_priors == 0
    after = pg.linearize()
    pg.optimize(5)
    poses = pg.poses()
    pg.close()
    fresh = _graph(pkg, g)
    fresh_sys = fresh.linearize()
    fresh.optimize(5)
    fresh_poses = fresh.poses()
    fresh.close()
    assert _bits(before) == _bits(after) == _bits(fresh_sys)
    assert np.array_equal(poses.view(np.int64), fresh_poses.view(np.int64))


# ---- validation --------------------------------------------------------------------------------------------------------------
def _bad_inputs(n_v):
    """name -> (vertex, type, meas, info, kind, delta) with exactly one defect"""
    def base():
        return dict(vertex=np.array([1, 2], np.int32), type=np.array([ppr.XYZ, ppr.POSE], np.int32),
                    meas=np.tile(ppr.IDENT, (2, 1)), info=np.tile(np.eye(6), (2, 1, 1)), kind=None, delta=None)
    out = {}
    for name, edit in [
            ("vertex_high", lambda p: p["vertex"].__setitem__(0, n_v)),
            ("vertex_negative", lambda p: p["vertex"].__setitem__(1, -1)),
            ("unknown_type", lambda p: p["type"].__setitem__(0, 2)),
            ("nan_position", lambda p: p["meas"].__setitem__((0, 1), np.nan)),
            ("inf_quaternion", lambda p: p["meas"].__setitem__((1, 4), np.inf)),
            ("zero_quaternion", lambda p: p["meas"].__setitem__((1, slice(3, 7)), 0.0)),
            ("nan_information", lambda p: p["info"].__setitem__((0, 1, 1), np.nan)),
            ("asymmetric_information", lambda p: p["info"].__setitem__((1, 0, 4), 0.5)),
            ("negative_diagonal", lambda p: p["info"].__setitem__((0, 2, 2), -1.0)),
            ("kind_without_delta", lambda p: p.__setitem__("kind", np.array([1, 0], np.int32))),
            ("delta_without_kind", lambda p: p.__setitem__("delta", np.array([1.0, 1.0]))),
            ("zero_delta", lambda p: (p.__setitem__("kind", np.array([1, 0], np.int32)), p.__setitem__("delta", np.array([0.0, 1.0])))),
            ("nan_delta", lambda p: (p.__setitem__("kind", np.array([0, 2], np.int32)), p.__setitem__("delta", np.array([1.0, np.nan])))),
            ("unknown_kind", lambda p: (p.__setitem__("kind", np.array([4, 0], np.int32)), p.__setitem__("delta", np.array([1.0, 1.0]))))]:
        p = base()
        edit(p)
        out[name] = p
    return out


@pytest.mark.gpu
def test_every_rejected_input_returns_invalid_and_changes_nothing(pkg):
    g, pr, fixed = ppr.lin_case("n7_xyz")
    pg = _graph(pkg, g, pr, fixed)
    ref = _bits(pg.linearize())
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(p):
        k = p["kind"].ctypes.data_as(ip) if p["kind"] is not None else None
        d = p["delta"].ctypes.data_as(dp) if p["delta"] is not None else None
        return pg.lib.lslam_pg_set_priors(pg.h, 2, p["vertex"].ctypes.data_as(ip), p["type"].ctypes.data_as(ip), p["meas"].ctypes.data_as(dp),
                                          np.ascontiguousarray(p["info"]).ctypes.data_as(dp), k, d)
    for name, p in _bad_inputs(len(g["init"])).items():
        rc = call(p)
        msg = pg.lib.lslam_pg_last_error().decode()
        print(name, rc, msg)
        assert rc == INVALID and msg, name
        assert pg.num_priors == len(pr["vertex"]) and _bits(pg.linearize()) == ref, name
    # what is NOT used is not checked: junk outside an XYZ prior's 3x3 and in its quaternion
    ok = dict(vertex=np.array([1], np.int32), type=np.array([ppr.XYZ], np.int32), meas=np.array([[1.0, 2, 3, np.nan, 0, 0, 0]]),
              info=np.full((1, 6, 6), np.nan), kind=None, delta=None)
    ok["info"][0, :3, :3] = np.eye(3)
    assert pg.lib.lslam_pg_set_priors(pg.h, 1, ok["vertex"].ctypes.data_as(ip), ok["type"].ctypes.data_as(ip), ok["meas"].ctypes.data_as(dp),
                                      ok["info"].ctypes.data_as(dp), None, None) == 0
    s = pg.linearize()
    assert pg.num_priors == 1 and np.isfinite(s["diag"]).all() and np.isfinite(s["chi2"])
    pg.close()


# ---- g2o files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_g2o_round_trip_reproduces_the_system_bit_for_bit(pkg, tmp_path):
    """save -> lslam_g2o_read + lslam_g2o_read_priors -> create: the same system bit for bit (17 significant digits); and
    lslam_g2o_read alone on that file returns the plain graph."""
    for name in ("n65_mixed", "n65_free_pose"):
        g, pr, fixed = ppr.lin_case(name)
        pr = dict(pr, info=ppr.used_info(pr))  # what the file can carry of an XYZ prior: its 3x3
        pg = _graph(pkg, g, pr, fixed)
        ref = pg.linearize()
        path = str(tmp_path / (name + ".g2o"))
        pg.save(path)
        pg.close()
        text = open(path).read()
        assert text.count("PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1\n") == 1
        assert text.count("EDGE_SE3_PRIOR ") == int((pr["type"] == ppr.POSE).sum()) and text.count("EDGE_SE3_PRIORXYZ ") == int((pr["type"] == ppr.XYZ).sum())
        assert ("FIX %d\n" % fixed in text) == (fixed >= 0)
        back = pkg.PoseGraph.read_g2o(path)
        assert np.array_equal(back["ij"], g["ij"]) and back["fixed"] == fixed
        assert np.array_equal(back["poses"].view(np.int64), np.ascontiguousarray(g["init"]).view(np.int64))
        assert np.array_equal(back["priors"]["vertex"], pr["vertex"]) and np.array_equal(back["priors"]["type"], pr["type"])
        pg2 = pkg.PoseGraph(0)
        pg2.load(path)
        assert pg2.fixed == fixed and pg2.num_priors == len(pr["vertex"])
        again = pg2.linearize()
        pg2.close()
        assert _bits(again) == _bits(ref), name
        plain = _graph(pkg, dict(g, init=back["poses"], ij=back["ij"], meas=back["meas"], info=back["info"]), None, max(fixed, 0))
        want = _graph(pkg, g, None, max(fixed, 0))
        assert _bits(plain.linearize()) == _bits(want.linearize())
        plain.close()
        want.close()


@pytest.mark.gpu
def test_committed_fixture_loads_and_optimizes(pkg):
    """tests/golden/posegraph_priors.g2o (hand-written, both new tags, no FIX line): load() keeps the priors and lets them fix
    the gauge; the system is the reference's and LM lowers chi2."""
    path = os.path.join(se3.ROOT, "tests", "golden", "posegraph_priors.g2o")
    pg = pkg.PoseGraph(0)
    f = pg.load(path)
    assert pg.fixed == -1 and pg.num_priors == 4
    g = dict(init=f["poses"], ij=f["ij"], meas=f["meas"], info=f["info"], fixed=-1)
    pr = dict(f["priors"], kernels=np.zeros(4, np.int32), deltas=np.ones(4))
    got = _in_pair_order(pg.linearize())
    _assert_system(got, g, pr, -1)
    pg.optimize(10)
    st = pg.last_stats
    pg.close()
    print("fixture chi2 %.6g -> %.6g" % (st.chi2_initial, st.chi2_final))
    assert st.chi2_final < st.chi2_initial
