"""Robust kernels on pose-graph edges (csrc/lslam_posegraph.hip: pg_edge_robust_kernel, pg_chi2_robust_kernel,
pg_edge_robust_tap_kernel) against tests/robust_posegraph_ref.py.  Parity with g2o is unpinned (it is not available); the
reference restates its published formulas.  Every tolerance is ten times a floor of the reference itself, measured on the CPU
by tests/test_robust_posegraph_ref.py and recorded in the reference module; none was calibrated against what the kernels
return.  Each test prints its figures before it asserts."""
import subprocess

import numpy as np
import pytest

import posegraph_se3 as se3
import robust_posegraph_ref as rr

po = se3.po
LIN = [(2, 1, 0, 0, False), (7, 6, 3, 3, True), (64, 100, 4, 32, False), (65, 100, 5, 0, True), (400, 600, 6, 399, False)]
assert all(c in se3.LIN_CASES for c in LIN)
_ids = lambda c: "n%d_seed%d_fixed%d%s" % (c[0], c[2], c[3], "_iso" if c[4] else "")  # noqa: E731


def _graph_on_gpu(pkg, g, kinds=None, deltas=None, shard=None):
    pg = pkg.PoseGraph(0)
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"], fixed=g["fixed"], kernels=kinds, deltas=deltas)
    if shard is not None:
        pg.set_shard(*shard)  # no all-reduce: this shard's raw contribution
    return pg


def _in_pair_order(s):
    o = np.lexsort((s["off_ij"][:, 1], s["off_ij"][:, 0]))
    return dict(diag=s["diag"], off=s["off"][o], off_ij=s["off_ij"][o].astype(np.int32), b=s["b"], chi2=s["chi2"])


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---- 1. linearise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", LIN, ids=_ids)
def test_weighted_linearize_matches_both_oracles(pkg, case):
    """Edge e carries kind e % 4 (NONE, Huber, Cauchy, DCS), delta from the median of the reference's e2 at the initial estimate
    (Huber, Cauchy: sqrt(median); DCS: median), so for n >= 64 every kind has edges on both sides of its threshold.
    PoseGraph.linearize() against weighted_system through the C oracle -- ten times floor (a): 3e-15 max|diag|, 3e-15
    max|off|, 2e-15 max|b|, 3.5e-15 sum rho0 -- and through the numpy oracle -- ten times floor (b): 1.6e-9 max|H|, 1.4e-9
    max|b|, 2.5e-14 sum rho0.  Fixed and isolated vertices as in test_se3_linearize_matches_both_oracles."""
    g = se3.graph(case)
    kinds, deltas = rr.kernel_mix(g)
    refc = rr.weighted_system(g, kinds, deltas)
    refn = rr.weighted_system(g, kinds, deltas, oracle="np")
    if case[0] >= 64:
        sd = rr.sides(kinds, deltas, refn["e2"])
        assert all(min(v) >= 1 for v in sd.values()), sd
    pg = _graph_on_gpu(pkg, g, kinds, deltas)
    s = pg.linearize()
    pg.close()
    got = _in_pair_order(s)
    assert sorted(tuple(p) for p in s["off_ij"].tolist()) == [tuple(p) for p in se3.pairs_of(g["ij"]).tolist()]
    f = g["fixed"]
    assert np.array_equal(got["diag"][f], np.eye(6)) and not got["b"][6 * f:6 * f + 6].any()
    assert not got["off"][(got["off_ij"] == f).any(1)].any()
    if g["isolated"] is not None:
        assert not got["diag"][g["isolated"]].any() and not got["b"][6 * g["isolated"]:6 * g["isolated"] + 6].any()
    dc, dn = se3.differences(got, refc), se3.differences(got, refn)
    print("case", case, "against C oracle", dc, "against numpy oracle", dn)
    assert dc["diag"] <= 10 * rr.W_SPREAD_H and dc["off"] <= 10 * rr.W_SPREAD_H, dc
    assert dc["b"] <= 10 * rr.W_SPREAD_B and dc["chi2"] <= 10 * rr.W_SPREAD_CHI2, dc
    assert dn["h"] <= 10 * rr.W_O2O_H and dn["b"] <= 10 * rr.W_O2O_B and dn["chi2"] <= 10 * rr.W_O2O_CHI2, dn
    # the kernels did something: the weighted system is not the plain one
    if case[0] >= 64:
        assert se3.differences(got, se3.c_system(g))["diag"] > 1e-3


# ---- 2. per-edge tap ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", [LIN[1], LIN[2], LIN[4]], ids=_ids)
def test_edge_tap_matches_the_reference_per_edge(pkg, case):
    """edge_robust() at the current estimate and at caller-supplied poses (the estimate moved by a random step of 0.3 m / 0.05
    in the quaternion vector per vertex: other poses with errors of the size the floors were measured at -- at the ground truth
    the errors are the 0.05 m measurement noise, differences of 10 m positions, and no evaluation of e2 keeps 3.5e-14 there)
    against the reference per edge: e2 within 10 x SPREAD_CHI2 = 3.5e-14 relative, rho0 within 10 x W_EDGE_RHO = 2e-13, weight within
    10 x W_EDGE_WEIGHT = 5e-14 (the per-edge figures of floor (a)).  robust_info() counts what the tap shows."""
    g = se3.graph(case)
    kinds, deltas = rr.kernel_mix(g)
    pg = _graph_on_gpu(pkg, g, kinds, deltas)
    rng = np.random.default_rng(case[2])
    n = len(g["init"])
    moved = po.oplus(g["init"], np.concatenate([rng.normal(0, 0.3, (n, 3)), rng.normal(0, 0.05, (n, 3))], 1).ravel(), g["fixed"])
    for name, poses in (("estimate", None), ("supplied", moved)):
        t = pg.edge_robust(poses)
        e2 = rr.edge_e2(g, poses)
        r0, r1 = rr.rho_edges(kinds, deltas, e2)
        d = [float(np.abs(a / b - 1).max()) for a, b in ((t["e2"], e2), (t["rho"], r0), (t["weight"], r1))]
        print(case, name, "e2 %.2e rho0 %.2e weight %.2e" % tuple(d))
        assert d[0] <= 10 * se3.SPREAD_CHI2 and d[1] <= 10 * rr.W_EDGE_RHO and d[2] <= 10 * rr.W_EDGE_WEIGHT, d
        assert np.array_equal(t["weight"][kinds == rr.NONE], np.ones((kinds == rr.NONE).sum()))
        assert _same_bits(t["rho"][kinds == rr.NONE], t["e2"][kinds == rr.NONE])
    assert np.abs(pg.edge_robust(moved)["e2"] / pg.edge_robust()["e2"] - 1).max() > 0.1  # the supplied poses were used
    assert _same_bits(pg.poses(), g["init"])                                             # ... and did not replace the estimate
    t, info = pg.edge_robust(), pg.robust_info()
    print(case, info)
    assert info["n_robust"] == int((kinds != rr.NONE).sum())
    assert info["n_downweighted"] == int(((kinds != rr.NONE) & (t["weight"] < 1)).sum()) > 0
    assert abs(info["chi2_plain"] - t["e2"].sum()) <= 10 * se3.SPREAD_CHI2 * t["e2"].sum()
    pg.clear_robust_kernels()
    t = pg.edge_robust()
    assert np.array_equal(t["weight"], np.ones(len(kinds))) and _same_bits(t["rho"], t["e2"])
    assert pg.robust_info()["n_robust"] == 0 and pg.robust_info()["n_downweighted"] == 0
    pg.close()


# ---- 3. shards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_edge_shards_sum_to_the_weighted_system(pkg):
    """n = 64, set_shard(0, ne / 2) and set_shard(ne / 2, ne) without an all-reduce: the kernel arrays are indexed by global
    edge id, each shard weights its own edges.  The raw contributions sum to the unsharded weighted system within the
    permutation spread bound (10 x 3e-16 of max|diag|, max|off|, 10 x 2e-16 of max|b|), their chi2 values to sum rho0 (10 x 3.5e-16)."""
    g = se3.graph(LIN[2])
    kinds, deltas = rr.kernel_mix(g)
    ne = len(kinds)
    cut = ne // 2
    out = []
    for shard in (None, (0, cut), (cut, ne)):
        pg = _graph_on_gpu(pkg, g, kinds, deltas, shard)
        out.append(pg.linearize())
        pg.close()
    full, lo, hi = out
    d = lo["diag"] + hi["diag"]
    d[g["fixed"]] = np.eye(6)
    summed = dict(diag=d, off=lo["off"] + hi["off"], off_ij=full["off_ij"], b=lo["b"] + hi["b"], chi2=lo["chi2"] + hi["chi2"])
    diff = se3.differences(summed, full)
    r0 = rr.weighted_system(g, kinds, deltas)["rho"]
    print("sharded against full", diff, "chi2 parts", lo["chi2"], hi["chi2"], "reference", r0[:cut].sum(), r0[cut:].sum())
    assert diff["diag"] <= 10 * rr.W_SPREAD_H and diff["off"] <= 10 * rr.W_SPREAD_H and diff["b"] <= 10 * rr.W_SPREAD_B
    assert diff["chi2"] <= 10 * rr.W_SPREAD_CHI2
    assert abs(lo["chi2"] - r0[:cut].sum()) <= 10 * rr.W_SPREAD_CHI2 * r0[:cut].sum()
    assert abs(hi["chi2"] - r0[cut:].sum()) <= 10 * rr.W_SPREAD_CHI2 * r0[cut:].sum()
    assert abs(summed["chi2"] - r0.sum()) <= 10 * rr.W_SPREAD_CHI2 * r0.sum()


# ---- 4. no behaviour change ------------------------------------------------------------------------------------------------------------
def _lin_and_lm(pg, iters=50):
    s = pg.linearize()
    its = pg.optimize(iters)
    st = pg.last_stats
    return s, dict(poses=pg.poses(), its=its, trials=st.lm_trials, chi0=st.chi2_initial, chi1=st.chi2_final, cg=st.cg_iterations)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [LIN[2], LIN[4]], ids=_ids)
def test_kernels_set_and_cleared_leave_the_plain_solver_bit_for_bit(pkg, case):
    """A PoseGraph whose kernels were set (and used) and then cleared against one that never had any: linearize() and
    optimize(50) -- poses, chi2, iterations, trials -- equal bit for bit.  Huber with delta = 1e150 on every edge (no e2
    reaches 1e300) gives the plain system within the permutation spread bound and the same iteration and trial counts."""
    g = se3.graph(case)
    kinds, deltas = rr.kernel_mix(g)
    plain = _graph_on_gpu(pkg, g)
    s0, r0 = _lin_and_lm(plain)
    plain.close()
    pg = _graph_on_gpu(pkg, g, kinds, deltas)
    sw = pg.linearize()
    assert not _same_bits(sw["diag"], s0["diag"])  # the kernels were live
    pg.clear_robust_kernels()
    s1, r1 = _lin_and_lm(pg)
    pg.close()
    for k in ("diag", "off", "b"):
        assert _same_bits(s1[k], s0[k]), k
    assert np.array_equal(s1["off_ij"], s0["off_ij"]) and s1["chi2"] == s0["chi2"]
    print(case, "plain", {k: v for k, v in r0.items() if k != "poses"}, "cleared", {k: v for k, v in r1.items() if k != "poses"})
    assert _same_bits(r1["poses"], r0["poses"])
    assert (r1["its"], r1["trials"], r1["chi0"], r1["chi1"], r1["cg"]) == (r0["its"], r0["trials"], r0["chi0"], r0["chi1"], r0["cg"])
    ne = len(kinds)
    hub = _graph_on_gpu(pkg, g, np.full(ne, rr.HUBER, np.int32), np.full(ne, 1e150))
    assert hub.robust_info()["n_robust"] == ne and hub.robust_info()["n_downweighted"] == 0
    s2, r2 = _lin_and_lm(hub)
    hub.close()
    d = se3.differences(s2, s0)
    print(case, "Huber 1e150 against plain", d, {k: v for k, v in r2.items() if k != "poses"})
    assert d["diag"] <= 10 * rr.W_SPREAD_H and d["off"] <= 10 * rr.W_SPREAD_H and d["b"] <= 10 * rr.W_SPREAD_B
    assert d["chi2"] <= 10 * rr.W_SPREAD_CHI2
    assert (r2["its"], r2["trials"]) == (r0["its"], r0["trials"])


# ---- 5. outliers, end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(rr.SCENARIO_KERNELS))
@pytest.mark.parametrize("name", list(rr.SCENARIOS))
def test_outlier_scenarios_match_the_reference(pkg, name, kernel):
    """Two laps of a 15 m loop with 4 of 40 (3 of 20) loop measurements displaced by 2 - 6 m, DCS phi = 1 / Cauchy delta = 0.1
    on the loop edges: optimize(100) against optimize_robust.  The loops below weight 0.05 are exactly the corrupted ones, all
    others are above 0.9; the final sum rho0 and the keyframe positions are the reference's within ten times the reference's
    own spread on this run (edges permuted; damped solves stopped at the PCG's residual -- SCENARIO_SPREAD; for sum rho0 at
    least the linearisation's 10 x 3.5e-16).  The LM accept / reject sequences of those CPU runs differ from each other (the
    runs end on a flat sum rho0), so FINAL VALUES ONLY are compared, not iteration or trial counts."""
    r = rr.scenario_reference(name, kernel)
    gc, bad, loops = r["gc"], r["bad"], r["loops"]
    pg = _graph_on_gpu(pkg, gc, r["kinds"], r["deltas"])
    its = pg.optimize(rr.SCENARIO_ITERS)
    st = pg.last_stats
    got = pg.poses()
    w = pg.edge_robust()["weight"]
    info = pg.robust_info()
    pg.close()
    low = np.sort(loops[w[loops] < 0.05])
    good = np.setdiff1d(loops, bad)
    spread_pos, spread_chi = rr.SCENARIO_SPREAD[(name, kernel)]
    ref_chi = r["hist"][-1]["chi2"]
    dpos = float(np.abs(got[:, :3] - r["poses"][:, :3]).max())
    dchi = abs(st.chi2_final - ref_chi) / ref_chi
    tol_chi = 10 * max(spread_chi, rr.W_SPREAD_CHI2)
    print(name, kernel, "gpu iterations", its, "trials", st.lm_trials, "reference iterations", len(r["hist"]), "trials",
          sum(h["trials"] for h in r["hist"]), "| bad weights", w[bad], "least good weight", w[good].min(),
          "| position difference %.3e (bound %.3e) sum rho0 %.17g / %.17g relative %.3e (bound %.3e)" % (dpos, 10 * spread_pos, st.chi2_final, ref_chi, dchi, tol_chi),
          "| error against ground truth %.3f (reference %.3f)" % (rr.position_error(got, r["g"]), r["robust_err"]), info)
    assert np.array_equal(low, bad)
    assert (w[good] > 0.9).all() and np.array_equal(w[:gc["n_odo"]], np.ones(gc["n_odo"]))
    assert info["n_robust"] == len(loops) and info["n_downweighted"] >= len(bad)
    assert dchi <= tol_chi
    assert dpos <= 10 * spread_pos
    assert rr.position_error(got, r["g"]) < 2 * rr.SCENARIO_CLEAN_ERR[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rr.SCENARIOS))
def test_plain_solver_is_bent_by_the_same_outliers(pkg, name):
    """The proof that the kernel did the work: the plain GPU run on the same corrupted graph ends further than five times the
    clean graph's error from ground truth (reference figures: 7.35 m and 15.0 m against 0.735 m and 0.349 m)."""
    g, gc, bad, loops = rr.outlier_scenario(name)
    pg = _graph_on_gpu(pkg, gc)
    pg.optimize(rr.SCENARIO_ITERS)
    err = rr.position_error(pg.poses(), g)
    w = pg.edge_robust()["weight"]
    pg.close()
    print(name, "plain GPU run: max position error %.3f m, clean %.3f m" % (err, rr.SCENARIO_CLEAN_ERR[name]))
    assert err > 5 * rr.SCENARIO_CLEAN_ERR[name]
    assert np.array_equal(w, np.ones(len(w)))


# ---- 6. invalid input ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_kernels_are_refused_and_change_nothing(pkg):
    """delta = 0, delta = NaN, delta = inf, delta < 0, kind = 9, kind = -1, and arrays for one argument with NULL for the other:
    LSLAM_ERR_INVALID with a text, and the solver goes on with the kernels it had, bit for bit."""
    from importlib import import_module
    capi = import_module("the-cooper-mapper_amd.capi")
    g = se3.graph(LIN[2])
    kinds, deltas = rr.kernel_mix(g)
    pg = _graph_on_gpu(pkg, g, kinds, deltas)
    before = pg.linearize()
    lib = pg.lib
    ip, dp = capi.c_int32_p, capi.c_double_p

    def call(k, d):
        k = None if k is None else np.ascontiguousarray(k, np.int32)
        d = None if d is None else np.ascontiguousarray(d, np.float64)
        rc = lib.lslam_pg_set_robust_kernels(pg.h, None if k is None else k.ctypes.data_as(ip), None if d is None else d.ctypes.data_as(dp))
        return rc, lib.lslam_pg_last_error().decode()

    robust_edge = int(np.nonzero(kinds != rr.NONE)[0][3])
    for what, value in (("delta", 0.0), ("delta", float("nan")), ("delta", float("inf")), ("delta", -1.0), ("kind", 9), ("kind", -1)):
        k, d = kinds.copy(), deltas.copy()
        if what == "delta":
            d[robust_edge] = value
        else:
            k[robust_edge] = value
        rc, msg = call(k, d)
        print(what, value, rc, msg)
        assert rc == -1 and "robust kernels" in msg, (what, value, rc, msg)
        after = pg.linearize()
        assert all(_same_bits(after[x], before[x]) for x in ("diag", "off", "b")) and after["chi2"] == before["chi2"]
    for k, d in ((kinds, None), (None, deltas)):
        rc, msg = call(k, d)
        assert rc == -1 and "robust kernels" in msg
    after = pg.linearize()
    assert all(_same_bits(after[x], before[x]) for x in ("diag", "off", "b")) and after["chi2"] == before["chi2"]
    # a delta that is not valid is ignored where the kind is NONE
    d = deltas.copy()
    d[kinds == rr.NONE] = float("nan")
    rc, msg = call(kinds, d)
    assert rc == 0, msg
    after = pg.linearize()
    assert all(_same_bits(after[x], before[x]) for x in ("diag", "off", "b")) and after["chi2"] == before["chi2"]
    # the Python mirror raises and keeps its kernels; they survive a topology change (_drop / _build)
    with pytest.raises(capi.LslamError):
        pg.set_robust_kernels(kinds, 0.0)
    with pytest.raises(ValueError):
        pg.set_robust_kernels(["Tukey"] * len(kinds), 1.0)
    assert pg.optimize(3) == 3
    pg.close()
    inc = pkg.PoseGraph(0)
    for p in g["init"]:
        inc.add_se3_node(p)
    inc.fixed = g["fixed"]
    names = {rr.NONE: None, rr.HUBER: "Huber", rr.CAUCHY: "Cauchy", rr.DCS: "DCS"}
    for e in range(len(kinds) - 1):
        assert inc.add_se3_edge(g["ij"][e, 0], g["ij"][e, 1], g["meas"][e], g["info"][e], robust_kernel=names[int(kinds[e])],
                                robust_delta=deltas[e]) == e
    inc.build()
    e = len(kinds) - 1
    inc.add_se3_edge(g["ij"][e, 0], g["ij"][e, 1], g["meas"][e], g["info"][e], robust_kernel=int(kinds[e]), robust_delta=deltas[e])
    rebuilt = inc.linearize()
    inc.close()
    assert all(_same_bits(rebuilt[x], before[x]) for x in ("diag", "off", "b")) and rebuilt["chi2"] == before["chi2"]


# ---- 7. mirrors --------------------------------------------------------------------------------------------------------------------------
class _StubDetector:
    """hands the prepared loops to Graph.optimize once, as LoopDetector.detect_nearest would"""

    def __init__(self, loops):
        self.loops = loops

    def detect_nearest(self, keyframes, new_keyframes):
        out, self.loops = self.loops, []
        return out


def _drive_graph_mirror(pkg, kernel, delta):
    from importlib import import_module
    graph_mod = import_module("the-cooper-mapper_amd.graph")
    lc = import_module("the-cooper-mapper_amd.loop_closure")
    pgm = import_module("the-cooper-mapper_amd.pose_graph")
    g, gc, bad, loops = rr.outlier_scenario("kf60")
    n = len(gc["init"])
    stub = _StubDetector([])
    G = graph_mod.Graph(loop_detector=stub, max_keyframes_per_update=n, loop_robust_kernel=kernel, loop_robust_delta=delta)
    none = np.zeros((0, 4), np.float32)
    kfs = [G.add_frame(pgm.pose7_to_mat(p), none, none) for p in gc["init"]]
    assert all(k is not None for k in kfs)
    prepared = [lc.Loop(kfs[int(a)], kfs[int(b)], pgm.pose7_to_mat(gc["meas"][e])) for e, (a, b) in zip(loops, gc["ij"][loops])]
    stub.loops = prepared
    found, iterations = G.optimize(1000)
    assert len(found) == len(loops) and G.loops == prepared
    return G, kfs, prepared, bad - loops[0], iterations


@pytest.mark.gpu
def test_graph_mirror_reports_exactly_the_corrupted_loops_and_cpp_agrees(pkg, tmp_path):
    """Graph(loop_robust_kernel="DCS") driven with the 60-keyframe scenario: dead-reckoned odometry as the frames, the
    prepared loops (corrupted ones included) through a stub detector.  rejected_loops() is exactly the corrupted loops;
    odometry edges carry no kernel.  The C++ program drives pose_graph::SolverG2OT (add_robust_kernel, edgeWeights) with the
    same 4x4 matrices: loop weights and positions equal the Python mirror's to 1e-9 (m) -- both hand the library the same bits.
    It then drives pose_graph::Graph with the same frames, the loops handed over through Graph::loop_source, and
    loop_robust_kernel = "DCS": loopWeights() is aligned with Graph::loops, the loops below 0.1 are exactly the corrupted ones.
    That Graph computes its odometry edges itself (inverse(prev.odom) * odom, its own rigid inverse against numpy's LAPACK
    one): its inputs equal the Python mirror's to rounding only, so positions are compared at ten times the reference's own
    spread on this scenario under rounding-level changes (SCENARIO_SPREAD kf60 / DCS: 2.5e-5 m) and the weights at 1e-6
    (a misaligned weight is off by 1).  Without a kernel the same mirror rejects nothing."""
    from importlib import import_module
    from test_abi import _build_cpp
    pgm = import_module("the-cooper-mapper_amd.pose_graph")
    G, kfs, prepared, bad_loops, iterations = _drive_graph_mirror(pkg, "DCS", 1.0)
    w = G.loop_weights()
    rejected = G.rejected_loops()
    print("loop weights", w, "rejected", [prepared.index(lp) for lp in rejected], "corrupted", bad_loops, "iterations", iterations)
    assert sorted(prepared.index(lp) for lp in rejected) == sorted(bad_loops.tolist())
    assert (np.delete(w, bad_loops) > 0.9).all() and len(G.loops) == len(w)
    allw = G.solver.edge_robust()["weight"]
    assert np.array_equal(allw[:len(kfs) - 1], np.ones(len(kfs) - 1)) and G.solver.robust_info()["n_robust"] == len(prepared)
    pos = np.stack([k.estimate[:3, 3] for k in kfs])
    # the same matrices for the C++ mirror
    lines = ["%d %d" % (len(kfs), len(G.solver._ij))]
    fmt = lambda M: " ".join("%.17g" % v for v in np.asarray(M, np.float64).ravel())  # noqa: E731
    for k in kfs:
        lines.append(fmt(k.odom))  # tf_odom2graph was the identity when the queue was flushed
    for e in range(len(kfs) - 1):
        lines.append("%d %d 0 0.8 0.4 0.8 1 2 1 %s" % (e, e + 1, fmt(np.linalg.inv(kfs[e].odom) @ kfs[e + 1].odom)))
    for lp in prepared:
        lines.append("%d %d 1 2 2 2 2 2 2 %s" % (lp.key1.node, lp.key2.node, fmt(lp.relative_pose.astype(np.float64))))
    (tmp_path / "graph.txt").write_text("\n".join(lines) + "\n")
    exe = _build_cpp(pkg, tmp_path, "robust_posegraph_end_to_end")
    out = subprocess.run([str(exe), str(tmp_path / "graph.txt"), "DCS", "1"], capture_output=True, text=True, timeout=120)
    print(out.stdout[:300], "...", out.stderr[-1500:])
    assert out.returncode == 0
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.split()]  # (the solver shim prints g2o's banner lines as well)
    cw = np.array([float(r[2]) for r in rows if r[0] == "WEIGHT"])
    cpos = np.array([[float(v) for v in r[2:5]] for r in rows if r[0] == "POS"])
    print("C++ against Python: weights %.3e positions %.3e" % (np.abs(cw - w).max(), np.abs(cpos - pos).max()))
    assert ["REFUSED", "1"] in rows and ["ITER", str(iterations)] in rows
    assert [int(r[1]) for r in rows if r[0] == "WEIGHT"] == G.loop_edges
    assert cw.shape == w.shape and np.abs(cw - w).max() <= 1e-9
    assert cpos.shape == pos.shape and np.abs(cpos - pos).max() <= 1e-9
    gw = np.array([float(r[2]) for r in rows if r[0] == "GWEIGHT"])
    gpos = np.array([[float(v) for v in r[2:5]] for r in rows if r[0] == "GPOS"])
    print("C++ Graph against Python Graph: weights %.3e positions %.3e" % (np.abs(gw - w).max(), np.abs(gpos - pos).max()),
          [r for r in rows if r[0] in ("GITER", "GLOOPS")])
    assert ["GLOOPS", str(len(prepared))] in rows and gw.shape == w.shape and gpos.shape == pos.shape
    assert sorted(np.nonzero(gw < 0.1)[0].tolist()) == sorted(bad_loops.tolist())
    assert np.abs(gw - w).max() <= 1e-6
    assert np.abs(gpos - pos).max() <= 10 * rr.SCENARIO_SPREAD[("kf60", "dcs")][0]
    G.solver.close()
    # the default: no kernel, nothing reported, and the map bends
    G0, kfs0, prepared0, _, _ = _drive_graph_mirror(pkg, None, 1.0)
    assert G0.loop_robust_kernel is None and G0.rejected_loops() == [] and np.array_equal(G0.loop_weights(), np.ones(len(prepared0)))
    pos0 = np.stack([k.estimate[:3, 3] for k in kfs0])
    g = rr.outlier_scenario("kf60")[0]
    e_k = float(np.linalg.norm(pos - g["gt"][:, :3], axis=1).max())
    e_0 = float(np.linalg.norm(pos0 - g["gt"][:, :3], axis=1).max())
    print("error against ground truth: DCS %.3f m, no kernel %.3f m" % (e_k, e_0))
    assert e_k < 2 * rr.SCENARIO_CLEAN_ERR["kf60"] and e_0 > 5 * rr.SCENARIO_CLEAN_ERR["kf60"]
    G0.solver.close()
