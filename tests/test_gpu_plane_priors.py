"""csrc/lslam_posegraph.hip's plane priors (lslam_pg_set_plane_priors) against the CPU reference tests/floor_ref.py, on top of
the XYZ / POSE priors of tests/posegraph_prior_ref.py's small graphs.  Parity stays unpinned (neither hdl_graph_slam nor g2o is
available); the semantics are the header's, as the reference restates them.

Every tolerance is ten times a floor of the references themselves, measured on the CPU (tests/test_floor_ref.py and the earlier
CPU suites) and recorded in floor_ref.py, posegraph_se3.py and robust_posegraph_ref.py; none was calibrated against what the
kernels return.  Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import floor_ref as F
import posegraph_prior_ref as ppr
import posegraph_se3 as se3
import robust_posegraph_ref as rr

pytestmark = pytest.mark.gpu
po = se3.po
INVALID = -1  # LSLAM_ERR_INVALID


def _graph(pkg, g, pr=None, pl=None, fixed=None):
    pg = pkg.PoseGraph(0)
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"], fixed=g["fixed"] if fixed is None else fixed, priors=pr, plane_priors=pl)
    return pg


def _in_pair_order(s):
    o = np.lexsort((s["off_ij"][:, 1], s["off_ij"][:, 0]))
    return dict(diag=s["diag"], off=s["off"][o], off_ij=s["off_ij"][o].astype(np.int32).reshape(-1, 2), b=s["b"], chi2=s["chi2"])


def _bits(s):
    return tuple(np.ascontiguousarray(s[k]).view(np.int64).tobytes() for k in ("diag", "off", "b")) + (np.float64(s["chi2"]).tobytes(),)


def _planes_for(g, seed, n_max=40):
    """up to n_max plane priors on random vertices of g (vertices repeat: several on one vertex, far apart in plane-prior order)"""
    n = len(g["init"])
    return F.make_planes(g, np.random.default_rng(seed).integers(0, n, min(2 * n, n_max)), seed)


def _assert_system(got, g, pr, pl, fixed):
    """against both references, as tests/test_gpu_posegraph_priors.py: 10 x SPREAD_* (C oracle) and 10 x O2O_* (numpy oracle)"""
    sc, sn = F.plane_system(g, pr, pl, oracle="c", fixed=fixed), F.plane_system(g, pr, pl, oracle="np", fixed=fixed)
    dc, dn = ppr.differences(got, sc), ppr.differences(got, sn)
    print("against C", dc, "against numpy", dn)
    assert dc["diag"] <= 10 * se3.SPREAD_H and dc["off"] <= 10 * se3.SPREAD_H, dc
    assert dc["b"] <= 10 * se3.SPREAD_B and dc["chi2"] <= 10 * se3.SPREAD_CHI2, dc
    assert dn["h"] <= 10 * se3.O2O_H and dn["b"] <= 10 * se3.O2O_B and dn["chi2"] <= 10 * se3.O2O_CHI2, dn
    return sc


@pytest.mark.parametrize("name", ppr.LIN_PRIOR_CASES)
def test_plane_prior_linearize_matches_both_references(pkg, name):
    """diag, off, b and chi2 of posegraph_prior_ref's small graphs with plane priors on top of their XYZ / POSE priors (1 to 400
    vertices, fixed and free gauges, several plane priors on one vertex, some on the fixed vertex)."""
    g, pr, fixed = ppr.lin_case(name)
    pl = _planes_for(g, 1)
    pg = _graph(pkg, g, pr, pl, fixed)
    assert pg.num_priors == len(pr["vertex"]) and pg.num_plane_priors == len(pl["vertex"])  # the two sets keep their counts
    got = _in_pair_order(pg.linearize())
    e2 = pg.prior_robust()["e2"]  # keeps its meaning: the XYZ / POSE priors only
    pg.close()
    assert len(e2) == len(pr["vertex"])
    _assert_system(got, g, pr, pl, fixed)
    if fixed >= 0:
        assert np.array_equal(got["diag"][fixed], np.eye(6)) and not got["b"][6 * fixed:6 * fixed + 6].any()


@pytest.mark.parametrize("name", ["n2_free_mixed", "n7_pose_fixed", "n65_mixed"])
def test_plane_priors_permuted_stay_inside_the_summation_spread(pkg, name):
    """The device sums a vertex's plane priors in the order they were set: another order is another rounding, nothing more.  The
    systems of eight permutations against the first order: inside 10 x posegraph_se3.SPREAD_*; the SAME order set twice: the same
    bits."""
    g, pr, fixed = ppr.lin_case(name)
    pl = _planes_for(g, 2)
    pg = _graph(pkg, g, pr, pl, fixed)
    first = _in_pair_order(pg.linearize())
    pg.set_plane_priors(pl)
    assert _bits(_in_pair_order(pg.linearize())) == _bits(first)
    worst = dict(diag=0.0, off=0.0, b=0.0, chi2=0.0)
    for r in range(8):
        pg.set_plane_priors(F.planes_permuted(pl, np.random.default_rng(r).permutation(len(pl["vertex"]))))
        d = ppr.differences(_in_pair_order(pg.linearize()), first)
        worst = {k: max(worst[k], d[k]) for k in worst}
    pg.close()
    print(name, "spread over 8 permutations", worst)
    assert worst["diag"] <= 10 * se3.SPREAD_H and worst["off"] == 0.0 and worst["b"] <= 10 * se3.SPREAD_B
    assert worst["chi2"] <= 10 * se3.SPREAD_CHI2


def _kernel_mix(g, pl):
    """plane prior p gets kind p % 4; delta from the reference's e2, so that every kernel's threshold sits among the errors it meets"""
    e2 = F.plane_rho(g["init"], pl)[0]
    kinds = np.arange(len(e2), dtype=np.int32) % 4
    med = float(np.median(e2[e2 > 0]))
    return dict(pl, kernels=kinds, deltas=np.where(kinds == rr.DCS, med, np.sqrt(med)))


@pytest.mark.parametrize("name", ["n65_free_pose", "n65_mixed"])
def test_plane_prior_robust_values_and_weighted_system(pkg, name):
    """lslam_pg_plane_prior_robust (e2, rho0, rho1) against robust_posegraph_ref.rho on the reference's e2 for every kernel, plane
    priors on both sides of each threshold (asserted on the reference alone), at the current estimate and at caller-supplied
    poses, and the weighted system.  Per prior 10 x W_EDGE_*."""
    g, pr, fixed = ppr.lin_case(name)
    q = _kernel_mix(g, _planes_for(g, 3))
    e2, r0, r1 = F.plane_rho(g["init"], q)
    sides = rr.sides(q["kernels"], q["deltas"], e2)
    assert all(a > 0 and b > 0 for a, b in sides.values()), sides
    pg = _graph(pkg, g, pr, q, fixed)
    tap, at = pg.plane_prior_robust(), pg.plane_prior_robust(g["gt"])
    got = _in_pair_order(pg.linearize())
    pg.close()
    # per prior: 10 x the recorded floor plus the error's own conditioning (floor_ref.plane_e2_rounding: derived, not measured;
    # rho0 and rho1 move by at most twice the relative change of e2 under every kernel)
    c0, cg = F.plane_e2_rounding(g["init"], q), F.plane_e2_rounding(g["gt"], q)
    de, dr, dw = np.abs(tap["e2"] - e2) / e2, np.abs(tap["rho"] - r0) / r0, np.abs(tap["weight"] - r1) / r1
    e2g, _, r1g = F.plane_rho(g["gt"], q)
    de_g, dw_g = np.abs(at["e2"] - e2g) / e2g, np.abs(at["weight"] - r1g) / r1g
    print(name, "sides", sides, "e2 %.3e rho0 %.3e weight %.3e (conditioning up to %.3e); at gt e2 %.3e weight %.3e (conditioning up to %.3e)" % (
        de.max(), dr.max(), dw.max(), c0.max(), de_g.max(), dw_g.max(), cg.max()))
    assert (de <= 10 * rr.W_EDGE_E2 + c0).all() and (dr <= 10 * rr.W_EDGE_RHO + 2 * c0).all() and (dw <= 10 * rr.W_EDGE_WEIGHT + 2 * c0).all()
    assert (de_g <= 10 * rr.W_EDGE_E2 + cg).all() and (dw_g <= 10 * rr.W_EDGE_WEIGHT + 2 * cg).all()
    assert (tap["weight"][q["kernels"] == rr.NONE] == 1.0).all() and (tap["weight"] < 1.0).any()
    _assert_system(got, g, pr, q, fixed)


def test_plane_prior_on_the_fixed_vertex_adds_only_to_chi2(pkg):
    g, pr, fixed = ppr.lin_case("n7_pose_fixed")
    pl = F.make_planes(g, [0, fixed, 5, fixed], 4)
    on_fixed = pl["vertex"] == fixed
    with_all = _graph(pkg, g, pr, pl, fixed)
    without = _graph(pkg, g, pr, F.planes_permuted(pl, np.nonzero(~on_fixed)[0]), fixed)
    a, b = with_all.linearize(), without.linearize()
    with_all.close()
    without.close()
    e2 = F.plane_rho(g["init"], pl)[0][on_fixed].sum()
    print("chi2 with %.17g without %.17g reference e2 of the plane priors on the fixed vertex %.17g" % (a["chi2"], b["chi2"], e2))
    assert np.array_equal(a["diag"], b["diag"]) and np.array_equal(a["b"], b["b"]) and np.array_equal(a["off"], b["off"])
    assert e2 > 0 and abs((a["chi2"] - b["chi2"]) - e2) <= 10 * se3.SPREAD_CHI2 * a["chi2"]


def test_free_gauge_is_well_posed_once_an_orientation_prior_holds_yaw(pkg):
    """fixed = -1, one XYZ prior and plane priors against the world floor on three keyframes that are not collinear: height, roll
    and pitch are held by the planes, the position by the fix -- yaw about the fix is not, until one orientation prior (POSE,
    zero translation block) holds it.  Asserted on the reference first (the system without it is singular), then the solve: the
    damped step against the reference's within 10 x the PCG's tolerance x the condition number, and an optimisation that ends
    at the reference LM's poses."""
    g = se3.graph((7, 6, 2, 3, False))
    g["fixed"] = -1
    gt = g["gt"]
    planes_on = [0, 3, 6]
    d = gt[planes_on, :3] - gt[planes_on[0], :3]
    assert np.linalg.norm(np.cross(d[1], d[2])) > 1e-2, "the three keyframes must not be collinear"
    pl = F.make_planes(g, planes_on, 5, sigma=(0.01, 0.02), world=(0.0, 0.0, 1.0, 0.0))
    pl["info"][:] = np.diag([1e4, 1e4, 2.5e3])
    xyz = ppr.make_priors(g, [0], [ppr.XYZ], 8, sigma=(0.05, 0.0))
    yaw = ppr.make_priors(g, [2], [ppr.POSE], 9, sigma=(0.0, 0.01), rank_deficient=(0,))
    both = {k: np.concatenate([xyz[k], yaw[k]]) for k in xyz}
    lam = 1e-9
    conds = {}
    for label, pr in (("without", xyz), ("with", both)):
        s = F.plane_system(g, pr, pl, oracle="np", fixed=-1)
        conds[label] = np.linalg.cond(ppr.to_sparse(s).toarray())
    print("condition number without the orientation prior %.3e, with it %.3e" % (conds["without"], conds["with"]))
    assert conds["without"] > 1e13 and conds["with"] < 1e9
    s = F.plane_system(g, both, pl, oracle="np", fixed=-1)
    want = ppr.solve_damped(ppr.to_sparse(s), s["b"], lam, -1)
    pg = _graph(pkg, g, both, pl, -1)
    pg.linearize()
    dx, _ = pg.solve(lam)
    err = np.abs(dx - want).max() / np.abs(want).max()
    print("damped step: relative error %.3e, bound %.3e" % (err, 10 * 1e-10 * conds["with"]))
    assert np.isfinite(dx).all() and err <= 10 * 1e-10 * conds["with"]
    its = pg.optimize(30)
    st, got = pg.last_stats, pg.poses()
    pg.close()
    # the reference LM over the same 30 iterations; its own spread between two stopping tolerances is the bound's floor
    full, hist = F.plane_optimize(g, both, pl, -1, 30)
    loose, _ = F.plane_optimize(g, both, pl, -1, 30, rel_tol=1e-9)
    tight, _ = F.plane_optimize(g, both, pl, -1, 30, rel_tol=1e-12)
    spread = float(np.abs(loose - tight).max())
    path = float(np.abs(full - g["init"]).max())
    tol = max(10 * spread, 1e-8 * path)
    err = float(np.abs(got - full).max())
    print("LM: %d iterations, chi2 %.6g -> %.6g (reference %.6g), pose error %.3e bound %.3e" % (its, st.chi2_initial, st.chi2_final, hist[-1]["chi2"], err, tol))
    assert its >= 1 and st.chi2_final < st.chi2_initial and np.isfinite(got).all()
    assert err <= tol


def test_clearing_the_set_restores_the_bits_of_the_graph_without_plane_priors(pkg):
    for name in ("n7_xyz", "n65_free_pose"):
        g, pr, fixed = ppr.lin_case(name)
        pg = _graph(pkg, g, pr, None, fixed)
        before = _bits(_in_pair_order(pg.linearize()))
        pg.set_plane_priors(_planes_for(g, 6))
        assert pg.num_plane_priors > 0 and _bits(_in_pair_order(pg.linearize())) != before
        pg.set_plane_priors(None)
        assert pg.num_plane_priors == 0 and _bits(_in_pair_order(pg.linearize())) == before
        assert pg.num_priors == len(pr["vertex"])
        # ... and a graph with plane priors but no other priors, then none at all
        pg.set_priors(None)
        plain = _bits(_in_pair_order(pg.linearize()))
        pg.set_plane_priors(_planes_for(g, 6))
        got = _in_pair_order(pg.linearize())
        _assert_system(got, g, None, _planes_for(g, 6), fixed)
        pg.set_plane_priors(None)
        assert _bits(_in_pair_order(pg.linearize())) == plain
        pg.close()


def test_every_rejected_input_changes_nothing(pkg):
    g, pr, fixed = ppr.lin_case("n7_xyz")
    pl = _planes_for(g, 7)
    pg = _graph(pkg, g, pr, pl, fixed)
    before = _bits(_in_pair_order(pg.linearize()))
    n = len(pl["vertex"])

    def bad(**kw):
        q = {k: np.array(v, copy=True) for k, v in pl.items()}
        for k, (i, val) in kw.items():
            q[k][i] = val
        return q
    flipped = bad()
    flipped["meas"][3] = -flipped["meas"][3]  # the same plane, its normal turned over: opposite hemispheres
    asym = np.array(pl["info"][1], copy=True)
    asym[0, 1] += 1e-3
    cases = [("vertex out of range", bad(vertex=(0, len(g["init"])))), ("vertex out of range", bad(vertex=(2, -1))),
             ("world plane is not finite", bad(world=((1, 0), np.nan))), ("measured plane is not finite", bad(meas=((2, 3), np.inf))),
             ("world plane has a zero normal", bad(world=(4, (0.0, 0.0, 0.0, 1.0)))),
             ("measured plane has a zero normal", bad(meas=(4, (0.0, 0.0, 0.0, 1.0)))),
             ("information is not finite", bad(info=((0, 1, 1), np.nan))), ("negative diagonal", bad(info=((0, 2, 2), -1.0))),
             ("not symmetric", bad(info=(1, asym))), ("opposite hemispheres", flipped),
             ("unknown robust kernel", dict(pl, kernels=np.full(n, 9, np.int32))),
             ("delta must be finite", dict(pl, kernels=np.full(n, rr.HUBER, np.int32), deltas=np.zeros(n)))]
    for what, q in cases:
        with pytest.raises(pkg.LslamError) as e:
            pg.set_plane_priors(q)
        assert e.value.code == INVALID and what in str(e.value), (what, str(e.value))
        assert pg.num_plane_priors == n and pg.num_priors == len(pr["vertex"])
    lib = pg.lib
    v = np.zeros(1, np.int32)
    four, nine, one = np.array([0.0, 0, 1, 0]), np.eye(3).reshape(9), np.ones(1)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.lslam_pg_set_plane_priors(pg.h, 1, ip(v), dp(four), dp(four), dp(nine), ip(v), None) == INVALID  # kind without delta
    assert lib.lslam_pg_set_plane_priors(pg.h, 1, ip(v), dp(four), dp(four), dp(nine), None, dp(one)) == INVALID
    assert lib.lslam_pg_set_plane_priors(pg.h, 1, ip(v), None, dp(four), dp(nine), None, None) == INVALID
    assert lib.lslam_pg_set_plane_priors(pg.h, -1, None, None, None, None, None, None) == INVALID
    assert lib.lslam_pg_set_plane_priors(None, 0, None, None, None, None, None, None) == INVALID
    assert pg.num_plane_priors == n
    assert _bits(_in_pair_order(pg.linearize())) == before
    pg.close()


def test_save_and_load_keep_the_plane_priors_and_the_other_readers_skip_them(pkg, tmp_path):
    """lslam_pg_save_g2o writes the plane priors behind the other priors under this project's own tag; lslam_g2o_read and
    lslam_g2o_read_priors return exactly what they return for the same graph saved without plane priors; the plane-prior reader
    returns what was set; a graph loaded back linearises to the same bits."""
    g, pr, fixed = ppr.lin_case("n7_pose_fixed")
    pl = _planes_for(g, 8)
    with_planes, without = _graph(pkg, g, pr, pl, fixed), _graph(pkg, g, pr, None, fixed)
    a, b = tmp_path / "with.g2o", tmp_path / "without.g2o"
    with_planes.save(a)
    without.save(b)
    lines = open(a).read().splitlines()
    tagged = [k for k, l in enumerate(lines) if l.startswith("EDGE_SE3_PRIOR_PLANE ")]
    assert len(tagged) == len(pl["vertex"]) and tagged == list(range(len(lines) - len(tagged), len(lines)))  # behind everything else
    assert [l for l in lines if not l.startswith("EDGE_SE3_PRIOR_PLANE ")] == open(b).read().splitlines()
    ra, rb = pkg.PoseGraph.read_g2o(a), pkg.PoseGraph.read_g2o(b)
    for k in ("poses", "ij", "meas", "info"):
        assert np.array_equal(ra[k], rb[k]), k
    assert ra["fixed"] == rb["fixed"] == fixed
    for k in ("vertex", "type", "meas", "info"):
        assert np.array_equal(ra["priors"][k], rb["priors"][k]), k
    assert len(rb["plane_priors"]["vertex"]) == 0
    q = ra["plane_priors"]
    assert np.array_equal(q["vertex"], pl["vertex"]) and np.array_equal(q["world"], pl["world"]) and np.array_equal(q["meas"], pl["meas"])
    assert np.array_equal(q["info"], pl["info"])  # 17 significant digits: the doubles come back exactly
    want = _bits(_in_pair_order(with_planes.linearize()))
    back = pkg.PoseGraph(0)
    back.load(a)
    assert back.num_plane_priors == len(pl["vertex"]) and back.num_priors == len(pr["vertex"])
    assert _bits(_in_pair_order(back.linearize())) == want
    for p in (with_planes, without, back):
        p.close()


def test_two_edge_shards_count_every_plane_prior_once(pkg):
    """posegraph_se3's 65-vertex shard case with XYZ / POSE priors and plane priors, shards (0, cut) and (cut, ne), no all-reduce
    (each shard's raw contribution): the host sum equals the full system within the sharded bounds (10 x SPREAD_*), and the second
    shard -- which carries no prior of either set -- gives the same shard of a graph without any BIT FOR BIT."""
    g = se3.graph((65, 100, 5, 32, True))
    _, pr, _ = ppr.lin_case("n65_mixed")  # the same graph
    pl = _planes_for(g, 9)
    ne = len(g["ij"])
    cut = ne // 2

    def system(priors, planes, shard=None):
        pg = _graph(pkg, g, priors, planes)
        if shard is not None:
            pg.set_shard(*shard)
        s = pg.linearize()
        pg.close()
        return s
    full = system(pr, pl)
    lo, hi, hi_plain = system(pr, pl, (0, cut)), system(pr, pl, (cut, ne)), system(None, None, (cut, ne))
    d = lo["diag"] + hi["diag"]
    d[g["fixed"]] = np.eye(6)
    summed = dict(diag=d, off=lo["off"] + hi["off"], off_ij=full["off_ij"], b=lo["b"] + hi["b"], chi2=lo["chi2"] + hi["chi2"])
    diff = ppr.differences(summed, full)
    print("sharded against full", diff)
    assert diff["diag"] <= 10 * se3.SPREAD_H and diff["off"] <= 10 * se3.SPREAD_H
    assert diff["b"] <= 10 * se3.SPREAD_B and diff["chi2"] <= 10 * se3.SPREAD_CHI2
    assert _bits(hi) == _bits(hi_plain)
    assert lo["chi2"] > system(pr, None, (0, cut))["chi2"]  # ... and the first shard does carry the plane priors
