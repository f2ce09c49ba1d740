"""csrc/lslam_pg_marginals.hip -- lslam_pg_marginals and lslam_pg_relative_covariances -- against the numpy fp64 reference of
tests/marginals_ref.py: the dense inverse of the system lslam_pg_linearize exports, finite-difference Jacobians for the relative
covariances.  The graphs are the smallest on which the path can go wrong: chains of 1, 2, 7, 22 and 43 vertices (22 crosses a
16-vertex workgroup of the panel kernels and the 21-vertex row block of the solver's own), and 130 vertices with 12 loop edges
(three aggregates: the only one on which the second level's dense product has more than one block row; query lists of 1, 9, 10,
11 and 40 vertices end a 10-vertex panel ragged, full, and spill into a second and a fifth panel).  Every case runs with the
block-Jacobi preconditioner alone (coarse = 0) and with the second level (coarse = 1).

Bounds (marginals_ref.column_bound, derived there): a solved column differs from the reference's by at most
2 tol ||Sigma||_2 + 64 eps kappa(H) ||Sigma||_2; a 6x6 block is six columns, so its Frobenius error is at most sqrt(6) of that
(symmetrising does not increase it).  Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import marginals_ref as mr
import posegraph_se3 as se3

po = se3.po
TOL = 1e-8  # the solver's default relative residual
COARSE = (0, 1)
VPP = 10    # vertices per panel (MG_W / 6 in lslam_pg_marginals.hip)
BOX = 2.0   # side of the cube the positions are drawn from [m]
# The iteration cap is an input of the call, not a tolerance.  Its default, 6 n_v, is CG's bound in exact arithmetic; in fp64
# block-Jacobi PCG on these chains (uniformly random rotations, information matrices of condition ~100) takes several times
# that -- on the device: 214 iterations on the 22-chain (default cap 132), 544 on the 43-chain (258), 961 on the 130-vertex
# graph (780).  Only test_default_options runs on the default.
MAX_ITERS = 4000
_cache = {}


def _graph(pkg, key):
    """(PoseGraph, the graph dict, lslam_pg_linearize's system, dense H, reference Sigma) per named graph, built once."""
    if key in _cache:
        return _cache[key]
    kind, n, fixed = key
    kw = {}
    if kind == "chain":
        g = mr.make_chain(n, 100 + n, fixed=fixed, box=BOX)
    elif kind == "loops":
        g = mr.make_chain(n, 200 + n + max(fixed, 0), n_loops=12, fixed=max(fixed, 0), box=BOX)
    elif kind == "priors":
        # no fixed vertex: two pose priors and one XYZ prior hold the gauge; Cauchy kernels on the loop edges, two of which are
        # far outliers; one plane prior
        g = mr.make_chain(n, 300 + n, n_loops=12, fixed=0, box=BOX)
        g["fixed"] = -1
        rng = np.random.default_rng(5)
        ne = len(g["ij"])
        loops = np.arange(n - 1, ne)
        g["meas"][loops[0], :3] += 40.0
        g["meas"][loops[5], :3] -= 25.0
        kw["kernels"] = ["NONE"] * (n - 1) + ["Cauchy"] * 12
        kw["deltas"] = 1.5
        pv = np.array([3, n - 2, n // 2], np.int32)
        pm = g["gt"][pv].copy()
        pm[2, 3:] = [0, 0, 0, 1]
        pi = mr.random_spd(rng, 3)
        kw["priors"] = dict(vertex=pv, type=np.array([pkg.pose_graph.PRIOR_POSE, pkg.pose_graph.PRIOR_POSE, pkg.pose_graph.PRIOR_XYZ], np.int32),
                            meas=pm, info=pi)
        # the floor z = 0 as vertex n // 3 sees it from its estimate (n_s = R^T n, d_s = d + n . t), 5 cm off
        pe = g["init"][n // 3]
        ns = po.qrot(po.qconj(pe[3:]), np.array([0.0, 0.0, 1.0]))
        kw["plane_priors"] = dict(vertex=np.array([n // 3], np.int32), world=np.array([[0.0, 0.0, 1.0, 0.0]]),
                                  meas=np.array([[ns[0], ns[1], ns[2], pe[2] + 0.05]]), info=np.diag([30.0, 20.0, 50.0])[None])
    pg = pkg.PoseGraph(0)
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"], fixed=g["fixed"], **kw)
    lin = pg.linearize()
    H, S = mr.covariance(lin, g["fixed"])
    _cache[key] = (pg, g, lin, H, S)
    return _cache[key]


def _block_errors(cov, S, vs):
    return np.array([np.linalg.norm(cov[k] - mr.block(S, v, v)) for k, v in enumerate(vs)])


@pytest.fixture(scope="module", autouse=True)
def _close_graphs():
    yield
    for pg, *_ in _cache.values():
        pg.close()
    _cache.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
@pytest.mark.parametrize("n", (1, 2, 7, 22, 43))
def test_chain_marginals_match_the_dense_inverse(pkg, n, coarse):
    """Every vertex of a chain with random SE(3) poses and full SPD information, cross blocks included; the fixed vertex's
    blocks are exact zeros; the raw columns of the last vertex are inside the column bound and their TRUE residual through
    the dense H is at most 2 tol."""
    pg, g, lin, H, S = _graph(pkg, ("chain", n, 0))
    vs = np.arange(n)
    cov, cross = pg.marginals(vs, cross=True, coarse=coarse, max_iters=MAX_ITERS)
    st = pg.marginal_stats
    bound = mr.column_bound(H, S, TOL)
    err = _block_errors(cov, S, vs)
    full = np.block([[cross[a, b] for b in range(n)] for a in range(n)])
    xerr = max(np.linalg.norm(cross[a, b] - mr.block(S, a, b)) for a in range(n) for b in range(n))
    print("n %d coarse %d: block error %.2e, cross %.2e (bound sqrt(6) x %.2e), iterations max %d, kappa %.2e, ||Sigma|| %.2e"
          % (n, coarse, err.max(), xerr, bound, st.iters_max, np.linalg.cond(H), np.linalg.norm(S, 2)))
    assert st.coarse_used == coarse and st.columns == 6 * n and st.panels == (n - 1 + VPP - 1) // VPP
    assert st.worst_rel_residual <= TOL
    assert not cov[0].any() and not cross[0].any() and not cross[:, 0].any()
    assert err.max() <= np.sqrt(6) * bound and xerr <= np.sqrt(6) * bound
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1)))
    assert np.array_equal(full, full.T)
    assert all(np.array_equal(cross[a, a], cov[a]) for a in range(n))
    if n > 1:
        x = pg.debug_marginal_columns(n - 1, coarse=coarse, max_iters=MAX_ITERS)
        E = np.eye(6 * n)[:, 6 * (n - 1):]
        cerr = np.linalg.norm(x - S[:, 6 * (n - 1):], axis=0).max()
        res = np.linalg.norm(H @ x - E, axis=0).max()
        print("   raw columns of vertex %d: error %.2e (bound %.2e), true residual %.2e (2 tol %.1e)" % (n - 1, cerr, bound, res, 2 * TOL))
        assert cerr <= bound and res <= 2 * TOL


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
def test_loop_graph_lists_of_every_panel_shape_give_the_same_bits(pkg, coarse):
    """130 vertices, 12 loop edges: lists of 1, 9, 10, 11 and 40 vertices -- vertex 77 alone, last, first, in a second panel --
    and a second call: its block has identical bits everywhere; so have duplicates in one list; everything inside the bound."""
    pg, g, lin, H, S = _graph(pkg, ("loops", 130, 0))
    bound = np.sqrt(6) * mr.column_bound(H, S, TOL)
    rng = np.random.default_rng(11)
    others = [int(v) for v in rng.permutation(np.r_[1:77, 78:130])]
    lists = {1: [77], VPP - 1: others[:VPP - 2] + [77], VPP: [77] + others[:VPP - 1], VPP + 1: others[:VPP] + [77],
             40: others[:25] + [77] + others[25:39]}
    blocks, worst, iters = [], 0.0, 0
    for size, vs in lists.items():
        assert len(vs) == size
        cov = pg.marginals(vs, coarse=coarse, max_iters=MAX_ITERS)
        st = pg.marginal_stats
        assert st.columns == 6 * size and st.panels == (size + VPP - 1) // VPP and st.worst_rel_residual <= TOL
        worst = max(worst, _block_errors(cov, S, vs).max())
        iters = max(iters, st.iters_max)
        blocks.append(cov[vs.index(77)])
    again = pg.marginals(lists[40], coarse=coarse, max_iters=MAX_ITERS)
    blocks.append(again[lists[40].index(77)])
    dup = pg.marginals([5, 77, 5, 99, 77, 77], coarse=coarse, max_iters=MAX_ITERS)
    assert pg.marginal_stats.columns == 18
    print("coarse %d: worst block error %.2e (bound %.2e), iterations max %d" % (coarse, worst, bound, iters))
    assert worst <= bound
    assert all(np.array_equal(b, blocks[0]) for b in blocks[1:])
    assert np.array_equal(dup[1], blocks[0]) and np.array_equal(dup[4], dup[1]) and np.array_equal(dup[5], dup[1])
    assert np.array_equal(dup[0], dup[2])
    # the cross blocks of a list with a duplicate and the fixed vertex: exact transposes, zeros at the fixed vertex
    vs = [12, 0, 101, 12]
    cov, cross = pg.marginals(vs, cross=True, coarse=coarse, max_iters=MAX_ITERS)
    for a in range(4):
        for b in range(4):
            assert np.array_equal(cross[a, b], cross[b, a].T)
            assert np.linalg.norm(cross[a, b] - mr.block(S, vs[a], vs[b])) <= bound
    assert not cross[1].any() and not cross[:, 1].any() and np.array_equal(cross[0, 3], cov[0])


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
def test_fixed_vertex_in_the_middle(pkg, coarse):
    pg, g, lin, H, S = _graph(pkg, ("loops", 130, 60))
    vs = [59, 60, 61, 0, 129]
    cov = pg.marginals(vs, coarse=coarse, max_iters=MAX_ITERS)
    err = _block_errors(cov, S, vs)
    bound = np.sqrt(6) * mr.column_bound(H, S, TOL)
    print("coarse %d: block error %.2e (bound %.2e)" % (coarse, err.max(), bound))
    assert not cov[1].any() and cov[0].any()
    assert err.max() <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
def test_priors_hold_the_gauge_without_a_fixed_vertex(pkg, coarse):
    """fixed = -1: two pose priors, one XYZ prior, a plane prior; Cauchy kernels on the loop edges, two of them far outliers.
    Against the dense inverse of the same (robustly weighted) linearisation."""
    pg, g, lin, H, S = _graph(pkg, ("priors", 130, -1))
    w = pg.edge_robust()["weight"]
    assert (w < 0.05).sum() >= 2  # the two outliers are down-weighted in the system the reference inverts
    vs = [0, 3, 43, 64, 65, 128, 129]
    cov, cross = pg.marginals(vs, cross=True, coarse=coarse, max_iters=MAX_ITERS)
    bound = np.sqrt(6) * mr.column_bound(H, S, TOL)
    err = _block_errors(cov, S, vs).max()
    xerr = max(np.linalg.norm(cross[a, b] - mr.block(S, vs[a], vs[b])) for a in range(len(vs)) for b in range(len(vs)))
    print("coarse %d: block error %.2e, cross %.2e (bound %.2e), iterations max %d" % (coarse, err, xerr, bound, pg.marginal_stats.iters_max))
    assert err <= bound and xerr <= bound
    assert all(c.any() for c in cov)


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
@pytest.mark.parametrize("ref", (0, 70, 129))
def test_relative_covariances_match_the_finite_difference_reference(pkg, ref, coarse):
    """ref fixed, interior and last; the queries include ref (exact zeros) and a duplicate.  Symmetric, smallest eigenvalue not
    below -bound, inside marginals_ref.relative_bound of the reference."""
    pg, g, lin, H, S = _graph(pkg, ("loops", 130, 0))
    js = [1, ref, 69, 71, 129, 0, 35, 71]
    got = pg.relative_covariances(ref, js, coarse=coarse, max_iters=MAX_ITERS)
    st = pg.marginal_stats
    want, J = mr.relative_covariance(S, pg.poses(), ref, js)
    worst = 0.0
    for k, j in enumerate(js):
        if j == ref:
            assert not got[k].any()
            continue
        bound = mr.relative_bound(H, S, J[k], TOL)
        d = np.linalg.norm(got[k] - want[k])
        worst = max(worst, d / bound)
        assert d <= bound, (j, d, bound)
        assert np.array_equal(got[k], got[k].T)
        assert np.linalg.eigvalsh(got[k]).min() >= -bound
    print("ref %d coarse %d: worst error / bound %.3f, iterations max %d" % (ref, coarse, worst, st.iters_max))
    assert np.array_equal(got[3], got[7])
    assert st.columns == 6 * len(set(js) | {ref}) and st.worst_rel_residual <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
def test_relative_covariance_equals_the_marginal_with_the_reference_fixed(pkg, coarse):
    """A pure-relative graph: Sigma_rel(ref, j) is the marginal of j on the same graph re-created with fixed = ref (there the
    estimate of ref is exact and J_j is the identity at zero error), within the sum of both bounds."""
    pg, g, lin, H, S = _graph(pkg, ("loops", 130, 0))
    ref, js = 70, [1, 69, 129, 0]
    rel = pg.relative_covariances(ref, js, coarse=coarse, max_iters=MAX_ITERS)
    _, J = mr.relative_covariance(S, pg.poses(), ref, js)
    pg2 = pkg.PoseGraph(0)
    pg2.set_graph(g["init"], g["ij"], g["meas"], g["info"], fixed=ref)
    H2, S2 = mr.covariance(pg2.linearize(), ref)
    cov = pg2.marginals(js, coarse=coarse, max_iters=MAX_ITERS)
    pg2.close()
    for k in range(len(js)):
        bound = mr.relative_bound(H, S, J[k], TOL) + np.sqrt(6) * mr.column_bound(H2, S2, TOL)
        d = np.linalg.norm(rel[k] - cov[k])
        print("coarse %d, j %d: %.2e (bound %.2e, |Sigma| %.2e)" % (coarse, js[k], d, bound, np.linalg.norm(cov[k])))
        assert d <= bound


def _raw_marginals(pg, vs, n_out, opts=None, ref=None):
    """The C entry points on pattern-filled buffers -> (status, cov buffer, cross buffer)."""
    v = np.ascontiguousarray(vs, np.int32)
    cov = np.full((len(v), 36), -7.25)
    cross = np.full((len(v), len(v), 36), -7.25)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    o = pg._marginal_opts(**(opts or {}))
    vp = v.ctypes.data_as(C.POINTER(C.c_int32))
    if ref is None:
        rc = pg.lib.lslam_pg_marginals(pg.h, len(v), vp, C.byref(o), dp(cov), dp(cross), None)
    else:
        rc = pg.lib.lslam_pg_relative_covariances(pg.h, ref, len(v), vp, C.byref(o), dp(cov), None)
    return rc, cov, cross


def _two_component_graph(pkg, plane_prior):
    """a chain 0 .. 3 with vertex 0 fixed and a chain 4 - 5 - 6 that nothing holds -- or that only a plane prior holds"""
    g = mr.make_chain(7, 9, box=BOX)
    keep = [k for k, (a, b) in enumerate(g["ij"].tolist()) if (a, b) != (3, 4)]
    pg = pkg.PoseGraph(0)
    kw = {}
    if plane_prior:
        pe = g["init"][5]
        ns = po.qrot(po.qconj(pe[3:]), np.array([0.0, 0.0, 1.0]))  # the floor z = 0 as vertex 5 sees it from its estimate
        kw["plane_priors"] = dict(vertex=np.array([5], np.int32), world=np.array([[0.0, 0.0, 1.0, 0.0]]),
                                  meas=np.array([[ns[0], ns[1], ns[2], pe[2]]]), info=np.diag([30.0, 20.0, 50.0])[None])
    pg.set_graph(g["init"], g["ij"][keep], g["meas"][keep], g["info"][keep], fixed=0, **kw)
    pg.build()
    return pg


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", COARSE)
@pytest.mark.parametrize("case", ("out_of_range", "no_gauge", "plane_prior_only", "edge_sharded"))
def test_refusals_write_nothing_and_leave_the_graph_usable(pkg, case, coarse):
    """LSLAM_ERR_INVALID, a message, the pattern-filled outputs untouched -- for both entry points; afterwards the held
    component still answers and the graph still optimises.  The 18 unknowns of the held component converge in far fewer than
    the 50 iterations the plane-prior case allows; the columns of vertex 5 end on p.Hp <= 0 (after 7 iterations, block-Jacobi)
    or on r.z <= 0 (at once, two-level) before the cap -- the system is singular there -- and the message names the vertex and
    says the system is not positive definite."""
    opts = dict(coarse=coarse, max_iters=MAX_ITERS)
    if case == "out_of_range":
        pg, vs = _two_component_graph(pkg, False), [1, 7]
    elif case == "no_gauge":
        pg, vs = _two_component_graph(pkg, False), [1, 5]
    elif case == "plane_prior_only":
        pg, vs = _two_component_graph(pkg, True), [1, 5]
        opts["max_iters"] = 50  # the cap is what ends it
    else:
        pg, vs = _two_component_graph(pkg, False), [1, 2]
        pg.set_shard(0, 2)
    for ref in (None, 2):
        rc, cov, cross = _raw_marginals(pg, vs, len(vs), opts, ref=ref)
        msg = pg.lib.lslam_pg_last_error().decode()
        print("%s, coarse %d, ref %s: %d %s" % (case, coarse, ref, rc, msg))
        assert rc == int(pkg.Status.ERR_INVALID) and msg
        assert (cov == -7.25).all() and (cross == -7.25).all()
        if case in ("no_gauge", "plane_prior_only"):
            assert "vertex 5" in msg
        if case == "plane_prior_only":
            assert "not positive definite" in msg or "did not reach the tolerance" in msg
    if case == "edge_sharded":
        pg.set_shard(0, len(pg._ij))
    ok = pg.marginals([1, 2], coarse=coarse, max_iters=MAX_ITERS)  # the held component still answers ...
    assert ok.any()
    pg.optimize(5)  # ... and the graph still optimises
    assert pg.last_stats.chi2_final <= pg.last_stats.chi2_initial
    pg.close()


@pytest.mark.gpu
def test_default_options(pkg):
    """No options at all = {rel_tol 0, max_iters 0, coarse -1} = the solver's tolerance spelled out: the same bits; on a
    graph whose solves never switched the second level on, coarse -1 is block-Jacobi."""
    pg, g, lin, H, S = _graph(pkg, ("chain", 7, 0))
    a = pg.marginals([3, 6])
    st = pg.marginal_stats
    assert st.coarse_used == 0 and st.iters_max <= 100 and st.worst_rel_residual <= TOL
    b = pg.marginals([3, 6], rel_tol=0.0, max_iters=0, coarse=-1)
    c = pg.marginals([6, 3], rel_tol=TOL, coarse=0)
    assert np.array_equal(a, b) and np.array_equal(a, c[::-1])
    loose = pg.marginals([3, 6], rel_tol=1e-3)
    assert pg.marginal_stats.iters_max < st.iters_max and pg.marginal_stats.worst_rel_residual <= 1e-3
    assert np.abs(loose - a).max() > 0.0


@pytest.mark.gpu
def test_optimise_after_marginals_is_the_optimise_without(pkg):
    """The call leaves the graph as lslam_pg_linearize leaves it: the LM run after it ends at the same poses, bit for bit."""
    g = mr.make_chain(43, 143, box=BOX)
    out = []
    for ask in (False, True):
        pg = pkg.PoseGraph(0)
        pg.set_graph(g["init"], g["ij"], g["meas"], g["info"], fixed=0)
        if ask:
            pg.marginals([1, 20, 42], coarse=1, max_iters=MAX_ITERS)
            pg.relative_covariances(3, [4, 40], coarse=0, max_iters=MAX_ITERS)
        pg.optimize(8)
        out.append(pg.poses())
        pg.close()
    assert np.array_equal(out[0], out[1])
