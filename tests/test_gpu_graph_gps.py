"""The graph node with GPS fixes (Graph(gps_sigma=...), add_frame(utm_coord=...)) on tests/posegraph_prior_ref.py's L-shaped
path: 30 keyframes, no revisit, odometry with a constant yaw bias, the start heading 90 degrees from ENU, UTM offsets of 5e5 /
4e6 m.  The conditions on the inputs (when the fixes span a plane, that the reference LM alone halves the error, that the
compared LM prefix is usable) are asserted on the CPU by tests/test_posegraph_prior_ref.py; nothing here was calibrated against
the GPU.  Each test prints its figures before it asserts."""
import numpy as np
import pytest

import posegraph_prior_ref as ppr
import posegraph_se3 as se3


def _positions(g):
    return np.array([kf.estimate[:3, 3] for kf in g.keyframes])


@pytest.mark.gpu
def test_fixes_are_queued_until_they_span_a_plane_then_bound_the_drift(pkg, ctx):
    """No prior reaches the solver before the spread condition; at that point all queued ones do and the solver is rebuilt
    with fixed = -1.  The RMS position error to ground truth is at most half that of the same run without gps_sigma (a
    condition, met by the reference alone on the CPU).  With gps_sigma=None, add_frame(..., utm_coord=...) changes nothing:
    poses and edges bit-identical to a run without the argument."""
    sc = ppr.graph_gps_scenario()
    g = pkg.Graph(ctx=ctx, gps_sigma=ppr.GRAPH_GPS_SIGMA)
    trace = ppr.drive_graph(g, sc, ppr.GRAPH_GPS_ITERS)
    first = next(k for k, (n_p, _) in enumerate(trace) if n_p > 0)
    assert not g.loops and len(g.keyframes) == 30
    assert all(t == (0, 0) for t in trace[:first]) and trace[first] == (first + 1, -1) and trace[-1] == (30, -1)
    assert g.solver.num_priors == 30 and g.gps_aligned and (g.gps_weights() == 1.0).all() and not g.rejected_fixes()
    truth = sc["gt"][:, :3, 3] + np.array(ppr.GRAPH_GPS_UTM) - g.utm_origin
    with_gps = ppr.rms_position_error(_positions(g), truth)
    off = pkg.Graph(ctx=ctx)
    ppr.drive_graph(off, sc, ppr.GRAPH_GPS_ITERS)
    plain = pkg.Graph(ctx=ctx)
    ppr.drive_graph(plain, sc, ppr.GRAPH_GPS_ITERS, with_fixes=False)
    in_first = np.array([np.linalg.inv(sc["gt"][0]) @ T for T in sc["gt"]])[:, :3, 3]
    without = ppr.rms_position_error(_positions(off), in_first)
    print("priors reach the solver at keyframe %d; RMS position error with GPS %.3f m, without %.3f m" % (first, with_gps, without))
    assert with_gps <= 0.5 * without
    assert off.solver.num_priors == 0 and off.solver.fixed == 0 and off.utm_origin is None
    assert np.array_equal(np.array([k.estimate for k in off.keyframes]).view(np.int64), np.array([k.estimate for k in plain.keyframes]).view(np.int64))
    assert off.solver._ij == plain.solver._ij and np.array_equal(np.stack(off.solver._meas), np.stack(plain.solver._meas))
    assert np.array_equal(off.tf_odom2graph, plain.tf_odom2graph)
    # The node's final state against the reference LM on the same edges and priors, run from the bookkeeping-only start until
    # it stops.  The node optimised pass by pass, GRAPH_GPS_ITERS iterations at the most each; the reference's own distance
    # from where it stops after that many iterations is the floor (GRAPH_GPS_CONVERGENCE_*, measured on the CPU), ten times it
    # the bound.
    book = pkg.Graph(ctx=ctx, gps_sigma=ppr.GRAPH_GPS_SIGMA)
    ppr.drive_graph(book, sc, 0)
    gg, pr = ppr.graph_arrays(book)
    ref, hist = ppr.optimize(gg, pr, -1, 300)
    fg, fpr = ppr.graph_arrays(g)
    assert len(hist) < 300 and np.array_equal(fg["ij"], gg["ij"]) and np.array_equal(fpr["meas"], pr["meas"])
    chi_node = ppr.total_chi2(fg["init"], fg, fpr)
    d_pose, d_chi = float(np.abs(fg["init"] - ref).max()), abs(chi_node - hist[-1]["chi2"]) / hist[-1]["chi2"]
    print("node's final state against the reference LM where it stops: poses %.3e (bound %.3e) chi2 %.12g / %.12g: %.3e (bound %.3e)" % (
        d_pose, 10 * ppr.GRAPH_GPS_CONVERGENCE_POSES, chi_node, hist[-1]["chi2"], d_chi, 10 * ppr.GRAPH_GPS_CONVERGENCE_CHI2))
    assert d_pose <= 10 * ppr.GRAPH_GPS_CONVERGENCE_POSES and d_chi <= 10 * ppr.GRAPH_GPS_CONVERGENCE_CHI2
    # the last keyframe's fix and tf_odom2graph: odometry is corrected onto ENU
    last = g.tf_odom2graph @ sc["odom"][-1]
    assert np.linalg.norm(last[:3, 3] - truth[-1]) <= 10 * max(ppr.GRAPH_GPS_SIGMA)


@pytest.mark.gpu
def test_solver_follows_the_reference_lm_on_the_graphs_edges_and_priors(pkg, ctx):
    """The node's bookkeeping alone (the solver never run: keyframes, odometry edges, the alignment, the priors), then
    GRAPH_GPS_LM_ITERS LM iterations of the solver against the numpy reference LM on the same edges and priors: the same
    trials, poses within the LM bound of tests/test_gpu_posegraph_priors.py (max of 10 x the reference's spread under solves
    that stop at the PCG's residual and 1e-8 x path length)."""
    sc = ppr.graph_gps_scenario()
    g = pkg.Graph(ctx=ctx, gps_sigma=ppr.GRAPH_GPS_SIGMA)
    ppr.drive_graph(g, sc, 0)
    gg, pr = ppr.graph_arrays(g)
    r = ppr.lm_run(gg, pr, -1, ppr.GRAPH_GPS_LM_ITERS)
    assert r["pcg_same_trials"]
    its = g.solver.optimize(ppr.GRAPH_GPS_LM_ITERS)
    st, got = g.solver.last_stats, g.solver.poses()
    tol = max(10 * r["pcg_spread"], se3.PCG_TOL * r["path"])
    err = float(np.abs(got - r["poses"]).max())
    print("trials gpu %d reference %s pose error %.3e bound %.3e chi2 %.12g / %.12g" % (st.lm_trials, r["trials"], err, tol, st.chi2_final, r["chi2"][-1]))
    assert its == ppr.GRAPH_GPS_LM_ITERS and st.lm_trials == sum(r["trials"])
    assert abs(st.chi2_initial - r["chi2"][0]) <= 10 * se3.O2O_CHI2 * r["chi2"][0]
    assert err <= tol


@pytest.mark.gpu
def test_utm_origin_handling_loses_nothing(pkg, ctx):
    """Every fix shifted by 1e6 m changes the node's final poses by no more than the fp64 rounding of fix - origin.  What that
    rounding does is measured on the reference alone (tests/test_posegraph_prior_ref.py, floors GRAPH_GPS_SHIFT_*: the priors'
    measurements 4.7e-10 m, the aligned estimates 7.0e-10, the reference LM's poses 3.0e-9, tf_odom2graph made from them
    6.3e-8; ulp of 5e6 m: 9.3e-10); the node -- driven pass by pass, the solver's final poses and its tf_odom2graph -- is allowed
    ten times those, and the measurements, host arithmetic, one ulp."""
    runs = []
    for shift in (0.0, 1.0e6):
        sc = ppr.graph_gps_scenario(shift)
        book = pkg.Graph(ctx=ctx, gps_sigma=ppr.GRAPH_GPS_SIGMA)
        ppr.drive_graph(book, sc, 0)
        gg, pr = ppr.graph_arrays(book)
        g = pkg.Graph(ctx=ctx, gps_sigma=ppr.GRAPH_GPS_SIGMA)
        ppr.drive_graph(g, sc, ppr.GRAPH_GPS_ITERS)
        runs.append((gg, pr, g.solver.poses(), g.tf_odom2graph))
    (g0, p0, x0, t0), (g1, p1, x1, t1) = runs
    d_meas, d_init = float(np.abs(p0["meas"] - p1["meas"]).max()), float(np.abs(g0["init"] - g1["init"]).max())
    d_pose, d_tf = float(np.abs(x0 - x1).max()), float(np.abs(t0 - t1).max())
    print("shift 1e6 m: priors move %.3e m, aligned estimates %.3e, the solver's final poses %.3e, tf_odom2graph %.3e (bounds %.3e %.3e %.3e %.3e)" % (
        d_meas, d_init, d_pose, d_tf, float(np.spacing(5.0e6)), 10 * ppr.GRAPH_GPS_SHIFT_INIT, 10 * ppr.GRAPH_GPS_SHIFT_POSES, 10 * ppr.GRAPH_GPS_SHIFT_TF))
    assert d_meas <= np.spacing(5.0e6) and d_init <= 10 * ppr.GRAPH_GPS_SHIFT_INIT
    assert d_pose <= 10 * ppr.GRAPH_GPS_SHIFT_POSES and d_tf <= 10 * ppr.GRAPH_GPS_SHIFT_TF
