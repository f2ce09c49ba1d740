"""The pose-graph node with floor planes (Graph(floor_sigma=...)): a 10-keyframe L-shaped path on flat ground whose odometry
drifts in z and pitch (floor_ref.graph_floor_scenario), NoLoops detector.  The planes that reach the solver are the reference
detection's; the optimised estimates are the dense reference LM's on the same edges and plane priors; z and pitch errors fall as
far as the reference LM makes them fall; without the switch nothing changes; an all-wall keyframe is counted and adds nothing; a
ramp taken for the floor loses its weight under Cauchy."""
import numpy as np
import pytest

import floor_ref as F
import posegraph_prior_ref as ppr

pytestmark = pytest.mark.gpu


def _graph(pkg, ctx, resident=False, **kw):
    if resident:
        return pkg.Graph(ctx=ctx, resident=True, floor_params=F.GRAPH_FLOOR_PARAMS, **kw)
    return pkg.Graph(ctx=ctx, loop_detector=ppr.NoLoops(), floor_params=F.GRAPH_FLOOR_PARAMS, **kw)


def _assert_planes_are_the_reference_detections(g, sc):
    p = F.params(**F.GRAPH_FLOOR_PARAMS)
    for kf, idx in g.floors:
        ref = F.detect(sc["clouds"][kf.node][1], p)
        assert ref["status"] == F.FLOOR_OK
        plane, w, N, E = ref["refits"][-1]
        rn, rd = F.refit_bounds(N, E, w)
        got = g.solver._plane_priors[idx]["meas"]
        err = np.abs(got - ref["plane"])
        assert err[:3].max() <= rn and err[3] <= rd, (kf.node, err, rn, rd)
        assert np.array_equal(kf.floor_coeffs, got) and g.solver._plane_priors[idx]["vertex"] == kf.node
        assert np.array_equal(g.solver._plane_priors[idx]["world"], [0.0, 0.0, 1.0, 0.0])


@pytest.mark.parametrize("resident", [False, True], ids=["host_clouds", "resident_store"])
def test_floors_bound_the_drift_as_the_reference_lm_does(pkg, ctx, resident):
    sc = F.graph_floor_scenario()
    n = len(sc["gt"])
    g = _graph(pkg, ctx, resident, floor_sigma=F.GRAPH_FLOOR_SIGMA)
    before = g.store.info() if resident else None
    F.drive_floor_graph(g, sc, F.GRAPH_FLOOR_ITERS)
    assert len(g.floors) == n and not g.floors_not_found and g.solver.num_plane_priors == n and g.solver.num_priors == 0
    if resident:  # detection moved no cloud: the uploads are the keyframes' own, nothing came down
        after = g.store.info()
        assert after["cloud_bytes_downloaded"] == before["cloud_bytes_downloaded"] == 0
        assert after["cloud_bytes_uploaded"] == sum((len(c) + len(s)) * 16 for c, s in sc["clouds"])
    _assert_planes_are_the_reference_detections(g, sc)
    assert (g.floor_weights() == 1.0).all() and g.rejected_floors() == []
    # the dense reference LM on the same edges and plane priors, from the bookkeeping-only start, at two stopping tolerances
    book = _graph(pkg, ctx, False, floor_sigma=F.GRAPH_FLOOR_SIGMA)
    F.drive_floor_graph(book, sc, 0)
    gg = F.graph_edges(book)
    pl = F.graph_planes(book)
    assert np.array_equal(pl["vertex"], F.graph_planes(g)["vertex"])
    loose, _ = F.plane_optimize(gg, None, pl, gg["fixed"], 300, rel_tol=1e-9)
    tight, hist = F.plane_optimize(gg, None, pl, gg["fixed"], 300, rel_tol=1e-13)
    spread = float(np.abs(loose - tight).max())
    path = float(np.abs(tight - gg["init"]).sum(0).max())
    tol = max(10 * spread, 1e-8 * path)
    got = g.solver.poses()
    err = float(np.abs(got - tight).max())
    print("estimates against the reference LM: %.3e, bound %.3e (spread between two stopping tolerances %.3e, path %.3e)" % (err, tol, spread, path))
    assert err <= tol
    # z and pitch: the drift against what is left, on the reference first, then on the node by the reference's factor
    z0, t0 = F.z_pitch_errors(gg["init"], sc["gt"])
    zr, tr = F.z_pitch_errors(tight, sc["gt"])
    zg, tg = F.z_pitch_errors(got, sc["gt"])
    print("z error: drift %.3f m, reference LM %.4f m, node %.4f m; tilt: drift %.4f rad, reference LM %.5f, node %.5f" % (
        z0.max(), zr.max(), zg.max(), t0.max(), tr.max(), tg.max()))
    assert zr.max() < z0.max() / 5 and tr.max() < t0.max() / 5, "the scenario must show the effect on the reference"
    assert zg.max() <= zr.max() + tol and tg.max() <= tr.max() + tol  # the reference's factor, to the LM bound


def test_without_the_switch_nothing_changes(pkg, ctx):
    """No floor_sigma: no detection, no plane prior, and the estimates are bit-equal to a Graph that was never given the floor
    arguments at all (the odometry-only graph is never optimised: the estimates are the bookkeeping's)."""
    sc = F.graph_floor_scenario()
    off = _graph(pkg, ctx, False)
    plain = pkg.Graph(ctx=ctx, loop_detector=ppr.NoLoops())
    F.drive_floor_graph(off, sc, F.GRAPH_FLOOR_ITERS)
    F.drive_floor_graph(plain, sc, F.GRAPH_FLOOR_ITERS)
    assert off.solver.num_plane_priors == 0 and off.floors == [] and off.floors_not_found == []
    assert all(not hasattr(k, "floor_coeffs") for k in off.keyframes)
    a, b = np.array([k.estimate for k in off.keyframes]), np.array([k.estimate for k in plain.keyframes])
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(off.tf_odom2graph, plain.tf_odom2graph)
    assert off.solver._ij == plain.solver._ij


def test_an_all_wall_keyframe_is_counted_and_adds_nothing(pkg, ctx):
    sc = F.graph_floor_scenario(all_wall=4)
    g = _graph(pkg, ctx, False, floor_sigma=F.GRAPH_FLOOR_SIGMA)
    F.drive_floor_graph(g, sc, F.GRAPH_FLOOR_ITERS)
    n = len(sc["gt"])
    assert len(g.floors) == n - 1 and g.solver.num_plane_priors == n - 1
    assert [(kf.node, st) for kf, st in g.floors_not_found] == [(4, F.FLOOR_NO_HYPOTHESIS)]
    assert g.keyframes[4].floor_coeffs is None and 4 not in [q["vertex"] for q in g.solver._plane_priors]
    assert F.detect(sc["clouds"][4][1], F.params(**F.GRAPH_FLOOR_PARAMS))["status"] == F.FLOOR_NO_HYPOTHESIS
    _assert_planes_are_the_reference_detections(g, sc)


def test_a_ramp_taken_for_the_floor_loses_its_weight_under_cauchy(pkg, ctx):
    """Keyframe 6's ground patch is tilted by 0.08 rad (inside the detector's 10 degrees: accepted); exact odometry whose
    information is worth something, Graph(odometry_information=floor_ref.GRAPH_FLOOR_STRONG_ODOMETRY) -- with the node's constant
    one NO kernel can reject, bending is cheaper (the Graph's docstring says so).  Asserted on the reference first: with Cauchy the
    ramp's weight falls below 0.1 and the others stay above 0.9; without a kernel every weight is 1 and the trajectory tilts with
    the ramp."""
    sc = F.graph_floor_scenario(tilted=6, drift=False)
    out = {}
    for kernel in (None, "Cauchy"):
        kw = dict(floor_sigma=F.GRAPH_FLOOR_SIGMA, floor_robust_kernel=kernel, floor_robust_delta=1.0, odometry_information=F.GRAPH_FLOOR_STRONG_ODOMETRY)
        g = _graph(pkg, ctx, False, **kw)
        F.drive_floor_graph(g, sc, F.GRAPH_FLOOR_ITERS)
        assert len(g.floors) == len(sc["gt"])
        book = _graph(pkg, ctx, False, **kw)
        F.drive_floor_graph(book, sc, 0)  # the reference LM starts where the node's bookkeeping leaves the estimates
        pl, gg = F.graph_planes(book), F.graph_edges(book)
        assert np.array_equal(gg["info"][0], F.GRAPH_FLOOR_STRONG_ODOMETRY)
        ref, _ = F.plane_optimize(gg, None, pl, gg["fixed"], 300, rel_tol=1e-12)
        out[kernel] = dict(w=g.floor_weights(), ref_w=F.plane_rho(ref, pl)[2], rejected=[k.node for k in g.rejected_floors()],
                           tilt=F.z_pitch_errors(g.solver.poses(), sc["gt"])[1].max(), ref_tilt=F.z_pitch_errors(ref, sc["gt"])[1].max())
    w, rw = out["Cauchy"]["w"], out["Cauchy"]["ref_w"]
    print("Cauchy: weight of the ramp %.3e (reference %.3e), others min %.4f (reference %.4f); tilt error plain %.4f rad (reference %.4f), Cauchy %.5f rad (reference %.5f)" % (
        w[6], rw[6], np.delete(w, 6).min(), np.delete(rw, 6).min(), out[None]["tilt"], out[None]["ref_tilt"], out["Cauchy"]["tilt"], out["Cauchy"]["ref_tilt"]))
    assert rw[6] < 0.1 and np.delete(rw, 6).min() > 0.9 and out[None]["ref_tilt"] > 2 * out["Cauchy"]["ref_tilt"], "the scenario must show the effect on the reference"
    assert w[6] < 0.1 and np.delete(w, 6).min() > 0.9 and out["Cauchy"]["rejected"] == [6]
    assert (out[None]["w"] == 1.0).all() and out[None]["rejected"] == []
    assert out[None]["tilt"] > 2 * out["Cauchy"]["tilt"]
