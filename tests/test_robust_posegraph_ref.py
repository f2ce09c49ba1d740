"""tests/robust_posegraph_ref.py, the reference for robust kernels on pose-graph edges, checked against itself: the kernels'
derivatives and thresholds, the floors that the GPU tolerances are ten times of (figures: the module's docstring), and the two
outlier scenarios.  CPU only.  Parity with g2o is unpinned (it is not available); the formulas are its published ones."""
import numpy as np
import pytest

import posegraph_se3 as se3
import robust_posegraph_ref as rr

po = se3.po
FLOOR_CASES = [c for c in se3.LIN_CASES if c[0] in (2, 64, 400) or (c[0] == 7 and c[4])]
_ids = lambda c: "n%d_seed%d_fixed%d%s" % (c[0], c[2], c[3], "_iso" if c[4] else "")  # noqa: E731


@pytest.mark.parametrize("kind,delta", [(rr.HUBER, 0.7), (rr.HUBER, 3.0), (rr.CAUCHY, 0.1), (rr.CAUCHY, 2.0)])
def test_rho1_is_the_derivative_of_rho0_for_huber_and_cauchy(kind, delta):
    """Central differences of rho0 in e2, on both sides of Huber's threshold delta^2 (never across it).  Step
    h = 1e-5 (e2 + delta^2), the scale on which both kernels vary (Cauchy's argument a = 1 + e2 / delta^2 is rounded at eps
    whatever e2 is): rounding eps (e2 + delta^2) / h = 2e-11 and truncation (h / (e2 + delta^2))^2 = 1e-10 of rho1; bound 1e-8."""
    t = delta * delta
    e2 = np.concatenate([t * np.array([1e-3, 0.1, 0.5, 0.99]), t * np.array([1.01, 2.0, 10.0, 1e3])])
    h = 1e-5 * (e2 + t)
    num = (rr.rho(kind, delta, e2 + h)[0] - rr.rho(kind, delta, e2 - h)[0]) / (2 * h)
    r1 = rr.rho(kind, delta, e2)[1]
    print(kind, delta, np.abs(num / r1 - 1).max())
    assert np.abs(num / r1 - 1).max() <= 1e-8
    if kind == rr.HUBER:
        assert np.array_equal(r1[:4], np.ones(4)) and (r1[4:] < 1).all()


def test_dcs_rho1_is_g2os_and_not_the_derivative():
    """g2o's DCS returns rho1 = s^2; d rho0 / d e2 = s^2 (delta - e2) / (delta + e2) is something else (negative beyond
    e2 = delta).  The closed form: rho0 = 4 delta^2 e2 / (delta + e2)^2 beyond the threshold e2 = delta."""
    d = 1.5
    e2 = np.array([0.1, 1.0, 1.5, 1.6, 3.0, 50.0])
    r0, r1 = rr.rho(rr.DCS, d, e2)
    far = e2 > d
    assert np.array_equal(r0[~far], e2[~far]) and np.array_equal(r1[~far], np.ones((~far).sum()))
    assert np.allclose(r0[far], 4 * d * d * e2[far] / (d + e2[far]) ** 2, rtol=2e-15, atol=0)  # half a dozen roundings each way
    assert np.allclose(r1[far], 4 * d * d / (d + e2[far]) ** 2, rtol=2e-15, atol=0)
    h = 1e-6 * e2[far]
    num = (rr.rho(rr.DCS, d, e2[far] + h)[0] - rr.rho(rr.DCS, d, e2[far] - h)[0]) / (2 * h)
    assert (num < 0).all() and (r1[far] > 0).all()  # rho0 falls beyond e2 = delta while the weight stays positive
    assert np.allclose(num, r1[far] * (d - e2[far]) / (d + e2[far]), rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind,delta", [(rr.HUBER, 0.7), (rr.HUBER, 1e150), (rr.DCS, 1.0), (rr.DCS, 0.03)])
def test_huber_and_dcs_are_continuous_at_their_thresholds(kind, delta):
    """rho0 and rho1 one ulp below, at and one ulp above the threshold (Huber: e2 = delta^2, DCS: e2 = delta) agree to a few
    ulp: both branches give (e2, 1) there."""
    thr = delta * delta if kind == rr.HUBER else delta
    e2 = np.array([np.nextafter(thr, 0.0), thr, np.nextafter(thr, np.inf)])
    r0, r1 = rr.rho(kind, delta, e2)
    assert np.abs(r0 / e2 - 1).max() <= 8 * np.finfo(float).eps and np.abs(r1 - 1).max() <= 8 * np.finfo(float).eps
    assert r0[1] == thr and r1[1] == 1.0  # the threshold itself is on the quadratic side


@pytest.mark.parametrize("case", FLOOR_CASES, ids=_ids)
def test_kind_none_reproduces_the_plain_oracle_bit_for_bit(case):
    g = se3.graph(case)
    ne = len(g["ij"])
    w = rr.weighted_system(g, np.zeros(ne, np.int32), np.ones(ne))
    c = se3.c_system(g)
    for k in ("diag", "off", "b"):
        assert np.array_equal(w[k].view(np.int64), c[k].view(np.int64)), k
    assert np.array_equal(w["weight"], np.ones(ne)) and np.array_equal(w["rho"], w["e2"])
    assert abs(w["chi2"] - c["chi2"]) <= se3.SPREAD_CHI2 * c["chi2"]  # summed here per edge, there in the oracle's loop


@pytest.mark.parametrize("case", FLOOR_CASES, ids=_ids)
def test_floor_a_weighted_system_under_edge_permutations(case):
    """Floor (a): the C-oracle weighted system against itself with its edges permuted (eight permutations), weights from the
    C oracle's own per-edge chi2; per edge, the C oracle's e2 / rho0 / weight against numpy's.  Measured figures in the
    reference's docstring; asserted at the recorded W_SPREAD_* / W_EDGE_*."""
    g = se3.graph(case)
    kinds, deltas = rr.kernel_mix(g)
    ref = rr.weighted_system(g, kinds, deltas)
    if case[0] >= 64:  # every robust kind meets edges on both sides of its threshold
        assert all(min(v) >= 5 for v in rr.sides(kinds, deltas, ref["e2"]).values()), rr.sides(kinds, deltas, ref["e2"])
    rng = np.random.default_rng(100 + case[2])
    for _ in range(8):
        d = se3.differences(rr.weighted_system(g, kinds, deltas, order=rng.permutation(len(kinds))), ref)
        print(case, d)
        assert d["diag"] <= rr.W_SPREAD_H and d["off"] <= rr.W_SPREAD_H and d["b"] <= rr.W_SPREAD_B and d["chi2"] <= rr.W_SPREAD_CHI2, d
    e2n = rr.edge_e2(g, source="np")
    r0n, r1n = rr.rho_edges(kinds, deltas, e2n)
    pe = [float(np.abs(a / b - 1).max()) for a, b in ((e2n, ref["e2"]), (r0n, ref["rho"]), (r1n, ref["weight"]))]
    print(case, "per edge, numpy against C: e2 %.2e rho0 %.2e weight %.2e" % tuple(pe))
    assert pe[0] <= rr.W_EDGE_E2 and pe[1] <= rr.W_EDGE_RHO and pe[2] <= rr.W_EDGE_WEIGHT, pe


@pytest.mark.parametrize("case", FLOOR_CASES, ids=_ids)
def test_floor_b_c_weighted_against_numpy_weighted(case):
    """Floor (b): analytic Jacobians + C assembly against central differences + scipy assembly, each weighting with its own
    e2.  Measured H 1.5e-10 max|H|, b 1.3e-10 max|b|, sum rho0 2.3e-15; asserted at the recorded W_O2O_*."""
    g = se3.graph(case)
    kinds, deltas = rr.kernel_mix(g)
    d = se3.differences(rr.weighted_system(g, kinds, deltas), rr.weighted_system(g, kinds, deltas, oracle="np"))
    print(case, d)
    assert d["h"] <= rr.W_O2O_H and d["b"] <= rr.W_O2O_B and d["chi2"] <= rr.W_O2O_CHI2, d


@pytest.mark.parametrize("name", list(rr.SCENARIOS))
def test_corruption_is_as_specified(name):
    g, gc, bad, loops = rr.outlier_scenario(name)
    sc = rr.SCENARIOS[name]
    assert len(bad) == sc["nbad"] and len(loops) == sc["n_loop"] and np.isin(bad, loops).all()
    same = np.setdiff1d(np.arange(len(g["ij"])), bad)
    assert np.array_equal(g["meas"][same], gc["meas"][same]) and np.array_equal(g["init"], gc["init"])
    rel = po.pose_mul(po.pose_inv(g["meas"][bad]), gc["meas"][bad])
    assert (np.abs(rel[:, :3]) >= 2.0 - 1e-12).all() and (np.abs(rel[:, :3]) <= 6.0 + 1e-12).all()


@pytest.mark.parametrize("kernel", list(rr.SCENARIO_KERNELS))
@pytest.mark.parametrize("name", list(rr.SCENARIOS))
def test_outlier_scenarios_the_kernel_rejects_exactly_the_corrupted_loops(name, kernel):
    """The reference alone: DCS phi = 1 and Cauchy delta = 0.1 on the loop edges end with every corrupted loop below weight
    0.05 and every other loop above 0.9; the kernel's max position error against ground truth is below twice the clean
    graph's, the plain run's above five times it.  Figures in the reference's docstring."""
    r = rr.scenario_reference(name, kernel)
    clean_err, plain_err = rr.scenario_baselines(name)
    w, bad = r["weights"], r["bad"]
    good = np.setdiff1d(r["loops"], bad)
    print(name, kernel, "clean %.3f plain %.3f robust %.3f" % (clean_err, plain_err, r["robust_err"]), "bad weights",
          w[bad], "least good weight", w[good].min(), "iterations", len(r["hist"]), "trials", [h["trials"] for h in r["hist"]])
    assert (w[bad] < 0.05).all() and (w[good] > 0.9).all()
    assert np.array_equal(w[:r["gc"]["n_odo"]], np.ones(r["gc"]["n_odo"]))  # odometry edges carry no kernel
    assert r["robust_err"] < 2 * clean_err and plain_err > 5 * clean_err
    assert abs(clean_err - rr.SCENARIO_CLEAN_ERR[name]) <= 1e-3  # the figure the GPU tests take from the reference module


@pytest.mark.parametrize("kernel", list(rr.SCENARIO_KERNELS))
@pytest.mark.parametrize("name", list(rr.SCENARIOS))
def test_scenario_spread_is_as_recorded(name, kernel):
    """optimize_robust against itself with the edges permuted and with damped solves that stop at the PCG's residual: final
    positions and final sum rho0 stay inside the recorded SCENARIO_SPREAD, which the GPU comparison takes ten times.  The
    accept / reject sequences of these runs differ (the reference's docstring), so only final values are recorded."""
    dpos, dchi, same = rr.scenario_spread(name, kernel)
    print(name, kernel, "position spread %.3e m, sum rho0 spread %.3e, same trials: %s" % (dpos, dchi, same))
    rec = rr.SCENARIO_SPREAD[(name, kernel)]
    assert dpos <= rec[0] and dchi <= rec[1]
