"""Reference for robust kernels on pose-graph edges (test infrastructure only; CPU, numpy fp64), shared by
tests/test_robust_posegraph_ref.py (CPU) and tests/test_gpu_robust_posegraph.py (GPU).

PARITY UNPINNED, like the rest of the pose-graph solver: g2o is not available here.  The semantics restated are g2o's
published ones (BaseBinaryEdge::constructQuadraticForm, robust_kernel_impl.cpp): with e2 = e^T Omega e and parameter delta,
rho = (rho0, rho1) is
  NONE (e2, 1);  HUBER e2 <= delta^2: (e2, 1), else (2 delta sqrt(e2) - delta^2, delta / sqrt(e2));
  CAUCHY a = e2 / delta^2 + 1: (delta^2 ln a, 1 / a);  DCS s = 2 delta / (delta + e2): s >= 1: (e2, 1), else (s^2 e2, s^2)
and the edge adds rho1 J^T Omega J to H, -rho1 J^T Omega e to b, rho0 to chi2 (no rho2 term).  DCS's rho1 is g2o's, not the
derivative of its rho0.  H and b are linear in Omega, so the weighted system is the existing oracles' system of the graph
with Omega_e replaced by rho1_e Omega_e: tests/posegraph_se3.c_system / np_system are reused unchanged.

MEASURED FLOORS of this reference (tests/test_robust_posegraph_ref.py asserts that it stays inside them; the GPU tests use
ten times them; nothing here was calibrated against the GPU).  Graphs: posegraph_se3.LIN_CASES with n in {2, 7 (isolated),
64, 400}, kind e % 4 on edge e, delta from the median of e2 (kernel_mix), eight edge permutations each:
  (a) weighted_system through the C oracle against itself with its edges permuted, the weights computed from the C
      oracle's own per-edge chi2: diag 2.8e-16 max|diag|, off 1.3e-16 max|off|, b 1.9e-16 max|b|, sum rho0 3.0e-16.
      A permutation does not move a per-edge value; the spread a reference has per edge is that of its two evaluations, the
      C oracle's e2 against numpy's: e2 1.6e-14 e2, rho0 1.6e-14 rho0, weight 3.9e-15 weight
  (b) C-weighted against numpy-weighted (each with its own e2): H 1.5e-10 max|H|, b 1.3e-10 max|b|, sum rho0 2.3e-15
The weight inherits e2's relative spread (|d rho1 / rho1| <= |d e2 / e2| for all three kernels), so (a) was expected a
little above posegraph_se3.SPREAD_*; measured on these cases it is below them (sum rho0 is summed pairwise by numpy, the C
oracle's chi2 in a running loop).  Every recorded figure is set just above its measurement.

OUTLIER SCENARIOS (the two rows of the table in DESIGN's pose-graph section): make_graph(laps=2, radius=15) with a few loop
measurements displaced by 2 - 6 m per axis (outlier_scenario).  optimize_robust's own spread on them -- the edges permuted
(three permutations), and every damped solve replaced by A^-1 (b + r), |r| = PCG_TOL |b| (three random r), what a PCG that stops
at that residual may return -- is recorded in SCENARIO_SPREAD below.  Measured (position in m, relative sum rho0):
  kf120 DCS 4.7e-7, 4.3e-10;  kf120 Cauchy 6.2e-7, 1.2e-15;  kf60 DCS 2.0e-6, 7.2e-8;  kf60 Cauchy 2.9e-7, 1.4e-15.
The LM accept / reject sequences of those CPU runs DIFFER from the unperturbed run's in three of the four (kf60 DCS keeps
its [1, 4, 10]): the runs end on a flat sum rho0, where a rejected trial is rounding noise.  So the GPU run is compared by
its final values only, not by its iteration and trial counts.
Reference figures (max position error against ground truth, m): kf120 clean 0.735, plain 7.348, DCS 0.858, Cauchy 0.844;
kf60 clean 0.349, plain 15.037, DCS 0.463, Cauchy 0.309.  Final weights: DCS bad <= 5.9e-4, good exactly 1; Cauchy bad
<= 1.2e-4, good >= 0.955.
"""
import numpy as np

import posegraph_se3 as se3

po, pc = se3.po, se3.pc

NONE, HUBER, CAUCHY, DCS = 0, 1, 2, 3

# ---- recorded floors (relative; see the module docstring) ----------------------------------------------------------------------
W_SPREAD_H = 3.0e-16      # (a) diag / max|diag|, off / max|off|
W_SPREAD_B = 2.0e-16      # (a) b / max|b|
W_SPREAD_CHI2 = 3.5e-16   # (a) sum rho0
W_EDGE_E2 = 2.0e-14       # (a) per edge, C oracle against numpy: e2 / e2
W_EDGE_RHO = 2.0e-14      # ... rho0 / rho0
W_EDGE_WEIGHT = 5.0e-15   # ... weight / weight
W_O2O_H = 1.6e-10         # (b) H / max|H|
W_O2O_B = 1.4e-10         # (b) b / max|b|
W_O2O_CHI2 = 2.5e-15      # (b) sum rho0


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
def rho(kind, delta, e2):
    """(rho0, rho1) of e2 under one kernel; e2 an array."""
    e2 = np.asarray(e2, np.float64)
    if kind == NONE:
        return e2.copy(), np.ones_like(e2)
    if kind == HUBER:
        out = e2 > delta * delta
        sq = np.sqrt(np.where(out, e2, 1.0))
        return np.where(out, 2.0 * delta * sq - delta * delta, e2), np.where(out, delta / sq, 1.0)
    if kind == CAUCHY:
        a = e2 / (delta * delta) + 1.0
        return delta * delta * np.log(a), 1.0 / a
    if kind == DCS:
        s = 2.0 * delta / (delta + e2)
        return np.where(s >= 1.0, e2, s * s * e2), np.where(s >= 1.0, 1.0, s * s)
    raise ValueError("unknown kernel %r" % (kind,))


def rho_edges(kinds, deltas, e2):
    """Per edge: kinds[e], deltas[e] applied to e2[e] -> (rho0, rho1)."""
    kinds = np.asarray(kinds)
    deltas = np.broadcast_to(np.asarray(deltas, np.float64), kinds.shape)
    r0, r1 = np.array(e2, np.float64), np.ones(len(kinds))
    for e in range(len(kinds)):
        a, b = rho(int(kinds[e]), float(deltas[e]), np.asarray(e2[e:e + 1]))
        r0[e], r1[e] = a[0], b[0]
    return r0, r1


def edge_e2(g, poses=None, source="np"):
    """e^T Omega e per edge: "np" from posegraph_oracle.edge_error, "c" from posegraph_oracle.c (pgo_chi2 of one edge)."""
    p = g["init"] if poses is None else poses
    if source == "np":
        e = po.edge_error(p, g["ij"], g["meas"])
        return np.einsum("ei,eij,ej->e", e, g["info"], e)
    import ctypes as C
    pp, ij, meas, info = pc._args(p, g["ij"], g["meas"], g["info"])
    L = pc.lib()
    out = np.zeros(len(ij))
    for e in range(len(ij)):
        out[e] = L.pgo_chi2(1, pc._d(pp), ij[e:e + 1].ctypes.data_as(C.POINTER(C.c_int32)), pc._d(meas[e:e + 1]), pc._d(info[e:e + 1]))
    return out


def weighted_system(g, kinds, deltas, poses=None, oracle="c", order=None):
    """The block system (layout of posegraph_se3.c_system) of the graph under per-edge kernels, through the C oracle
    (`oracle="c"`, edges taken in `order`, e2 from the C oracle) or the numpy oracle ("np", e2 from edge_error);
    chi2 = sum rho0 (in `order`).  Also returns the per-edge e2, rho0, weight in the graph's edge order."""
    e2 = edge_e2(g, poses, "c" if oracle == "c" else "np")
    r0, r1 = rho_edges(kinds, deltas, e2)
    gw = dict(g, info=g["info"] * r1[:, None, None])
    s = se3.c_system(gw, poses, order) if oracle == "c" else se3.np_system(gw, poses)
    o = np.arange(len(e2)) if order is None else order
    s["chi2"] = float(np.sum(r0[o]))
    s.update(e2=e2, rho=r0, weight=r1)
    return s


def kernel_mix(g, poses=None):
    """Edge e gets kind e % 4; delta from the reference's e2 at `poses`: Huber and Cauchy sqrt(median e2), DCS median e2 --
    so every kernel's threshold sits in the middle of the errors it meets."""
    e2 = edge_e2(g, poses)
    kinds = np.arange(len(e2), dtype=np.int32) % 4
    med = float(np.median(e2))
    deltas = np.where(kinds == DCS, med, np.sqrt(med))
    return kinds, deltas


def sides(kinds, deltas, e2):
    """per robust kind: (edges on the quadratic side, edges beyond the threshold).  Cauchy has no threshold: e2 against delta^2."""
    out = {}
    for k in (HUBER, CAUCHY, DCS):
        m = np.asarray(kinds) == k
        thr = deltas[m] if k == DCS else deltas[m] ** 2
        out[k] = (int((e2[m] <= thr).sum()), int((e2[m] > thr).sum()))
    return out


# ---- LM under kernels -----------------------------------------------------------------------------------------------------------------
def robust_chi2(poses, ij, meas, info, kinds, deltas):
    e = po.edge_error(poses, ij, meas)
    return float(np.sum(rho_edges(kinds, deltas, np.einsum("ei,eij,ej->e", e, info, e))[0]))


def optimize_robust(poses, ij, meas, info, kinds, deltas, fixed=0, max_iters=50):
    """posegraph_oracle.optimize's schedule (g2o's OptimizationAlgorithmLevenberg) with the weights: the system of each
    iteration is po.linearize on rho1 Omega, `cur` / `tmp` are sums of rho0 (g2o's activeRobustChi2), the gain denominator
    and the lambda schedule are unchanged.  -> (poses, history, final weights)"""
    poses = poses.copy()
    hist = []
    lam = None
    ni = 2.0
    for it in range(max_iters):
        e = po.edge_error(poses, ij, meas)
        r0, r1 = rho_edges(kinds, deltas, np.einsum("ei,eij,ej->e", e, info, e))
        H, b, _ = po.linearize(poses, ij, meas, info * r1[:, None, None])
        cur = float(np.sum(r0))
        if lam is None:
            d = H.diagonal().copy()
            d[fixed * 6: fixed * 6 + 6] = 0.0
            lam = 1e-5 * d.max()
        rho_gain, qmax = 0.0, 0
        while True:
            dx = po.solve_damped(H, b, lam, fixed)
            trial = po.oplus(poses, dx, fixed)
            tmp = robust_chi2(trial, ij, meas, info, kinds, deltas)
            scale = float(dx @ (lam * dx + b)) + 1e-3
            rho_gain = (cur - tmp) / scale
            if rho_gain > 0 and np.isfinite(tmp):
                alpha = min(1.0 - (2 * rho_gain - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                poses = trial
                cur = tmp
            else:
                lam *= ni
                ni *= 2.0
            qmax += 1
            if not (rho_gain < 0 and qmax < 10):
                break
        hist.append(dict(iter=it, chi2=cur, lam=lam, trials=qmax))
        if qmax == 10 or rho_gain == 0:
            break
    e = po.edge_error(poses, ij, meas)
    return poses, hist, rho_edges(kinds, deltas, np.einsum("ei,eij,ej->e", e, info, e))[1]


# ---- the two outlier scenarios ---------------------------------------------------------------------------------------------------------
SCENARIOS = {"kf120": dict(n_kf=120, n_loop=40, seed=3, nbad=4), "kf60": dict(n_kf=60, n_loop=20, seed=7, nbad=3)}
SCENARIO_KERNELS = {"dcs": (DCS, 1.0), "cauchy": (CAUCHY, 0.1)}
SCENARIO_ITERS = 100
# optimize_robust's own spread per (scenario, kernel): (max |position difference| in m, relative difference of the final sum
# rho0) over the permuted and the stopped-early runs (module docstring); measured by test_scenario_spread_is_as_recorded
SCENARIO_SPREAD = {
    ("kf120", "dcs"): (6e-7, 6e-10),
    ("kf120", "cauchy"): (8e-7, 3e-15),
    ("kf60", "dcs"): (2.5e-6, 9e-8),
    ("kf60", "cauchy"): (4e-7, 3e-15),
}


def outlier_scenario(name):
    """make_graph(laps=2, radius=15) of the scenario, `nbad` of its loop measurements corrupted: translation offsets uniform
    2 - 6 m with a random sign per axis, quaternion-vector noise of sigma 0.2.  -> (clean graph, corrupted graph, corrupted
    edge ids, loop edge ids); `fixed` is vertex 0."""
    sc = SCENARIOS[name]
    g = po.make_graph(n_kf=sc["n_kf"], n_loop=sc["n_loop"], laps=2, radius=15.0, seed=sc["seed"])
    g["fixed"] = 0
    loops = np.arange(g["n_odo"], len(g["ij"]))
    rng = np.random.default_rng(100 + sc["seed"])
    bad = rng.choice(loops, sc["nbad"], replace=False)
    off = rng.uniform(2.0, 6.0, (len(bad), 3)) * rng.choice([-1.0, 1.0], (len(bad), 3))
    dq = rng.normal(0.0, 0.2, (len(bad), 3))
    meas = g["meas"].copy()
    m = po.pose_mul(meas[bad], po.from_vector_mqt(np.concatenate([off, dq], 1)))
    m[:, 3:] /= np.linalg.norm(m[:, 3:], axis=1, keepdims=True)
    meas[bad] = m
    return g, dict(g, meas=meas), np.sort(bad), loops


def scenario_kernels(g, loops, kernel):
    """the kernel on every loop edge, none on the odometry edges"""
    kind, delta = SCENARIO_KERNELS[kernel]
    kinds = np.zeros(len(g["ij"]), np.int32)
    kinds[loops] = kind
    return kinds, np.full(len(kinds), delta)


def position_error(poses, g):
    return float(np.linalg.norm(poses[:, :3] - g["gt"][:, :3], axis=1).max())


_cache = {}
# the numpy LM's max position error against ground truth on the CLEAN graph (m), asserted by the CPU suite to 1e-3; the GPU
# tests take it from here instead of running the clean graph through the numpy LM again
SCENARIO_CLEAN_ERR = {"kf120": 0.735, "kf60": 0.349}


def scenario_baselines(name):
    """Computed once per process: the plain numpy LM on the clean and on the corrupted graph -> (clean error, plain error)."""
    if ("base", name) not in _cache:
        g, gc, bad, loops = outlier_scenario(name)
        a = lambda q: (q["init"], q["ij"], q["meas"], q["info"])  # noqa: E731
        clean, _ = po.optimize(*a(g), fixed=0, max_iters=SCENARIO_ITERS)
        plain, _ = po.optimize(*a(gc), fixed=0, max_iters=SCENARIO_ITERS)
        _cache[("base", name)] = (position_error(clean, g), position_error(plain, g))
    return _cache[("base", name)]


def scenario_reference(name, kernel):
    """Computed once per process: optimize_robust on the corrupted graph with the kernel on its loop edges -> dict(g, gc,
    bad, loops, kinds, deltas, poses, hist, weights, robust_err)."""
    key = (name, kernel)
    if key not in _cache:
        g, gc, bad, loops = outlier_scenario(name)
        kinds, deltas = scenario_kernels(gc, loops, kernel)
        P, hist, w = optimize_robust(gc["init"], gc["ij"], gc["meas"], gc["info"], kinds, deltas, fixed=0, max_iters=SCENARIO_ITERS)
        _cache[key] = dict(g=g, gc=gc, bad=bad, loops=loops, kinds=kinds, deltas=deltas, poses=P, hist=hist, weights=w,
                           robust_err=position_error(P, g))
    return _cache[key]


def scenario_spread(name, kernel):
    """-> (position spread in m, relative spread of the final sum rho0, every run took the reference run's trials)"""
    r = scenario_reference(name, kernel)
    gc, kinds, deltas = r["gc"], r["kinds"], r["deltas"]
    ref_trials = [h["trials"] for h in r["hist"]]
    dpos, dchi, same = 0.0, 0.0, True

    def account(P, hist):
        nonlocal dpos, dchi, same
        dpos = max(dpos, float(np.abs(P[:, :3] - r["poses"][:, :3]).max()))
        dchi = max(dchi, abs(hist[-1]["chi2"] - r["hist"][-1]["chi2"]) / r["hist"][-1]["chi2"])
        same = same and [h["trials"] for h in hist] == ref_trials

    for rep in range(3):
        o = np.random.default_rng(rep).permutation(len(kinds))
        P, hist, _ = optimize_robust(gc["init"], gc["ij"][o], gc["meas"][o], gc["info"][o], kinds[o], deltas[o], fixed=0,
                                     max_iters=SCENARIO_ITERS)
        account(P, hist)
    exact = po.solve_damped
    try:
        for rep in range(3):
            rng = np.random.default_rng(rep)

            def stopped_early(H, b, lam, fx):
                rr = rng.normal(size=len(b))
                rr[6 * fx:6 * fx + 6] = 0.0
                return exact(H, b + rr * (se3.PCG_TOL * np.linalg.norm(b) / np.linalg.norm(rr)), lam, fx)
            po.solve_damped = stopped_early
            P, hist, _ = optimize_robust(gc["init"], gc["ij"], gc["meas"], gc["info"], kinds, deltas, fixed=0, max_iters=SCENARIO_ITERS)
            account(P, hist)
    finally:
        po.solve_damped = exact
    return dpos, dchi, same
