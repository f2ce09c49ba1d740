"""Reference for unary constraints on pose-graph vertices -- GPS position (XYZ) and absolute-pose (POSE) priors -- (test
infrastructure only; CPU, numpy fp64), shared by tests/test_posegraph_prior_ref.py (CPU) and
tests/test_gpu_posegraph_priors.py (GPU).

PARITY UNPINNED, like the rest of the pose-graph solver: neither g2o nor hdl_graph_slam is available here.  The semantics
restated are their published ones (g2o EdgeSE3Prior with a zero offset, hdl_graph_slam EdgeSE3PriorXYZ) in the conventions
of oracle/posegraph_oracle.py (update X <- X * fromVectorMQT(d), error in toVectorMQT coordinates).  On vertex v with
estimate X = (t, q):
  XYZ   e = t - z (3 rows), J = [R(q) | 0], Omega = the upper-left 3x3 of the 6x6 information (the rest is ignored)
  POSE  e = toVectorMQT(Z^-1 X) (6 rows): the binary edge u -> v with measurement Z from an extra vertex u at the identity
A prior adds rho1 J^T Omega J to its vertex's diagonal block, -rho1 J^T Omega e to its segment of b and rho0 to chi2
(robust_posegraph_ref.rho; no kernel: rho = (e2, 1)); on the fixed vertex it adds only rho0 to chi2.

Two systems in the layout of posegraph_se3.c_system / np_system:
  prior_system(..., oracle="np")  edges and POSE priors through posegraph_oracle.py (central differences), XYZ analytic
  prior_system(..., oracle="c")   edges and POSE priors through posegraph_oracle.c as the AUGMENTED graph (one extra vertex
                                  fixed at the identity, one binary edge per POSE prior behind the graph's edges), restricted
                                  to the original vertices; XYZ analytic in numpy on top
The two anchors (asserted by the CPU suite): the augmented C system against the numpy system for POSE priors, and the
analytic XYZ Jacobian against central differences under the file's update rule.

MEASURED FLOORS (tests/test_posegraph_prior_ref.py asserts that the references stay inside the recorded figures; the GPU
tests use ten times them; nothing here was calibrated against the GPU).  Graphs: LIN_PRIOR_CASES below.
  (a) POSE priors, augmented C system against the numpy system (the POSE-only cases): H 1.5e-10 max|H|, b 6.5e-11 max|b|,
      chi2 5.2e-15 chi2; every case, prior_system "c" against "np": 1.5e-10 / 1.0e-10 / 5.3e-15 -- inside the existing
      C-against-numpy floors posegraph_se3.O2O_* (2e-10 / 3.5e-10 / 1e-14), which are therefore reused unchanged
  (b) XYZ: analytic J = [R | 0] against central differences (h = 1e-6) 1.1e-9 of the largest Jacobian entry (1), and the
      central differences at h against h / 2 2.6e-9.  Above posegraph_se3.FD_REL (5e-10): that was measured on an edge's
      RELATIVE translation; here the differenced quantity is the absolute position, up to 10 m, and the rounding
      eps |t| / h = 2e-9 of the differences dominates.  Recorded as XYZ_FD_REL = 3e-9 (the analytic side has no such term)
  (c) summation order: the priors permuted (eight permutations per case, with and without kernels), oracle="c": diag
      3.2e-19 max|diag|, b 1.6e-18 max|b|, chi2 0 -- a vertex has at most three priors and far more edge terms; inside
      posegraph_se3.SPREAD_* (4.5e-16 / 4.5e-16 / 3.5e-15), reused unchanged
  (d) per prior, the C oracle's e2 (pgo_chi2 of the augmented edge) against numpy's: 2.1e-15 e2, and the weights computed
      from each: 4.0e-15 -- inside robust_posegraph_ref.W_EDGE_* (2e-14 / 2e-14 / 5e-15), reused unchanged
  (e) the weighted system (prior_kernel_mix on every case): prior_system "c" with the weights from the C oracle's e2 against
      the same with the weights from numpy's e2 -- what the spread of a weight does to the system: diag 3.4e-18 max|diag|,
      b 1.2e-17 max|b|, chi2 0; with the priors permuted as in (c) 3.2e-19 / 7.8e-19 / 0 -- inside posegraph_se3.SPREAD_*,
      so the weighted system is held to the same floors as the plain one
  (f) the graph node's scenario (graph_gps_scenario, 30 keyframes): every fix shifted by 1e6 m moves what reaches the solver
      by 4.7e-10 m, the aligned estimates by 7.0e-10, the reference LM's poses (7-vectors) after its 50 iterations by 3.0e-9
      and tf_odom2graph = last estimate x last odometry^-1 made from them by 6.3e-8 (the orientation's share over the 15 m
      lever of the odometry position) -- the rounding of fix - origin at 5e6 m, ulp 9.3e-10, and nothing else:
      GRAPH_GPS_SHIFT_*.  The reference LM itself crawls
      at the end: after 50 iterations its poses are 4.8e-5 m from where it stops (81 iterations), chi2 7.2e-10 of itself
      above: GRAPH_GPS_CONVERGENCE_*
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import posegraph_se3 as se3
import robust_posegraph_ref as rr

po, pc = se3.po, se3.pc

XYZ, POSE = 0, 1
XYZ_FD_REL = 3e-9  # (b): central differences of e = t - z against the analytic Jacobian, and against themselves at h / 2
IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


# ---- prior sets ---------------------------------------------------------------------------------------------------------------
def empty_priors():
    return dict(vertex=np.zeros(0, np.int32), type=np.zeros(0, np.int32), meas=np.zeros((0, 7)), info=np.zeros((0, 6, 6)),
                kernels=np.zeros(0, np.int32), deltas=np.ones(0))


def make_priors(g, vertices, types, seed, sigma=(0.5, 0.1), rank_deficient=()):
    """One prior per entry of `vertices` / `types` (a vertex may repeat) on graph `g`: the measurement is the ground truth
    perturbed by `sigma` (translation, quaternion vector), with a random sign on the quaternion (both hemispheres of q_e);
    dense, exactly symmetric SPD information A A^T + c I.  XYZ priors carry it in the upper-left 3x3 and finite,
    asymmetric junk everywhere else, which must be ignored; `rank_deficient`: indices of POSE priors whose translation rows
    and columns are zero (an orientation prior, positive semi-definite)."""
    rng = np.random.default_rng(1000 + seed)
    vertices = np.asarray(vertices, np.int32)
    types = np.asarray(types, np.int32)
    n = len(vertices)
    d = np.concatenate([rng.normal(0, sigma[0], (n, 3)), rng.normal(0, sigma[1], (n, 3))], 1)
    meas = po.pose_mul(g["gt"][vertices], po.from_vector_mqt(d))
    meas[:, 3:] /= np.linalg.norm(meas[:, 3:], axis=1, keepdims=True)
    meas[:, 3:] *= rng.choice([-1.0, 1.0], (n, 1))
    A = rng.normal(size=(n, 6, 6))
    info = A @ np.transpose(A, (0, 2, 1)) + rng.uniform(0.5, 2.0, (n, 1, 1)) * np.eye(6)
    info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    for p in range(n):
        if types[p] == XYZ:
            junk = rng.normal(size=(6, 6)) * 100.0
            junk[:3, :3] = info[p, :3, :3]
            info[p] = junk
    for p in rank_deficient:
        assert types[p] == POSE
        info[p, :3, :] = 0.0
        info[p, :, :3] = 0.0
    return dict(vertex=vertices, type=types, meas=meas, info=info, kernels=np.zeros(n, np.int32), deltas=np.ones(n))


def permuted(pr, order):
    return {k: np.asarray(v)[order] for k, v in pr.items()}


def used_info(pr):
    """the information the prior uses: an XYZ prior's outside its 3x3 zeroed"""
    info = np.array(pr["info"], np.float64)
    x = np.asarray(pr["type"]) == XYZ
    info[x, 3:, :] = 0.0
    info[x, :, 3:] = 0.0
    return info


# ---- errors, Jacobians, per-prior values -----------------------------------------------------------------------------------
def _augmented_edges(n, pr, sel):
    """POSE priors `sel` as binary edges from the extra vertex n"""
    v = np.asarray(pr["vertex"])[sel]
    return np.stack([np.full(len(v), n, np.int32), v.astype(np.int32)], 1).astype(np.int32), pr["meas"][sel]


def prior_error(poses, pr):
    """(n_p, 6); rows 3..5 of an XYZ prior are zero"""
    n = len(poses)
    t = np.asarray(pr["type"])
    e = np.zeros((len(t), 6))
    x = np.nonzero(t == XYZ)[0]
    e[x, :3] = poses[pr["vertex"][x], :3] - pr["meas"][x, :3]
    s = np.nonzero(t == POSE)[0]
    if len(s):
        ij, meas = _augmented_edges(n, pr, s)
        e[s] = po.edge_error(np.vstack([poses, IDENT]), ij, meas)
    return e


def quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def xyz_jacobian(pose):
    """analytic: d (t + R dt - z) / d [dt, dq] = [R | 0], padded to 6 x 6"""
    J = np.zeros((6, 6))
    J[:3, :3] = quat_matrix(pose[3:])
    return J


def xyz_jacobian_numeric(pose, h=1e-6):
    """central differences of e = t - z under X <- X * fromVectorMQT(d)"""
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros((1, 6))
        d[0, k] = h
        J[:3, k] = (po.pose_mul(pose[None], po.from_vector_mqt(d))[0, :3] - po.pose_mul(pose[None], po.from_vector_mqt(-d))[0, :3]) / (2 * h)
    return J


def prior_jacobians(poses, pr):
    """(n_p, 6, 6): XYZ analytic, POSE the numpy oracle's central differences of the augmented edge (vertex j)"""
    t = np.asarray(pr["type"])
    J = np.zeros((len(t), 6, 6))
    for p in np.nonzero(t == XYZ)[0]:
        J[p] = xyz_jacobian(poses[pr["vertex"][p]])
    s = np.nonzero(t == POSE)[0]
    if len(s):
        ij, meas = _augmented_edges(len(poses), pr, s)
        J[s] = po.numeric_jacobians(np.vstack([poses, IDENT]), ij, meas)[1]
    return J


def prior_e2(poses, pr, source="np"):
    """e^T Omega e per prior; "c": a POSE prior's from posegraph_oracle.c (pgo_chi2 of its augmented edge), XYZ as numpy"""
    e = prior_error(poses, pr)
    out = np.einsum("pi,pij,pj->p", e, used_info(pr), e)
    if source == "c":
        import ctypes as C
        L = pc.lib()
        for p in np.nonzero(np.asarray(pr["type"]) == POSE)[0]:
            pp, ij, meas, info = pc._args(np.vstack([IDENT, poses[pr["vertex"][p]]]), np.array([[0, 1]]), pr["meas"][p:p + 1], pr["info"][p:p + 1])
            out[p] = L.pgo_chi2(1, pc._d(pp), ij.ctypes.data_as(C.POINTER(C.c_int32)), pc._d(meas), pc._d(info))
    return out


def prior_rho(poses, pr, source="np"):
    """-> (e2, rho0, rho1) per prior under its kernel"""
    e2 = prior_e2(poses, pr, source)
    r0, r1 = rr.rho_edges(pr["kernels"], pr["deltas"], e2) if len(e2) else (e2.copy(), np.ones(0))
    return e2, r0, r1


def raw_prior_quaternion_w(poses, pr):
    """w of qz* (x) q_v before normalisation and sign choice, per POSE prior: negative = the sgn = -1 branch"""
    s = np.nonzero(np.asarray(pr["type"]) == POSE)[0]
    return po.pose_mul(po.pose_inv(pr["meas"][s]), poses[pr["vertex"][s]])[:, 6]


# ---- the block system -------------------------------------------------------------------------------------------------------
def _fix(sysd, fixed):
    if fixed is None or fixed < 0:
        return
    sysd["diag"][fixed] = np.eye(6)
    sysd["b"][6 * fixed:6 * fixed + 6] = 0.0
    if len(sysd["off_ij"]):
        sysd["off"][(sysd["off_ij"] == fixed).any(1)] = 0.0


def _np_edges(g, poses, edge_weights):
    """the numpy oracle's system of the edges alone, NO vertex fixed"""
    n = len(poses)
    pr = se3.pairs_of(g["ij"])
    if len(g["ij"]) == 0:
        return dict(diag=np.zeros((n, 6, 6)), off=np.zeros((0, 6, 6)), off_ij=pr, b=np.zeros(6 * n), chi2=0.0)
    info = g["info"] if edge_weights is None else g["info"] * edge_weights[:, None, None]
    H, b, c2 = po.linearize(poses, g["ij"], g["meas"], info)
    Hd = H.toarray()
    diag = np.stack([Hd[6 * v:6 * v + 6, 6 * v:6 * v + 6] for v in range(n)])
    off = np.stack([Hd[6 * a:6 * a + 6, 6 * c:6 * c + 6] for a, c in pr]) if len(pr) else np.zeros((0, 6, 6))
    return dict(diag=diag, off=off, off_ij=pr, b=b.copy(), chi2=c2)


def augmented_graph(g, pr, poses=None, weights=None):
    """The graph with one extra vertex n at the identity and one binary edge n -> v per POSE prior, behind the graph's
    edges (info scaled by `weights`, one per POSE prior, when given) -> (poses, ij, meas, info)"""
    p = g["init"] if poses is None else poses
    s = np.nonzero(np.asarray(pr["type"]) == POSE)[0]
    ij, meas = _augmented_edges(len(p), pr, s)
    info = pr["info"][s] if weights is None else pr["info"][s] * weights[:, None, None]
    ne = len(g["ij"])
    return (np.vstack([p, IDENT]), np.concatenate([np.asarray(g["ij"], np.int32).reshape(ne, 2), ij]).astype(np.int32),
            np.concatenate([np.asarray(g["meas"]).reshape(ne, 7), meas]), np.concatenate([np.asarray(g["info"]).reshape(ne, 6, 6), info]))


def prior_system(g, pr, poses=None, oracle="np", fixed=None, e2_source=None):
    """Block system (layout of posegraph_se3.c_system: diag, off in sorted-pair order, off_ij, b, chi2) of the graph's plain
    edges plus the priors under their kernels, at `poses` (default g["init"]); `fixed` (default g["fixed"]; -1: none) gets
    the identity block and a zero right-hand side.  chi2 = the edges' chi2 + sum of the priors' rho0.  Also returns the
    per-prior e2 / rho / weight."""
    p = g["init"] if poses is None else poses
    fixed = g["fixed"] if fixed is None else fixed
    n = len(p)
    e2, r0, r1 = prior_rho(p, pr, e2_source or ("c" if oracle == "c" else "np"))  # (e2_source: the weights' e2 from the OTHER oracle)
    t = np.asarray(pr["type"])
    xs, ps = np.nonzero(t == XYZ)[0], np.nonzero(t == POSE)[0]
    pairs = se3.pairs_of(g["ij"])
    if oracle == "c":
        P, ij, meas, info = augmented_graph(g, pr, p, r1[ps])
        if len(ij):
            diag, b, _ = pc.linearize(P, ij, meas, info, fixed=n)
            off = pc.offdiag_blocks(P, ij, meas, info, pairs, fixed=n) if len(pairs) else np.zeros((0, 6, 6))
            s = dict(diag=diag[:n].copy(), off=off, off_ij=pairs, b=b[:6 * n].copy())
            ne = len(g["ij"])
            s["chi2"] = pc.linearize(P[:n], ij[:ne], meas[:ne], info[:ne], fixed=0)[2] if ne else 0.0
        else:
            s = dict(diag=np.zeros((n, 6, 6)), off=np.zeros((0, 6, 6)), off_ij=pairs, b=np.zeros(6 * n), chi2=0.0)
        add = xs  # POSE priors are already in
    else:
        s = _np_edges(g, p, None)
        add = np.arange(len(t))
    if len(add):
        e, J, W = prior_error(p, pr), prior_jacobians(p, pr), used_info(pr)
        for q in add:  # prior order
            v = pr["vertex"][q]
            A = J[q].T @ W[q]
            s["diag"][v] += r1[q] * (A @ J[q])
            s["b"][6 * v:6 * v + 6] -= r1[q] * (A @ e[q])
    s["chi2"] = float(s["chi2"] + np.sum(r0))
    _fix(s, fixed)
    s.update(e2=e2, rho=r0, weight=r1)
    return s


def _max_h(s):
    return max(np.abs(s["diag"]).max(), np.abs(s["off"]).max() if s["off"].size else 0.0)


def differences(a, b):
    """largest differences of two systems relative to b's own scale: diag, off, h (both / max|H|), b, chi2"""
    assert np.array_equal(a["off_ij"], b["off_ij"])
    dd = np.abs(a["diag"] - b["diag"]).max()
    do = np.abs(a["off"] - b["off"]).max() if b["off"].size else 0.0
    return dict(diag=dd / np.abs(b["diag"]).max(), off=do / max(np.abs(b["off"]).max() if b["off"].size else 0.0, 1e-300),
                h=max(dd, do) / _max_h(b), b=np.abs(a["b"] - b["b"]).max() / np.abs(b["b"]).max(), chi2=abs(a["chi2"] - b["chi2"]) / b["chi2"])


def to_sparse(s):
    """H of a block system as scipy CSR"""
    n = len(s["diag"])
    H = sp.lil_matrix((6 * n, 6 * n))
    for v in range(n):
        H[6 * v:6 * v + 6, 6 * v:6 * v + 6] = s["diag"][v]
    for (a, c), blk in zip(s["off_ij"], s["off"]):
        H[6 * a:6 * a + 6, 6 * c:6 * c + 6] = blk
        H[6 * c:6 * c + 6, 6 * a:6 * a + 6] = blk.T
    return H.tocsr()


# ---- LM with priors -----------------------------------------------------------------------------------------------------------
def total_chi2(poses, g, pr):
    c = po.chi2(poses, g["ij"], g["meas"], g["info"]) if len(g["ij"]) else 0.0
    return float(c + np.sum(prior_rho(poses, pr)[1]))


def solve_damped(H, b, lam, fixed):
    """(H + lam I) dx = b over the free vertices; fixed = -1: every vertex is free"""
    n6 = H.shape[0]
    idx = np.arange(n6) if fixed < 0 else np.r_[0:6 * fixed, 6 * fixed + 6:n6]
    A = (H + lam * sp.identity(n6, format="csr"))[idx][:, idx].tocsc()
    dx = np.zeros(n6)
    dx[idx] = spla.spsolve(A, b[idx])
    return dx


def oplus(poses, dx, fixed):
    d = dx.reshape(-1, 6).copy()
    if fixed >= 0:
        d[fixed] = 0.0
    out = po.pose_mul(poses, po.from_vector_mqt(d))
    out[:, 3:] /= np.linalg.norm(out[:, 3:], axis=1, keepdims=True)
    if fixed >= 0:
        out[fixed] = poses[fixed]
    return out


def optimize(g, pr, fixed=None, max_iters=50, solve=None, on_trial=None):
    """posegraph_oracle.optimize's schedule (g2o's OptimizationAlgorithmLevenberg) on edges + priors: the system of each
    iteration is prior_system(oracle="np"), `cur` / `tmp` are the edges' chi2 plus the priors' sum of rho0, the gain
    denominator and the lambda schedule are unchanged; `fixed` = -1 holds no vertex.  -> (poses, history)"""
    fixed = g["fixed"] if fixed is None else fixed
    solve = solve or solve_damped
    poses = g["init"].copy()
    hist, lam, ni = [], None, 2.0
    for it in range(max_iters):
        s = prior_system(g, pr, poses, "np", fixed=-1)
        H, b, cur = to_sparse(s), s["b"], s["chi2"]
        if lam is None:
            d = H.diagonal().copy()
            if fixed >= 0:
                d[6 * fixed:6 * fixed + 6] = 0.0
            lam = 1e-5 * d.max()
        gain, qmax = 0.0, 0
        while True:
            dx = solve(H, b, lam, fixed)
            trial = oplus(poses, dx, fixed)
            tmp = total_chi2(trial, g, pr)
            gain = (cur - tmp) / (float(dx @ (lam * dx + b)) + 1e-3)
            accepted = gain > 0 and np.isfinite(tmp)
            if on_trial is not None:
                on_trial(H, b, lam, dx, accepted)
            if accepted:
                lam *= max(1.0 / 3.0, min(1.0 - (2 * gain - 1) ** 3, 2.0 / 3.0))
                ni = 2.0
                poses, cur = trial, tmp
            else:
                lam *= ni
                ni *= 2.0
            qmax += 1
            if not (gain < 0 and qmax < 10):
                break
        hist.append(dict(iter=it, chi2=cur, lam=lam, trials=qmax))
        if qmax == 10 or gain == 0:
            break
    return poses, hist


def lm_run(g, pr, fixed, iters):
    """The numpy LM over `iters` iterations with what a GPU comparison needs: poses, per-iteration trials and chi2, the
    path length (sum of max|dx| over the accepted steps), and the spread of poses / final chi2 / trial sequence under
    damped solves that stop at the PCG's residual (A^-1 (b + r), |r| = PCG_TOL |b|, three random r)."""
    path = []
    P, hist = optimize(g, pr, fixed, iters, on_trial=lambda H, b, lam, dx, acc: path.append(np.abs(dx).max() if acc else 0.0))
    spread, chi_spread, same = 0.0, 0.0, True
    for rep in range(3):
        rng = np.random.default_rng(rep)

        def stopped_early(H, b, lam, fx):
            r = rng.normal(size=len(b))
            if fx >= 0:
                r[6 * fx:6 * fx + 6] = 0.0
            return solve_damped(H, b + r * (se3.PCG_TOL * np.linalg.norm(b) / np.linalg.norm(r)), lam, fx)
        P2, h2 = optimize(g, pr, fixed, iters, solve=stopped_early)
        same = same and [h["trials"] for h in h2] == [h["trials"] for h in hist]
        spread = max(spread, float(np.abs(P2 - P).max()))
        chi_spread = max(chi_spread, abs(h2[-1]["chi2"] - hist[-1]["chi2"]) / hist[-1]["chi2"])
    return dict(poses=P, trials=[h["trials"] for h in hist], chi2=[total_chi2(g["init"], g, pr)] + [h["chi2"] for h in hist],
                path=float(sum(path)), pcg_spread=spread, pcg_chi2_spread=chi_spread, pcg_same_trials=same)


def c_lm_augmented(g, pr, iters):
    """posegraph_oracle.c's LM on the augmented graph (POSE priors only, no kernels; the extra vertex fixed) -> (poses of the
    original vertices, per-iteration trial counts, PgoStats of the full run)"""
    assert (np.asarray(pr["type"]) == POSE).all() and not np.asarray(pr["kernels"]).any()
    a = augmented_graph(g, pr)
    n = len(g["init"])
    cum = []
    for k in range(1, iters + 1):
        out, st = pc.optimize(*a, fixed=n, max_iters=k)
        cum.append(st.trials)
    return out[:n], list(np.diff([0] + cum)), st


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def lin_case(name):
    """-> (graph, priors, fixed): the linearisation cases.  Sizes 1 (no edge, one prior), 2, 7, 65, 400; XYZ only, POSE only,
    mixed, two and three priors on one vertex, a prior on the fixed vertex, fixed = -1, rank-deficient POSE information, both
    hemispheres of q_e, and 300 priors (three blocks of pg_prior_kernel, the last one partly filled)."""
    if name == "n1_xyz":
        g = dict(gt=IDENT[None].copy(), init=np.array([[0.3, -0.2, 0.1, 0.1, 0.2, -0.1, 0.9]]), ij=np.zeros((0, 2), np.int32),
                 meas=np.zeros((0, 7)), info=np.zeros((0, 6, 6)), fixed=-1, isolated=None)
        g["init"][:, 3:] /= np.linalg.norm(g["init"][:, 3:])
        return g, make_priors(g, [0], [XYZ], 0), -1
    if name == "n2_pose":
        g = se3.graph((2, 1, 0, 0, False))
        return g, make_priors(g, [1], [POSE], 1), 0
    if name == "n2_free_mixed":
        g = se3.graph((2, 1, 0, 0, False))
        return g, make_priors(g, [0, 1, 1], [POSE, XYZ, POSE], 2), -1
    if name == "n7_xyz":
        g = se3.graph((7, 6, 3, 3, True))
        return g, make_priors(g, [0, 1, 2, 4, 5, 6, 6], [XYZ] * 7, 3), 3  # two on the isolated vertex 6
    if name == "n7_pose_fixed":
        g = se3.graph((7, 6, 2, 3, False))
        return g, make_priors(g, [3, 0, 0, 0, 5], [POSE] * 5, 4, rank_deficient=(2,)), 3  # one on the fixed vertex, three on vertex 0
    if name == "n65_mixed":
        g = se3.graph((65, 100, 5, 32, True))
        v = [0, 7, 7, 7, 32, 32, 40, 63, 64, 64, 12, 13]
        t = [XYZ, POSE, XYZ, POSE, XYZ, POSE, POSE, POSE, XYZ, POSE, POSE, XYZ]
        return g, make_priors(g, v, t, 5, rank_deficient=(6, 10)), 32
    if name == "n65_free_pose":
        g = se3.graph((65, 100, 5, 32, True))
        v = list(range(0, 65, 4)) + [8, 8]
        return g, make_priors(g, v, [POSE] * len(v), 6, rank_deficient=(3,)), -1
    if name == "n400_many":
        g = se3.graph((400, 600, 6, 200, False))
        v = list(range(300))
        v[100], v[101] = 17, 17  # three priors on vertex 17, far apart in prior order
        return g, make_priors(g, v, [XYZ if k % 3 else POSE for k in range(300)], 7), -1
    raise KeyError(name)


LIN_PRIOR_CASES = ["n1_xyz", "n2_pose", "n2_free_mixed", "n7_xyz", "n7_pose_fixed", "n65_mixed", "n65_free_pose", "n400_many"]


def prior_kernel_mix(g, pr, poses=None):
    """Prior p gets kind p % 4; delta from the reference's e2: Huber and Cauchy sqrt(median e2), DCS median e2 -- so every
    kernel's threshold sits in the middle of the errors it meets.  -> a copy of `pr` with kernels and deltas"""
    p = g["init"] if poses is None else poses
    e2 = prior_e2(p, pr)
    kinds = np.arange(len(e2), dtype=np.int32) % 4
    med = float(np.median(e2[e2 > 0]))
    return dict(pr, kernels=kinds, deltas=np.where(kinds == rr.DCS, med, np.sqrt(med)))


# LM runs: the 40-vertex graphs of posegraph_se3.LM_CASES with NO vertex fixed and priors on three vertices.
LM_PRIOR_VERTICES = [3, 20, 36]
# (start, seed, iterations compared), chosen on the CPU like posegraph_se3.LM_CASES: the numpy LM and (POSE) the C oracle's LM
# on the augmented graph take the same trials in every compared iteration, the sequence survives solves that stop at the
# PCG's residual, and chi2 still falls by more than 1e-9 of itself in the last compared iteration.
LM_POSE_CASES = [("mild", 0, 6), ("mild", 1, 6), ("gross", 2, 8)]
LM_XYZ_CASES = [("mild", 0, 6), ("mild", 5, 6)]


def lm_case(start, seed, type_):
    g = se3.lm_graph(start, seed, 0)
    v = LM_PRIOR_VERTICES if type_ == POSE else LM_PRIOR_VERTICES + [11, 29]  # (three positions leave no gauge freedom; five condition it)
    pr = make_priors(g, v, [type_] * len(v), 50 + seed, sigma=(0.05, 0.02))
    pr["info"][:] = 4.0 * np.eye(6)
    return g, pr


# ---- the GPS outlier scenario -----------------------------------------------------------------------------------------------------
GPS_SIGMA = (0.3, 0.6)  # (xy, z) metres
GPS_OUTLIER = 7         # the displaced fix


def gps_scenario(kernel):
    """A 60-keyframe lap (make_graph) with its loop closures dropped -- odometry only, so the drift is unbounded -- and one GPS
    fix per third keyframe, noise GPS_SIGMA, information diag(1 / sxy^2, 1 / sxy^2, 1 / sz^2); fix GPS_OUTLIER is displaced by
    50 sigma_xy along x.  `kernel`: None or "cauchy" (delta 1) on every fix.  No vertex fixed.  -> (graph, priors)"""
    g = po.make_graph(n_kf=60, n_loop=0, laps=1, radius=15.0, seed=11)
    g["fixed"] = -1
    rng = np.random.default_rng(77)
    v = np.arange(0, 60, 3, dtype=np.int32)
    meas = np.tile(IDENT, (len(v), 1))
    meas[:, :3] = g["gt"][v, :3] + rng.normal(size=(len(v), 3)) * np.array([GPS_SIGMA[0], GPS_SIGMA[0], GPS_SIGMA[1]])
    meas[GPS_OUTLIER, 0] += 50 * GPS_SIGMA[0]
    info = np.zeros((len(v), 6, 6))
    info[:, :3, :3] = np.diag([1 / GPS_SIGMA[0] ** 2, 1 / GPS_SIGMA[0] ** 2, 1 / GPS_SIGMA[1] ** 2])
    kinds = np.full(len(v), rr.CAUCHY if kernel == "cauchy" else rr.NONE, np.int32)
    return g, dict(vertex=v, type=np.full(len(v), XYZ, np.int32), meas=meas, info=info, kernels=kinds, deltas=np.ones(len(v)))


GPS_ITERS = 30
_cache = {}


def gps_reference(kernel):
    """Computed once per process: the numpy LM on the scenario -> dict(g, pr, poses, hist, weights, err): err = the largest
    position error against ground truth over the keyframes (m)."""
    if kernel not in _cache:
        g, pr = gps_scenario(kernel)
        P, hist = optimize(g, pr, -1, GPS_ITERS)
        _cache[kernel] = dict(g=g, pr=pr, poses=P, hist=hist, weights=prior_rho(P, pr)[2],
                              err=float(np.linalg.norm(P[:, :3] - g["gt"][:, :3], axis=1).max()))
    return _cache[kernel]


# ---- the graph node with GPS fixes (tests/test_gpu_graph_gps.py; its CPU conditions in tests/test_posegraph_prior_ref.py) ---------
GRAPH_GPS_SIGMA = (0.1, 0.2)       # (xy, z) metres: the noise the fixes are made with and the sigma the Graph is told
GRAPH_GPS_UTM = (5.0e5, 4.0e6, 0.0)  # UTM offsets of the scene
GRAPH_GPS_YAW_BIAS = 0.02          # rad per step added to every odometry increment
GRAPH_GPS_LM_ITERS = 4             # compared LM prefix from the bookkeeping-only state (chosen on the CPU, see the CPU test)
GRAPH_GPS_ITERS = 50               # LM iterations a pass of the driven node may take
# floors (f) of the module docstring, each just above its measurement
GRAPH_GPS_SHIFT_MEAS = 5e-10       # a 1e6 m shift of every fix: the priors' measurements [m]
GRAPH_GPS_SHIFT_INIT = 8e-10       # ... the aligned estimates
GRAPH_GPS_SHIFT_POSES = 3.5e-9     # ... the reference LM's poses (7-vectors) after GRAPH_GPS_ITERS iterations
GRAPH_GPS_SHIFT_TF = 7e-8          # ... tf_odom2graph made from them
GRAPH_GPS_CONVERGENCE_POSES = 5e-5   # the reference LM after GRAPH_GPS_ITERS iterations against where it stops [m]
GRAPH_GPS_CONVERGENCE_CHI2 = 8e-10   # ... chi2, relative


def _yaw_pose(x, y, z, yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [x, y, z]
    return T


def graph_gps_scenario(utm_shift=0.0, n=30, corner=15):
    """`n` frames 1 m apart on an L-shaped path with no revisit (`corner` of them north, the rest east; 29 m of travel at
    n = 30, below the loop detector's 30 m), the start heading rotated 90 degrees from ENU; odometry = the true increments with a constant yaw bias,
    starting at the identity; one fix per frame: the true ENU position + GRAPH_GPS_SIGMA noise + the UTM offsets (+
    `utm_shift` on every coordinate).  -> dict(gt (n, 4, 4) in ENU without the offsets, odom (n, 4, 4), fixes (n, 3),
    clouds: a small (corner, surf) pair per frame)."""
    rng = np.random.default_rng(2024)
    gt = []
    for k in range(n):
        gt.append(_yaw_pose(0.0, float(k), 0.0, np.pi / 2) if k < corner else _yaw_pose(float(k - corner + 1), corner - 1.0, 0.0, 0.0))
    gt = np.array(gt)
    bias = _yaw_pose(0.0, 0.0, 0.0, GRAPH_GPS_YAW_BIAS)
    odom = [np.eye(4)]
    for k in range(n - 1):
        odom.append(odom[-1] @ np.linalg.inv(gt[k]) @ gt[k + 1] @ bias)
    sig = np.array([GRAPH_GPS_SIGMA[0], GRAPH_GPS_SIGMA[0], GRAPH_GPS_SIGMA[1]])
    fixes = gt[:, :3, 3] + rng.normal(size=(n, 3)) * sig + np.array(GRAPH_GPS_UTM) + utm_shift
    clouds = [(rng.uniform(-5, 5, (8, 4)).astype(np.float32), rng.uniform(-5, 5, (8, 4)).astype(np.float32)) for _ in range(n)]
    return dict(gt=gt, odom=np.array(odom), fixes=fixes, clouds=clouds)


def drive_graph(graph, sc, max_iterations, with_fixes=True):
    """Every frame through add_frame + optimize(max_iterations) -> per pass (priors in the solver, solver's fixed vertex)"""
    trace = []
    graph._bookkeeping_only = max_iterations == 0  # (0: keyframes, edges, alignment and priors only -- needs no device)
    for k in range(len(sc["odom"])):
        c, s = sc["clouds"][k]
        kf = graph.add_frame(sc["odom"][k], c, s, utm_coord=sc["fixes"][k]) if with_fixes else graph.add_frame(sc["odom"][k], c, s)
        assert kf is not None
        graph.optimize(max_iterations or 1000)
        trace.append((len(graph.solver._priors), graph.solver.fixed))
    return trace


def graph_arrays(graph):
    """The solver's graph as the reference's dicts: (g with init / ij / meas / info / fixed, priors)"""
    s = graph.solver
    ne = len(s._ij)
    g = dict(init=np.stack(s._nodes) if s.h is None else s.poses(), ij=np.array(s._ij, np.int32).reshape(ne, 2), meas=np.stack(s._meas),
             info=np.stack(s._info), fixed=s.fixed)
    p = s._priors
    pr = dict(vertex=np.array([q["vertex"] for q in p], np.int32), type=np.array([q["type"] for q in p], np.int32),
              meas=np.stack([q["meas"] for q in p]), info=np.stack([q["info"] for q in p]),
              kernels=np.array([q["kind"] for q in p], np.int32), deltas=np.array([q["delta"] for q in p]))
    return g, pr


def rms_position_error(positions, truth):
    return float(np.sqrt(((np.asarray(positions) - np.asarray(truth)) ** 2).sum(1).mean()))


class NoLoops:
    """a loop detector that never finds one (and needs no device): what the L-shaped path gives the real one"""
    def detect_nearest(self, keyframes, new_keyframes):
        return []
