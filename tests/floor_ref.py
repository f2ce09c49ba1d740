"""Independent numpy reference of the floor detection (include/lslam_c.h, "floor detection") and of the pose graph's plane
priors ("plane priors"), written from the header's specification and sharing nothing with the library.

Detection: the hash, the candidate rule, the fp64 hypothesis planes, the fp32 counts, the tie rule, the refit and the statuses.
fp32 expressions are numpy float32 operations in the header's order (numpy rounds after every operation: no FMA).  The refit
sums are exact (math.fsum), so they are free of any order; the device's fixed-order fp64 sums are held to them within a bound
derived from the count and the extent (refit_bounds).
"""
import math

import numpy as np

FLOOR_OK, FLOOR_FEW_CANDIDATES, FLOOR_NO_HYPOTHESIS, FLOOR_FEW_INLIERS, FLOOR_STEEP = 0, 1, 2, 3, 4
DEFAULTS = dict(up=(0.0, 0.0, 1.0), sensor_height=1.8, height_clip_range=1.0, max_range=0.0, n_hypotheses=512,
                inlier_threshold=0.1, min_inliers=512, max_normal_angle_deg=10.0, refit_iterations=1, seed=1)
U53 = 2.0 ** -53
F32 = np.float32


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in p:
            raise TypeError(k)
    p.update(kw)
    return p


# ---- the hash --------------------------------------------------------------------------------------------------------------
def fmix32(h):
    """MurmurHash3's 32-bit finaliser, on Python ints or uint64 arrays holding 32-bit values."""
    M = 0xFFFFFFFF
    h = h & M
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    h ^= h >> 16
    return h


def slots(seed, H, K):
    """-> int64[H, 3]: slot j of hypothesis h = (fmix32(seed + 0x9E3779B9 (3 h + j + 1)) K) >> 32."""
    out = np.zeros((H, 3), np.int64)
    for h in range(H):
        for j in range(3):
            x = fmix32((int(seed) + 0x9E3779B9 * (3 * h + j + 1)) & 0xFFFFFFFF)
            out[h, j] = (x * int(K)) >> 32
    return out


# ---- the stages ------------------------------------------------------------------------------------------------------------
def unit_up(p):
    u = np.array([float(F32(v)) for v in p["up"]], np.float64)
    u = u / math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    return u, u.astype(F32)


def cos_max(p):
    return math.cos(float(F32(p["max_normal_angle_deg"])) * (3.14159265358979323846 / 180.0))


def candidates(pts, p):
    """-> int64[K], the candidates' input indices in input order."""
    a = np.asarray(pts, F32)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    _, u = unit_up(p)
    with np.errstate(all="ignore"):
        h = (u[0] * x + u[1] * y) + u[2] * z
        lo = -(F32(p["sensor_height"]) + F32(p["height_clip_range"]))
        hi = -(F32(p["sensor_height"]) - F32(p["height_clip_range"]))
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (h >= lo) & (h <= hi)
        if F32(p["max_range"]) > 0:
            ok &= ((x * x + y * y) + z * z) <= F32(p["max_range"]) * F32(p["max_range"])
    return np.flatnonzero(ok)


def hypotheses(cand, p):
    """cand: float32[K, >= 3] -> (triples int64[H, 3], planes float64[H, 4], mark int[H]: 0 votes, -1 degenerate, -2 steep)."""
    H, K = int(p["n_hypotheses"]), len(cand)
    tri = slots(p["seed"], H, K)
    planes, mark = np.zeros((H, 4)), np.full(H, -1, np.int64)
    u, _ = unit_up(p)
    cm = cos_max(p)
    c64 = np.asarray(cand, F32)[:, :3].astype(np.float64)
    for h in range(H):
        s = tri[h]
        if K == 0 or s[0] == s[1] or s[0] == s[2] or s[1] == s[2]:
            continue
        a, b, c = c64[s[0]], c64[s[1]], c64[s[2]]
        e1, e2 = b - a, c - a
        n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        u2 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
        v2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]
        if not n2 > (1e-12 * u2) * v2:
            continue
        n = n / math.sqrt(n2)
        dot = (n[0] * u[0] + n[1] * u[1]) + n[2] * u[2]
        if dot < 0.0:
            n, dot = -n, -dot
        d = -((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2])
        planes[h] = (n[0], n[1], n[2], d)
        mark[h] = -2 if dot < cm else 0
    return tri, planes, mark


def inliers32(plane32, cand, thr):
    """The fp32 test: fabsf(((nx x + ny y) + nz z) + d) <= thr -> bool[K]."""
    pl = np.asarray(plane32, F32)
    a = np.asarray(cand, F32)
    with np.errstate(all="ignore"):
        dist = ((pl[0] * a[:, 0] + pl[1] * a[:, 1]) + pl[2] * a[:, 2]) + pl[3]
        return np.abs(dist) <= F32(thr)


def counts(planes32, mark, cand, thr):
    """-> int64[H]: the inlier count of every voting hypothesis, the mark of the others."""
    out = np.array(mark, np.int64)
    for h in np.flatnonzero(out == 0):
        out[h] = int(inliers32(planes32[h], cand, thr).sum())
    return out


def best(cnt):
    """The largest count, the lowest index among equals; -1 when no hypothesis votes."""
    cnt = np.asarray(cnt)
    if not (cnt >= 0).any():
        return -1
    return int(np.argmax(np.where(cnt >= 0, cnt, -1)))  # argmax returns the first maximum


def exact_sums(pts64):
    """sum p [3], sum p p^T [3, 3], exactly (fsum), from float64 copies of fp32 points."""
    s1 = np.array([math.fsum(pts64[:, k]) for k in range(3)])
    s2 = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            s2[i, j] = s2[j, i] = math.fsum(pts64[:, i] * pts64[:, j])  # a product of two fp32 values is exact in fp64
    return s1, s2


def fit(pts64, u):
    """centroid, covariance, eigenvector of the smallest eigenvalue oriented to u, d = -n.c -> (plane[4], eigenvalues[3])."""
    N = len(pts64)
    s1, s2 = exact_sums(pts64)
    c = s1 / N
    C = s2 / N - np.outer(c, c)
    w, V = np.linalg.eigh(C)
    n = V[:, 0] / np.linalg.norm(V[:, 0])
    if n @ u < 0:
        n = -n
    return np.array([n[0], n[1], n[2], -(n @ c)]), w


def detect(pts, p, planes32=None):
    """The whole detection -> dict: the result's fields, and the taps ``cand_idx``, ``triples``, ``planes`` (fp64),
    ``marks``, ``counts``, per refit ``refits`` = [(plane, eigenvalues, n_inliers, extent)].  planes32: score with THESE fp32
    planes (the device's downloaded ones) instead of the reference's own rounded to fp32."""
    a = np.asarray(pts, F32)
    idx = candidates(a, p)
    cand = a[idx, :3]
    K = len(idx)
    tri, planes, mark = hypotheses(cand, p)
    p32 = planes.astype(F32) if planes32 is None else np.asarray(planes32, F32)
    thr = F32(p["inlier_threshold"])
    cnt = counts(p32, mark, cand, thr)
    b = best(cnt)
    u, _ = unit_up(p)
    out = dict(plane=np.zeros(4), n_candidates=K, n_inliers=0, best_hypothesis=-1, best_count=0, rms_distance=0.0,
               status=FLOOR_OK, cand_idx=idx, triples=tri, planes=planes, marks=mark, counts=cnt, refits=[])
    if K < 3 or K < int(p["min_inliers"]):
        out["status"] = FLOOR_FEW_CANDIDATES
        return out
    if b < 0:
        out["status"] = FLOOR_NO_HYPOTHESIS
        return out
    out["best_hypothesis"], out["best_count"] = b, int(cnt[b])
    need = max(3, int(p["min_inliers"]))
    plane = p32[b].astype(np.float64)
    out["plane"] = plane
    c64 = cand.astype(np.float64)
    for it in range(int(p["refit_iterations"]) + 1):
        m = inliers32(plane.astype(F32), cand, thr)
        N = int(m.sum())
        out["n_inliers"] = N
        d = c64[m] @ plane[:3] + plane[3]
        out["rms_distance"] = math.sqrt(math.fsum(d * d) / N) if N else 0.0
        if N < need:
            out["status"] = FLOOR_FEW_INLIERS
            return out
        if it == int(p["refit_iterations"]):
            break
        plane, w = fit(c64[m], u)
        out["plane"] = plane
        out["refits"].append((plane, w, N, float(np.abs(c64[m]).max())))
        if plane[:3] @ u < cos_max(p):
            out["status"] = FLOOR_STEEP
            return out
    return out


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def plane32_bounds(extent):
    """|downloaded fp32 plane - reference fp64 plane| <= (bn per normal component, bd for d).  A unit normal's components are at
    most 1: rounding to fp32 moves one by at most half an ulp of [0.5, 1], 2^-25; |d| = |n.a| <= sqrt(3) extent: half an ulp of a
    value below 2^ceil(log2(sqrt(3) extent)).  The two fp64 evaluations (three subtractions, a cross product, a square root,
    three divisions, a dot product: under 16 roundings, each relative 2^-53, of quantities bounded as above) may differ by
    16 * 2^-53 of those magnitudes."""
    dmax = math.sqrt(3.0) * max(extent, 1.0)
    bn = 2.0 ** -25 + 16 * U53
    bd = 2.0 ** (math.ceil(math.log2(dmax)) - 24) + 16 * U53 * dmax
    return bn, bd


def refit_bounds(N, extent, eigenvalues):
    """|device refit plane - reference refit plane| <= (bn, bd).  The device sums N terms in fp64 in a fixed order: whatever
    the order, |error| <= (N - 1) 2^-53 sum |terms| (Higham, Accuracy and Stability, eq. 4.4), i.e. <= N^2 u E for sum p and
    N^2 u E^2 for sum p p^T with E the largest |coordinate|; the reference's sums are exact.  So the centroid errs by at most
    N u E, an entry of C = S2 / N - c c^T by 3 N u E^2 (+ 4 u E^2 of its own roundings), the matrix by 3 times that in the
    Frobenius norm; the eigenvector of the smallest eigenvalue turns by at most 2 |dC| / gap (Davis-Kahan), gap = the distance
    to the next eigenvalue, plus the two eigen-solvers' own backward errors, 64 u |C| <= 64 u 3 E^2 each.  d = -n.c inherits
    sqrt(3) E per unit of normal error, the centroid's error and 4 roundings."""
    E = max(float(extent), 1e-30)
    gap = float(eigenvalues[1] - eigenvalues[0])
    dC = 3.0 * (3.0 * N + 4.0) * U53 * E * E + 2.0 * 64.0 * U53 * 3.0 * E * E
    bn = 2.0 * dC / gap
    bd = bn * math.sqrt(3.0) * E + math.sqrt(3.0) * (N + 4.0) * U53 * E
    return bn, bd


# ---- scenes ----------------------------------------------------------------------------------------------------------------
TINY_SLOPE, TINY_SIGMA, TINY_HALF = 0.02, 0.01, 10.0


def tiny_scene(seed=0):
    """The prototype's tiny scene in the sensor frame: 1600 ground points on a 2 % slope in x (z = -1.8 + 0.02 x, noise
    TINY_SIGMA), a 400-point wall at x = 8 and 300 clutter points in the height band -> (float32[2300, 4] shuffled, the planted
    plane (n, d) with a unit normal)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((1600, 3))
    g[:, :2] = rng.uniform(-TINY_HALF, TINY_HALF, (1600, 2))
    g[:, 2] = -1.8 + TINY_SLOPE * g[:, 0] + rng.normal(0, TINY_SIGMA, 1600)
    w = np.stack([np.full(400, 8.0), rng.uniform(-5, 5, 400), rng.uniform(-1.8, 1.2, 400)], 1)
    c = np.stack([rng.uniform(-TINY_HALF, TINY_HALF, 300), rng.uniform(-TINY_HALF, TINY_HALF, 300), rng.uniform(-2.8, -0.8, 300)], 1)
    pts = np.concatenate([g, w, c])[rng.permutation(2300)]
    out = np.zeros((2300, 4), F32)
    out[:, :3] = pts
    n = np.array([-TINY_SLOPE, 0.0, 1.0])
    s = np.linalg.norm(n)
    return out, np.array([n[0] / s, n[1] / s, n[2] / s, 1.8 / s])


def plane_error(got, want):
    """-> (angle between the normals [rad], |d difference|)."""
    c = float(np.clip(np.dot(got[:3], want[:3]) / (np.linalg.norm(got[:3]) * np.linalg.norm(want[:3])), -1, 1))
    return math.acos(c) if c < 1 - 1e-9 else float(np.linalg.norm(np.cross(got[:3], want[:3]))), abs(got[3] - want[3])


def plane_in_sensor_frame(world4, R, t):
    """The world plane seen from a sensor at (R, t), sensor -> world: n_l = R^T n_w, d_l = d_w + n_w.t."""
    n = np.asarray(world4[:3], np.float64)
    return np.concatenate([R.T @ n, [world4[3] + n @ t]])


# What detect() itself achieves on synth.make_scan(rings=16, azimuth_steps=450) with the default parameters, against the world
# floor (0, 0, 1, 0) carried into the sensor frame by the returned pose: measured by tests/test_floor_ref.py on the CPU (it
# asserts the recorded figures still hold); the GPU test allows ten times these.
SYNTH_REF_ANGLE, SYNTH_REF_DIST = 3.0e-5, 9.0e-4  # measured: 2.36e-5 rad, 8.34e-4 m (the range noise is 0.02 m)


# =============================================================================================================================
# Plane priors of the pose-graph solver (include/lslam_c.h, "plane priors"), in the conventions of oracle/posegraph_oracle.py:
# update X <- X * fromVectorMQT(d).  Built on posegraph_se3 / posegraph_prior_ref by import (loaded on first use: the detection
# half above needs neither the oracle nor scipy).
#
# MEASURED FLOORS (tests/test_floor_ref.py asserts the references stay inside them; the GPU tests use ten times them; nothing
# was calibrated against the GPU).
#   (a) analytic J against central differences (h = 1e-6) under the update rule, 200 random poses and plane pairs with |t| up to
#       10 m: 1.1e-9 of the largest Jacobian entry (2 for the tangent rows, 1 for the distance row); the differences at h against
#       h / 2: 3.1e-9.  The distance row differences d_w + n_w.t with |t| up to 10 m: the rounding eps |t| / h of the
#       differences dominates, as for posegraph_prior_ref.XYZ_FD_REL.  Recorded as PLANE_FD_REL = 4e-9.
#   (b) the system: plane_system(oracle="c") against plane_system(oracle="np") differ only in what prior_system contributes (the
#       plane terms are the same numpy arithmetic on both sides), so posegraph_se3.O2O_* hold unchanged; the plane priors permuted:
#       (four permutations per LIN_PRIOR_CASES graph) diag 3.9e-17 max|diag|, b 4.1e-17 max|b|, chi2 0 -- inside posegraph_se3.SPREAD_*, reused unchanged.
PLANE_FD_REL = 4e-9


def _pp():
    import posegraph_prior_ref as pp
    return pp


def unit_plane(pl):
    pl = np.asarray(pl, np.float64)
    return pl / np.linalg.norm(pl[..., :3], axis=-1, keepdims=True)


def tangent_basis(nm):
    """a = the unit axis of the smallest |n_m| component (the lowest index among equals); b1 = normalise(n_m x a); b2 = n_m x b1"""
    a = np.zeros(3)
    a[int(np.argmin(np.abs(nm)))] = 1.0  # argmin returns the first minimum
    b1 = np.cross(nm, a)
    b1 = b1 / np.linalg.norm(b1)
    return b1, np.cross(nm, b1)


def plane_local(pose, world4):
    """The world plane in the sensor frame of X = (t, q): n_l = R^T n_w, d_l = d_w + n_w.t"""
    R = _pp().quat_matrix(pose[3:])
    w = unit_plane(world4)
    return R.T @ w[:3], w[3] + w[:3] @ pose[:3]


def plane_error3(pose, world4, meas4):
    m = unit_plane(meas4)
    nl, dl = plane_local(pose, world4)
    b1, b2 = tangent_basis(m[:3])
    return np.array([b1 @ nl, b2 @ nl, dl - m[3]])


def plane_jacobian(pose, world4, meas4):
    """analytic, 3 x 6: rows 0, 1 = [0 | 2 (b_k x n_l)^T], row 2 = [n_l^T | 0]"""
    m = unit_plane(meas4)
    nl, _ = plane_local(pose, world4)
    b1, b2 = tangent_basis(m[:3])
    J = np.zeros((3, 6))
    J[0, 3:], J[1, 3:], J[2, :3] = 2.0 * np.cross(b1, nl), 2.0 * np.cross(b2, nl), nl
    return J


def plane_jacobian_numeric(pose, world4, meas4, h=1e-6):
    """central differences of the error under X <- X * fromVectorMQT(d)"""
    po = _pp().po
    J = np.zeros((3, 6))
    for k in range(6):
        d = np.zeros((1, 6))
        d[0, k] = h
        J[:, k] = (plane_error3(po.pose_mul(pose[None], po.from_vector_mqt(d))[0], world4, meas4)
                   - plane_error3(po.pose_mul(pose[None], po.from_vector_mqt(-d))[0], world4, meas4)) / (2 * h)
    return J


def empty_planes():
    return dict(vertex=np.zeros(0, np.int32), world=np.zeros((0, 4)), meas=np.zeros((0, 4)), info=np.zeros((0, 3, 3)),
                kernels=np.zeros(0, np.int32), deltas=np.ones(0))


def make_planes(g, vertices, seed, sigma=(0.05, 0.1), world=None):
    """One plane prior per entry of `vertices` (a vertex may repeat): a random world plane (or `world`) carried into the sensor
    frame by the GROUND TRUTH, its normal turned by about sigma[0] rad and its distance moved by sigma[1]; planes are given
    un-normalised (scaled by 0.5 .. 2); dense, exactly symmetric SPD 3x3 information."""
    rng = np.random.default_rng(3000 + seed)
    vertices = np.asarray(vertices, np.int32)
    n = len(vertices)
    W, M = np.zeros((n, 4)), np.zeros((n, 4))
    for p in range(n):
        w = np.concatenate([rng.normal(size=3), [rng.uniform(-3, 3)]]) if world is None else np.asarray(world, np.float64)
        nl, dl = plane_local(g["gt"][vertices[p]], w)
        nm = nl + rng.normal(0, sigma[0], 3)
        M[p] = np.concatenate([nm / np.linalg.norm(nm), [dl + rng.normal(0, sigma[1])]]) * rng.uniform(0.5, 2.0)
        W[p] = w * (rng.uniform(0.5, 2.0) if world is None else 1.0)
    A = rng.normal(size=(n, 3, 3))
    info = A @ np.transpose(A, (0, 2, 1)) + rng.uniform(0.5, 2.0, (n, 1, 1)) * np.eye(3)
    info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    return dict(vertex=vertices, world=W, meas=M, info=info, kernels=np.zeros(n, np.int32), deltas=np.ones(n))


def planes_permuted(pl, order):
    return {k: np.asarray(v)[order] for k, v in pl.items()}


def plane_rho(poses, pl):
    """-> (e2, rho0, rho1) per plane prior under its kernel"""
    import robust_posegraph_ref as rr
    n = len(pl["vertex"])
    e2 = np.zeros(n)
    for p in range(n):
        e = plane_error3(poses[pl["vertex"][p]], pl["world"][p], pl["meas"][p])
        e2[p] = e @ pl["info"][p] @ e
    if n == 0:
        return e2, e2.copy(), np.ones(0)
    r0, r1 = rr.rho_edges(pl["kernels"], pl["deltas"], e2)
    return e2, r0, r1


def plane_system(g, pr, pl, poses=None, oracle="np", fixed=None):
    """posegraph_prior_ref.prior_system of the edges and the POSE / XYZ priors `pr` (None: none), plus the plane priors `pl`
    under their kernels, in plane-prior order; the fixed vertex gets the identity block afterwards, so a plane prior on it adds
    its rho0 to chi2 only.  Also returns the plane priors' e2 / rho / weight (plane_e2, plane_rho, plane_weight)."""
    pp = _pp()
    p = g["init"] if poses is None else poses
    fixed = g["fixed"] if fixed is None else fixed
    s = pp.prior_system(g, pp.empty_priors() if pr is None else pr, p, oracle, fixed=-1)
    e2, r0, r1 = plane_rho(p, pl)
    for q in range(len(pl["vertex"])):
        v = pl["vertex"][q]
        e = plane_error3(p[v], pl["world"][q], pl["meas"][q])
        J = plane_jacobian(p[v], pl["world"][q], pl["meas"][q])
        A = J.T @ pl["info"][q]
        s["diag"][v] += r1[q] * (A @ J)
        s["b"][6 * v:6 * v + 6] -= r1[q] * (A @ e)
    s["chi2"] = float(s["chi2"] + np.sum(r0))
    pp._fix(s, fixed)
    s.update(plane_e2=e2, plane_rho=r0, plane_weight=r1)
    return s


def plane_total_chi2(poses, g, pr, pl):
    pp = _pp()
    return float(pp.total_chi2(poses, g, pp.empty_priors() if pr is None else pr) + np.sum(plane_rho(poses, pl)[1]))


def plane_optimize(g, pr, pl, fixed=None, max_iters=50, rel_tol=0.0, solve=None):
    """posegraph_prior_ref.optimize's schedule (g2o's Levenberg) on edges + priors + plane priors, dense enough for graphs of about
    a dozen vertices.  rel_tol > 0: also stop once an accepted step lowers chi2 by less than rel_tol of itself (the two stopping
    tolerances whose spread the graph tests compare against).  -> (poses, history)"""
    pp = _pp()
    fixed = g["fixed"] if fixed is None else fixed
    solve = solve or pp.solve_damped
    poses = g["init"].copy()
    hist, lam, ni = [], None, 2.0
    for it in range(max_iters):
        s = plane_system(g, pr, pl, poses, "np", fixed=-1)
        H, b, cur = pp.to_sparse(s), s["b"], s["chi2"]
        if lam is None:
            d = H.diagonal().copy()
            if fixed >= 0:
                d[6 * fixed:6 * fixed + 6] = 0.0
            lam = 1e-5 * d.max()
        gain, qmax, before = 0.0, 0, cur
        while True:
            dx = solve(H, b, lam, fixed)
            trial = pp.oplus(poses, dx, fixed)
            tmp = plane_total_chi2(trial, g, pr, pl)
            gain = (cur - tmp) / (float(dx @ (lam * dx + b)) + 1e-3)
            if gain > 0 and np.isfinite(tmp):
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
        if rel_tol > 0 and before - cur <= rel_tol * before:
            break
    return poses, hist


def plane_e2_rounding(poses, pl):
    """Per plane prior, how far two correct fp64 evaluations of e2 = e^T Omega e may differ, relative to e2, because of the
    error's own conditioning: d_l - d_m = d_w + n_w.t - d_m and b.n_l are differences of terms up to 1 + |d_w| + |t|_1 + |d_m| in
    size (seven roundings each, in any order: 16 u of that size covers two evaluations), and d e2 = 2 (Omega e).de.  Small
    where the error is large against the pose's coordinates (the initial estimates), the dominant term where it is small
    (ground truth 10 m from the origin with centimetre residuals)."""
    out = np.zeros(len(pl["vertex"]))
    for p in range(len(out)):
        x = poses[pl["vertex"][p]]
        e = plane_error3(x, pl["world"][p], pl["meas"][p])
        size = 1.0 + abs(unit_plane(pl["world"][p])[3]) + np.abs(x[:3]).sum() + abs(unit_plane(pl["meas"][p])[3])
        out[p] = 2.0 * np.abs(pl["info"][p] @ e).sum() * 16 * U53 * size / (e @ pl["info"][p] @ e)
    return out


# ---- the graph node with floors (tests/test_gpu_graph_floor.py) ------------------------------------------------------------
GRAPH_FLOOR_SIGMA = (0.005, 0.01)       # (normal [rad], distance [m]): what the Graph is told
GRAPH_FLOOR_NOISE = 0.005               # range noise of the ground points [m]
GRAPH_FLOOR_DRIFT = (0.004, 0.03)       # planted per-step odometry drift: pitch [rad], z [m]
GRAPH_FLOOR_HEIGHT = 1.8
GRAPH_FLOOR_PARAMS = dict(n_hypotheses=64, min_inliers=100)
GRAPH_FLOOR_ITERS = 50
# The ramp test's odometry information (sigma 1 cm, 0.01 rad on the half-angle coordinates).  With the node's constant one
# (graph.cpp:279-288: sigma about 1 m / 0.7 rad) bending the trajectory onto an outlying floor costs less than ANY kernel charges
# for rejecting it, so no kernel can reject -- what DESIGN says of loops; a rejection needs odometry that is worth something.
GRAPH_FLOOR_STRONG_ODOMETRY = np.diag([1e4, 1e4, 1e4, 1e4, 1e4, 1e4])


def _yaw_pitch_pose(x, y, z, yaw, pitch=0.0):
    T = np.eye(4)
    c, s, cp, sp_ = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cp, 0.0, sp_], [0.0, 1.0, 0.0], [-sp_, 0.0, cp]])
    T[:3, 3] = [x, y, z]
    return T


def graph_floor_scenario(n=10, corner=5, all_wall=None, tilted=None, tilt=0.08, drift=True):
    """`n` keyframes 1 m apart on an L-shaped path over flat ground (z = 0; the sensor GRAPH_FLOOR_HEIGHT above it), in the shape
    of posegraph_prior_ref.graph_gps_scenario.  Odometry starts at the true first pose -- the graph frame's floor is z = 0 -- and
    carries a planted drift in pitch and z on every step.  Each keyframe's surface cloud, built in its sensor frame from the TRUE
    pose: a 600-point ground patch within 6 m (noise GRAPH_FLOOR_NOISE along z) and a 150-point wall 5 m ahead.  `all_wall`: that
    keyframe sees only the wall (600 + 150 wall points); `tilted`: that keyframe's ground patch is tilted by `tilt` rad about its
    y axis -- a ramp taken for the floor; `drift` = False: exact odometry.  -> dict(gt, odom, clouds [(corner, surf)])"""
    rng = np.random.default_rng(4242)
    gt = np.array([_yaw_pitch_pose(0.0, float(k), GRAPH_FLOOR_HEIGHT, np.pi / 2) if k < corner
                   else _yaw_pitch_pose(float(k - corner + 1), corner - 1.0, GRAPH_FLOOR_HEIGHT, 0.0) for k in range(n)])
    drift = _yaw_pitch_pose(0.0, 0.0, GRAPH_FLOOR_DRIFT[1], 0.0, GRAPH_FLOOR_DRIFT[0]) if drift else np.eye(4)
    odom = [gt[0].copy()]
    for k in range(n - 1):
        odom.append(odom[-1] @ np.linalg.inv(gt[k]) @ gt[k + 1] @ drift)
    clouds = []
    for k in range(n):
        def wall(m):
            return np.stack([np.full(m, 5.0), rng.uniform(-4, 4, m), rng.uniform(-GRAPH_FLOOR_HEIGHT, 1.5, m)], 1)
        if k == all_wall:
            s = wall(750)
        else:
            gxy = rng.uniform(-6, 6, (600, 2))
            ground = np.stack([gxy[:, 0], gxy[:, 1], -GRAPH_FLOOR_HEIGHT + rng.normal(0, GRAPH_FLOOR_NOISE, 600)], 1)  # roll = pitch = 0: the sensor frame's z is up
            if k == tilted:
                ground[:, 2] += np.tan(tilt) * ground[:, 0]
            s = np.concatenate([ground, wall(150)])
        surf = np.zeros((len(s), 4), F32)
        surf[:, :3] = s[rng.permutation(len(s))]
        clouds.append((rng.uniform(-5, 5, (8, 4)).astype(F32), surf))
    return dict(gt=gt, odom=np.array(odom), clouds=clouds)


def drive_floor_graph(graph, sc, max_iterations):
    """every frame through add_frame + optimize; max_iterations = 0: the bookkeeping and the detection only"""
    graph._bookkeeping_only = max_iterations == 0
    for k in range(len(sc["odom"])):
        c, s = sc["clouds"][k]
        assert graph.add_frame(sc["odom"][k], c, s) is not None
        graph.optimize(max_iterations or 1000)


def graph_planes(graph):
    """the solver's plane priors as the reference's dict"""
    p = graph.solver._plane_priors
    if not p:
        return empty_planes()
    return dict(vertex=np.array([q["vertex"] for q in p], np.int32), world=np.stack([q["world"] for q in p]),
                meas=np.stack([q["meas"] for q in p]), info=np.stack([q["info"] for q in p]),
                kernels=np.array([q["kind"] for q in p], np.int32), deltas=np.array([q["delta"] for q in p]))


def z_pitch_errors(poses7, gt):
    """per keyframe: |z - true z| and the angle between the keyframe's up axis and the world's (roll and pitch together)"""
    pp = _pp()
    z = np.abs(poses7[:, 2] - gt[:, 2, 3])
    tilt = np.array([np.arccos(np.clip(pp.quat_matrix(p[3:])[2, 2], -1, 1)) for p in poses7])
    return z, tilt


def graph_edges(graph):
    """the solver's vertices and edges as the reference's dict (init: the current estimates)"""
    s = graph.solver
    ne = len(s._ij)
    return dict(init=np.stack(s._nodes) if s.h is None else s.poses(), ij=np.array(s._ij, np.int32).reshape(ne, 2),
                meas=np.stack(s._meas), info=np.stack(s._info), fixed=s.fixed)
