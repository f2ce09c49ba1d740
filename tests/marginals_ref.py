"""numpy fp64 reference for the pose-graph marginal covariances (lslam_pg_marginals, lslam_pg_relative_covariances), shared by
tests/test_marginals_ref.py (CPU) and tests/test_gpu_pg_marginals.py (GPU).

  * covariance(): the dense H from a block system in lslam_pg_linearize's layout (diag, off, off_ij), Sigma = inv(H) with the
    fixed vertex's rows and columns zeroed.
  * relative_jacobians(): central finite differences of the edge error of oracle/posegraph_oracle.py (through
    tests/posegraph_se3.py) under the increment pg_update_kernel applies, X <- X * fromVectorMQT(d), for an edge (ref, j) whose
    measurement is the current relative pose.  Independent of the device's analytic Jacobians.  Five-point central stencil at
    h = 2e-3: truncation h^4 / 30 f^(5), rounding ~ eps / h; FD_REL below is its own error, measured by halving h
    (tests/test_marginals_ref.py asserts it).
  * column_bound(): what a column of H^-1 solved to |r| <= tol |e| may differ from the reference by -- derived, not tuned:
    x - H^-1 e = H^-1 (H x - e), so |x - H^-1 e|_2 <= ||Sigma||_2 |H x - e|; the factor 2 covers the recurrence residual of CG
    against the true residual; 64 eps kappa(H) ||Sigma||_2 is the reference's own error (numpy's LU inverse, backward stable:
    relative error of order eps kappa).
Nothing here was calibrated against what the kernels return."""
import numpy as np

import posegraph_se3 as se3

po = se3.po
EPS = np.finfo(np.float64).eps
FD_H = 2e-3
FD_REL = 2e-11  # relative_jacobians(h) against (h / 2), relative to the largest Jacobian entry (measured: up to 7.6e-12)


def dense_H(sysd):
    n = len(sysd["diag"])
    H = np.zeros((6 * n, 6 * n))
    for v in range(n):
        H[6 * v:6 * v + 6, 6 * v:6 * v + 6] = sysd["diag"][v]
    for (a, c), blk in zip(np.asarray(sysd["off_ij"]).tolist(), sysd["off"]):
        H[6 * a:6 * a + 6, 6 * c:6 * c + 6] = blk
        H[6 * c:6 * c + 6, 6 * a:6 * a + 6] = blk.T
    return H


def covariance(sysd, fixed):
    """-> (H, Sigma): Sigma = inv(H), the fixed vertex's rows and columns zeroed (its block of H^-1 is the identity)."""
    H = dense_H(sysd)
    S = np.linalg.inv(H)
    if fixed >= 0:
        f = slice(6 * fixed, 6 * fixed + 6)
        S[f, :] = 0.0
        S[:, f] = 0.0
    return H, S


def column_bound(H, S, tol):
    """|x - Sigma e|_2 for one solved column (module docstring)."""
    nS = np.linalg.norm(S, 2)
    return 2.0 * tol * nS + 64.0 * EPS * np.linalg.cond(H) * nS


def block(S, a, b):
    return S[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def relative_jacobians(poses, ref, js, h=FD_H):
    """[J_ref | J_j] (n, 6, 12) of an edge (ref, j) measured as the current relative pose, five-point central differences."""
    js = np.asarray(js, np.int64).reshape(-1)
    xi, xj = poses[np.full(len(js), ref)], poses[js]
    meas = po.pose_mul(po.pose_inv(xi), xj)
    J = np.zeros((len(js), 6, 12))
    for k in range(6):
        d = np.zeros((len(js), 6))
        d[:, k] = h
        for mult, wgt in ((1.0, 8.0), (-1.0, -8.0), (2.0, -1.0), (-2.0, 1.0)):
            inc = po.from_vector_mqt(mult * d)
            J[:, :, k] += wgt * po._err_pairs(po.pose_mul(xi, inc), xj, meas) / (12.0 * h)
            J[:, :, 6 + k] += wgt * po._err_pairs(xi, po.pose_mul(xj, inc), meas) / (12.0 * h)
    return J


def relative_covariance(S, poses, ref, js):
    """Sigma_rel (n, 6, 6) = [J_r J_j] Sigma_(r,j) [J_r J_j]^T; j == ref: zeros.  Also returns the Jacobians."""
    js = np.asarray(js, np.int64).reshape(-1)
    J = relative_jacobians(poses, ref, js)
    out = np.zeros((len(js), 6, 6))
    for k, j in enumerate(js):
        if j == ref:
            continue
        idx = np.r_[6 * ref:6 * ref + 6, 6 * j:6 * j + 6]
        out[k] = J[k] @ S[np.ix_(idx, idx)] @ J[k].T
    return out, J


def relative_bound(H, S, J, tol):
    """Bound on |Sigma_rel - reference|_F for one query: the joint 12x12 marginal is 12 solved columns (Frobenius error at most
    sqrt(12) column bounds, symmetrising does not increase it) propagated through ||[J_r J_j]||_2^2, plus the reference's own
    finite-difference error: dJ <= FD_REL max|J| per entry (Frobenius sqrt(72) of that), entering twice."""
    nJ = np.linalg.norm(J, 2)
    dJ = FD_REL * np.abs(J).max() * np.sqrt(72.0)
    return nJ * nJ * np.sqrt(12.0) * column_bound(H, S, tol) + 2.0 * nJ * dJ * np.linalg.norm(S, 2)


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def random_spd(rng, n, lo=0.5, hi=2.0):
    A = rng.normal(size=(n, 6, 6))
    W = A @ np.transpose(A, (0, 2, 1)) + rng.uniform(lo, hi, (n, 1, 1)) * np.eye(6)
    return 0.5 * (W + np.transpose(W, (0, 2, 1)))


def make_chain(n, seed, n_loops=0, fixed=0, box=10.0, meas_sigma=(0.05, 0.02), init_sigma=(0.2, 0.03)):
    """A chain of n vertices with random SE(3) poses (uniform positions in a cube, uniformly random rotations), full random SPD
    information, `n_loops` extra random edges; the estimate is the ground truth perturbed, so that H is evaluated away from the
    optimum.  n = 1: a single vertex without edges."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    gt = np.concatenate([rng.uniform(-box / 2, box / 2, (n, 3)), q], 1)
    edges = [(v, v + 1) for v in range(n - 1)]
    while len(edges) < n - 1 + n_loops:
        a, b = (int(v) for v in rng.choice(n, 2, replace=False))
        if abs(a - b) > 1:
            edges.append((a, b))
    ij = np.array(edges, np.int32).reshape(-1, 2)

    def perturbed(p, sig):
        d = np.concatenate([rng.normal(0, sig[0], (len(p), 3)), rng.normal(0, sig[1], (len(p), 3))], 1)
        out = po.pose_mul(p, po.from_vector_mqt(d))
        out[:, 3:] /= np.linalg.norm(out[:, 3:], axis=1, keepdims=True)
        return out

    meas = perturbed(po.pose_mul(po.pose_inv(gt[ij[:, 0]]), gt[ij[:, 1]]), meas_sigma) if len(ij) else np.zeros((0, 7))
    init = perturbed(gt, init_sigma)
    if fixed >= 0:
        init[fixed] = gt[fixed]
    return dict(gt=gt, init=init, ij=ij, meas=meas, info=random_spd(rng, len(ij)), fixed=fixed)


def adjoint_right(T):
    """For B = (R, t) as a pose 7-vector: the matrix that carries a right increment [dt, dq_v] applied BEFORE B to the equal
    increment applied AFTER it, A [d] B = A B [Ad d] to first order: [[R^T, -2 R^T [t]x], [0, R^T]] (dq_v is half the angle)."""
    x, y, z, w = T[3:]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = T[:3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    A = np.zeros((6, 6))
    A[:3, :3] = R.T
    A[:3, 3:] = -2.0 * R.T @ tx
    A[3:, 3:] = R.T
    return A
