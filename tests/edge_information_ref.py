"""numpy restatement of the edge-information specification of include/lslam_c.h: the Gauss-Newton normal matrix of a scan
match in the pose graph's edge coordinates [t, q], from a sweep's taps, and the policy that turns it into an edge's
information (graph.py).  The sums are math.fsum's: exact, then rounded once.

Shared by tests/test_edge_information_ref.py (CPU: the Jacobian against finite differences of the frozen-correspondence
residual, the policy) and tests/test_gpu_edge_information.py (GPU: the kernel against these sums).
"""
import math

import numpy as np

UPPER = [(r, c) for r in range(6) for c in range(r, 6)]  # the 21 upper-triangular entries, row-major
U = 2.0 ** -53


def rows(points, coeff, flags, T):
    """-> (J (n_kept, 6) float64, b (n_kept,)) of the rows kept (flags & 4), in point order.  points (n, >= 3) float32 in the
    sensor frame, coeff (n, 4) float32, T the float32 4x4 of lslam_pose_to_isometry.  Every operation rounded on its own, in the
    header's order: the same bits as the device forms."""
    p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    cf = np.asarray(coeff, np.float32).astype(np.float64)
    keep = (np.asarray(flags, np.uint8) & 4) != 0
    R = np.asarray(T, np.float32).reshape(4, 4)[:3, :3].astype(np.float64)
    p, cf = p[keep], cf[keep]
    c0, c1, c2 = cf[:, 0], cf[:, 1], cf[:, 2]
    m = [(R[0, j] * c0 + R[1, j] * c1) + R[2, j] * c2 for j in range(3)]
    x = [p[:, 1] * m[2] - p[:, 2] * m[1], p[:, 2] * m[0] - p[:, 0] * m[2], p[:, 0] * m[1] - p[:, 1] * m[0]]
    J = np.stack(m + [2.0 * v for v in x], axis=1)
    return J, cf[:, 3]


def exact_sums(points, coeff, flags, T, n_corner):
    """-> dict: H (6, 6) and sum_b2 (exact sums, rounded once), absH (6, 6) = sum |J_a J_b| and abs_b2 (what the fp64
    summation bound scales with), n_rows, n_line, n_plane."""
    J, b = rows(points, coeff, flags, T)
    H, A = np.zeros((6, 6)), np.zeros((6, 6))
    for r, c in UPPER:
        prod = J[:, r] * J[:, c]  # (the device's products are rounded too: one more rounding per term, inside the bound)
        H[r, c] = H[c, r] = exact_dot(J[:, r], J[:, c])
        A[r, c] = A[c, r] = math.fsum(np.abs(prod).tolist())
    f = np.asarray(flags, np.uint8)
    fit = (f & 2) != 0
    return dict(H=H, absH=A, sum_b2=exact_dot(b, b), abs_b2=math.fsum((b * b).tolist()), n_rows=int(((f & 4) != 0).sum()),
                n_line=int(fit[:n_corner].sum()), n_plane=int(fit[n_corner:].sum()), J=J, b=b)


def exact_dot(a, b):
    """sum a_k b_k with exact products (Dekker's split through fractions would be overkill: float products of float64 values
    are summed as exact pairs hi + lo by math.fsum)."""
    terms = []
    for x, y in zip(a.tolist(), b.tolist()):
        hi = x * y
        terms.append(hi)
        terms.append(_two_prod_err(x, y, hi))
    return math.fsum(terms)


def _two_prod_err(x, y, hi):
    """x * y - hi exactly (Veltkamp / Dekker; no overflow for the magnitudes of a scan match)."""
    def split(v):
        t = 134217729.0 * v
        h = t - (t - v)
        return h, v - h
    xh, xl = split(x)
    yh, yl = split(y)
    return ((xh * yh - hi) + xh * yl + xl * yh) + xl * yl


def sum_bound(n_rows, abs_sum):
    """The project's fp64 summation bound (tests/test_gpu_icp_general.py): any order of n_rows rounded products."""
    return (n_rows + 8) * U * abs_sum


def residuals(points, coeff, flags, T64, delta):
    """The frozen-correspondence weighted residual c . (T * fromVectorMQT(delta) * p) + const of every kept row, float64; T64:
    pose [t, q] (float64) of T."""
    from posegraph_se3 import po
    p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    cf = np.asarray(coeff, np.float32).astype(np.float64)
    keep = (np.asarray(flags, np.uint8) & 4) != 0
    p, cf = p[keep], cf[keep]
    X = po.pose_mul(np.asarray(T64, np.float64), po.from_vector_mqt(np.asarray(delta, np.float64)))
    w = po.qrot(X[3:][None, :].repeat(len(p), 0), p) + X[:3]
    return (cf[:, :3] * w).sum(1)


# ---- the policy (graph.py; include/lslam_loop_closure.hpp) --------------------------------------------------------------------
MIN_ROWS = 50  # ScanMatch.cpp:142: the reference's floor for a usable match


def edge_information(omega_ref, H, sum_b2, n_rows, range_sigma):
    """Omega = Omega_ref + H / max(sum_b2 / (n_rows - 6), range_sigma^2); Omega_ref alone where n_rows < 50."""
    omega_ref = np.asarray(omega_ref, np.float64)
    H = np.asarray(H, np.float64).reshape(6, 6)
    if n_rows < MIN_ROWS or not (np.isfinite(H).all() and math.isfinite(sum_b2)):  # sums that are not finite say nothing
        return omega_ref.copy()
    s2 = max(float(sum_b2) / float(n_rows - 6), float(range_sigma) * float(range_sigma))
    return omega_ref + H / s2
