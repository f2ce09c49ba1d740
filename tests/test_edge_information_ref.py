"""tests/edge_information_ref.py on its own (CPU): the tangent-space Jacobian against central finite differences of the
frozen-correspondence residual c . (T * fromVectorMQT(delta) * p) -- which pins the right-hand perturbation and the factor 2 of
the quaternion's vector part -- at general poses and next to ry = 90 degrees, where the Euler form is singular; the exact sums;
and the policy that turns a match Hessian into an edge's information.

Tolerance of the finite-difference comparison, per row, relative to |c| (1 + 2 |p|) (the scale of the row's entries):
  8 * 2^-24   the reference takes the float32 T: its rotation is orthonormal to float32 rounding only, the pose [t, q] the
              residual is evaluated at is that matrix's nearest rotation
  1e-8        central differences with h = 1e-5: truncation h^2 / 6 times the third derivative (< 2e-11), rounding 2^-53 / h
              of a residual of the size of |c| |T p| (< 1e-9 at these ranges)
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_information_ref as E  # noqa: E402
from posegraph_se3 import po  # noqa: E402


def rot_euler(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz  # LOAM's order (util/transform_utils.h)


def quat_of(R):
    """Unit quaternion [x, y, z, w] of the rotation nearest to R (R: a float32 rotation widened)."""
    u, _, vt = np.linalg.svd(R)
    R = u @ vt
    w = math.sqrt(max(0.0, 1.0 + np.trace(R))) / 2.0
    if w > 1e-3:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = s / 4.0, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


POSES = [(0.3, -0.7, 1.1, 1.0, -2.0, 0.5), (-1.2, 0.4, 2.9, 30.0, 4.0, -45.0), (2.5, 1.3, -0.2, -7.0, 0.3, 12.0),
         (0.2, math.pi / 2 - 1e-3, -0.4, 3.0, 1.0, -2.0), (-0.6, math.pi / 2 + 5e-4, 0.9, -5.0, 2.0, 8.0),
         (0.1, -math.pi / 2 + 1e-4, 0.3, 0.0, 0.0, 0.0)]


def problem(seed, n=200):
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.uniform(-40.0, 40.0, (n, 3))
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    w = rng.uniform(0.1, 1.0, n)
    coeff = np.concatenate([nrm * w[:, None], (w * rng.normal(scale=0.05, size=n))[:, None]], axis=1).astype(np.float32)
    flags = rng.choice(np.array([0, 1, 3, 7], np.uint8), n, p=[0.05, 0.1, 0.15, 0.7])
    return pts, coeff, flags


@pytest.mark.parametrize("k", range(len(POSES)))
def test_jacobian_against_finite_differences(k):
    rx, ry, rz, tx, ty, tz = POSES[k]
    T = np.eye(4)
    T[:3, :3] = rot_euler(rx, ry, rz)
    T[:3, 3] = (tx, ty, tz)
    T32 = T.astype(np.float32)
    pts, coeff, flags = problem(k)
    J, b = E.rows(pts, coeff, flags, T32)
    keep = (flags & 4) != 0
    assert J.shape == (int(keep.sum()), 6) and np.array_equal(b, coeff[keep, 3].astype(np.float64))
    pose = np.concatenate([T32[:3, 3].astype(np.float64), quat_of(T32[:3, :3].astype(np.float64))])
    h = 1e-5
    fd = np.zeros_like(J)
    for a in range(6):
        d = np.zeros(6)
        d[a] = h
        fd[:, a] = (E.residuals(pts, coeff, flags, pose, d) - E.residuals(pts, coeff, flags, pose, -d)) / (2 * h)
    scale = np.linalg.norm(coeff[keep, :3].astype(np.float64), axis=1) * (1.0 + 2.0 * np.linalg.norm(pts[keep, :3].astype(np.float64), axis=1))
    err = np.abs(J - fd).max(axis=1) / scale
    print("pose %d: largest |J - fd| / scale %.3g" % (k, err.max()))
    assert err.max() <= 8 * 2.0 ** -24 + 1e-8
    # the conventions the tolerance pins: a left-hand perturbation or a missing factor 2 is off by the size of the row
    wrong = np.abs(np.concatenate([J[:, :3], J[:, 3:] / 2.0], axis=1) - fd).max(axis=1) / scale
    assert np.median(wrong) > 1e-3


def test_exact_sums():
    pts, coeff, flags = problem(11, 300)
    T32 = np.eye(4, dtype=np.float32)
    T32[:3, :3] = rot_euler(0.4, 1.2, -0.8).astype(np.float32)
    r = E.exact_sums(pts, coeff, flags, T32, 100)
    J = r["J"]
    assert r["n_rows"] == len(J) == int(((flags & 4) != 0).sum())
    assert r["n_line"] == int(((flags[:100] & 2) != 0).sum()) and r["n_plane"] == int(((flags[100:] & 2) != 0).sum())
    assert np.array_equal(r["H"], r["H"].T)
    H = J.T @ J  # numpy's own order of summation: inside the bound
    assert (np.abs(H - r["H"]) <= E.sum_bound(r["n_rows"], r["absH"])).all()
    assert abs(float(r["b"] @ r["b"]) - r["sum_b2"]) <= E.sum_bound(r["n_rows"], r["abs_b2"])
    # exact: a sum whose rounded products cancel keeps the products' low parts
    a = np.array([1.0 + 2.0 ** -30, -(1.0 + 2.0 ** -30)])
    c = np.array([1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30])
    assert E.exact_dot(a, c) == 0.0
    assert E.exact_dot(np.array([1.0 + 2.0 ** -30, -1.0]), np.array([1.0 + 2.0 ** -30, 1.0 + 2.0 ** -29])) == 2.0 ** -60


ODOM = np.diag([0.8, 0.4, 0.8, 1.0, 2.0, 1.0])
LOOP = 2.0 * np.eye(6)


def test_policy():
    rng = np.random.default_rng(5)
    J = rng.normal(size=(400, 6))
    J[:, 2] = 0.0  # a direction the match does not observe
    H = J.T @ J
    for ref in (ODOM, LOOP):
        # H = 0: the reference's constant, positive definite
        O = E.edge_information(ref, np.zeros((6, 6)), 0.0, 0, 0.02)
        assert np.array_equal(O, ref) and np.linalg.eigvalsh(O).min() > 0
        O = E.edge_information(ref, np.zeros((6, 6)), 0.0, 400, 0.02)
        assert np.array_equal(O, ref)
        # fewer than 50 rows: the constant, whatever H says
        assert np.array_equal(E.edge_information(ref, H, 1.0, 49, 0.02), ref)
        assert not np.array_equal(E.edge_information(ref, H, 1.0, 50, 0.02), ref)
        # sums that are not finite (the reference's 0 / 0 for a point exactly on its line): the constant
        Hn = H.copy()
        Hn[0, 3] = Hn[3, 0] = np.nan
        assert np.array_equal(E.edge_information(ref, Hn, 1.0, 400, 0.02), ref)
        assert np.array_equal(E.edge_information(ref, H, np.inf, 400, 0.02), ref)
        # the floor: residuals below the sensor's noise do not make the edge more certain than the sensor
        lo = E.edge_information(ref, H, 1e-9, 400, 0.02)
        assert np.array_equal(lo, ref + H / (0.02 * 0.02))
        # above it the residual variance sum_b2 / (n_rows - 6) scales
        hi = E.edge_information(ref, H, 394 * 0.01, 400, 0.02)
        assert np.array_equal(hi, ref + H / (394 * 0.01 / 394.0)) and np.array_equal(hi, ref + H / 0.01)
        for O in (lo, hi):
            assert np.array_equal(O, O.T) and np.linalg.eigvalsh(O).min() > 0
            # the unobserved direction keeps exactly the reference's weight
            assert O[2, 2] == ref[2, 2] and not O[2, [0, 1, 3, 4, 5]].any()


def test_package_policy_is_the_reference(pkg):
    """graph.hessian_information and the reference: the same bits."""
    import importlib
    g = importlib.import_module("the-cooper-mapper_amd.graph")
    rng = np.random.default_rng(6)
    for n_rows, b2, sig in ((10, 1.0, 0.02), (49, 1.0, 0.02), (50, 1e-6, 0.02), (400, 3.0, 0.02), (4000, 0.5, 0.1)):
        J = rng.normal(size=(max(n_rows, 6), 6)) * rng.uniform(0.1, 50.0, 6)
        H = J.T @ J
        for ref in (g.ODOMETRY_INFORMATION, g.LOOP_INFORMATION):
            a, b = g.hessian_information(ref, H, b2, n_rows, sig), E.edge_information(ref, H, b2, n_rows, sig)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(g.ODOMETRY_INFORMATION, ODOM) and np.array_equal(g.LOOP_INFORMATION, LOOP)


def test_graph_options_are_validated(pkg):
    """Checked before anything touches the device."""
    import importlib
    g = importlib.import_module("the-cooper-mapper_amd.graph")
    with pytest.raises(ValueError, match="range_sigma"):
        g.Graph(resident=True, edge_information="hessian")
    with pytest.raises(ValueError, match="resident"):
        g.Graph(edge_information="hessian", range_sigma=0.02)
    with pytest.raises(ValueError):
        g.Graph(edge_information="identity")
