"""The numpy reference of the marginal-covariance tests (tests/marginals_ref.py) held to a result worked out by hand, and to
its own finite-difference error.  CPU only."""
import numpy as np

import marginals_ref as mr
import posegraph_se3 as se3

po = se3.po


def _three_chain(seed):
    """0 - 1 - 2, vertex 0 fixed, random SE(3) poses, DIAGONAL information, measurements equal to the estimate's relative poses
    (zero error: the edge covariance is then exactly the inverse information in the relative pose's right increment)."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(3, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([rng.uniform(-1.0, 1.0, (3, 3)), q], 1)
    ij = np.array([[0, 1], [1, 2]], np.int32)
    meas = po.pose_mul(po.pose_inv(poses[ij[:, 0]]), poses[ij[:, 1]])
    info = np.stack([np.diag(rng.uniform(1.0, 4.0, 6)) for _ in range(2)])
    return dict(init=poses, ij=ij, meas=meas, info=info, fixed=0)


def test_relative_covariance_of_a_three_chain_is_the_propagated_sum():
    """Sigma_rel(0, 2) = Ad Sigma_01 Ad^T + Sigma_12 with Sigma_e = Omega_e^-1 and Ad = adjoint_right(T_12): the first edge's
    noise acts before T_12, the second's after it.  To 1e-12 of the largest entry (figures printed: up to 1.5e-13)."""
    for seed in range(4):
        g = _three_chain(seed)
        H, S = mr.covariance(se3.c_system(g), g["fixed"])  # the C oracle's system: analytic Jacobians
        got, J = mr.relative_covariance(S, g["init"], 0, [2, 0, 1])
        Ad = mr.adjoint_right(g["meas"][1])
        want02 = Ad @ np.linalg.inv(g["info"][0]) @ Ad.T + np.linalg.inv(g["info"][1])
        want01 = np.linalg.inv(g["info"][0])
        d02 = np.abs(got[0] - want02).max() / np.abs(want02).max()
        d01 = np.abs(got[2] - want01).max() / np.abs(want01).max()
        print("seed %d: Sigma_rel(0,2) off by %.2e, Sigma_rel(0,1) by %.2e of the largest entry" % (seed, d02, d01))
        assert d02 <= 1e-12 and d01 <= 1e-12
        assert np.array_equal(got[1], np.zeros((6, 6)))  # j == ref


def test_relative_covariance_does_not_depend_on_which_vertex_is_fixed():
    """With 1 fixed instead of 0 the relative covariance of (0, 2) is the same: a relative pose does not see the gauge.  With 1
    fixed J_ref takes part, and with it the finite-difference error: the bound is relative_bound's at tol = 0 for both sides."""
    g = _three_chain(7)
    H0, S0 = mr.covariance(se3.c_system(g), 0)
    a, J = mr.relative_covariance(S0, g["init"], 0, [2])
    g1 = dict(g, fixed=1)
    H1, S1 = mr.covariance(se3.c_system(g1), 1)
    b, _ = mr.relative_covariance(S1, g["init"], 0, [2])
    d = np.linalg.norm(a - b)
    bound = mr.relative_bound(H0, S0, J[0], 0.0) + mr.relative_bound(H1, S1, J[0], 0.0)
    print("fixed 0 against fixed 1: %.2e (bound %.2e, |Sigma_rel| %.2e)" % (d, bound, np.linalg.norm(a)))
    assert d <= bound


def test_finite_difference_jacobians_stay_inside_their_own_error():
    """relative_jacobians at h against h / 2 on general graphs: inside FD_REL of the largest entry; and at zero error J_j = I."""
    worst = 0.0
    for seed in range(6):
        g = mr.make_chain(12, seed)
        js = np.arange(12)
        J1 = mr.relative_jacobians(g["init"], 5, js)
        J2 = mr.relative_jacobians(g["init"], 5, js, h=mr.FD_H / 2)
        worst = max(worst, np.abs(J1 - J2).max() / np.abs(J1).max())
        assert np.abs(J1[:, :, 6:] - np.eye(6)).max() <= 1e-10
    print("h against h / 2: %.2e of the largest entry (FD_REL %.1e)" % (worst, mr.FD_REL))
    assert worst <= mr.FD_REL


def test_column_bound_covers_a_perturbed_solve():
    """A column with residual exactly tol |e| is inside the bound (the inequality the GPU tests rely on)."""
    g = mr.make_chain(22, 3, n_loops=3)
    H, S = mr.covariance(se3.np_system(g), 0)
    rng = np.random.default_rng(0)
    tol = 1e-8
    for c in (6, 40, 131):
        r = rng.normal(size=len(H))
        r[:6] = 0.0
        x = np.linalg.solve(H, np.eye(len(H))[:, c] + r * (tol / np.linalg.norm(r)))
        assert np.linalg.norm(x - S[:, c]) <= mr.column_bound(H, S, tol)
