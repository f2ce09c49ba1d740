"""Shared by tests/test_oracle_posegraph_c.py (CPU) and tests/test_gpu_posegraph_se3.py (GPU): the general SE(3) graph
cases of oracle/posegraph_oracle.make_graph_se3, the two CPU references' systems in one layout, and the MEASURED floors of
the references that every tolerance of the GPU tests is derived from.  Nothing here was calibrated against the GPU: the CPU
tests assert that the references stay inside these figures, the GPU tests use ten times them.

Measured (gcc -O3 with and without FMA contraction, ten seeds, sizes 2 .. 400, eight edge permutations each):
  summation-order spread of posegraph_oracle.c against itself with its edges permuted
      diagonal blocks 4.1e-16 max|diag|, off-diagonal blocks 2.2e-16 max|off|, b 4.2e-16 max|b|, chi2 3.2e-15 chi2
      (the same file compiled with -ffp-contract=off against =fast differs from itself by 4.6e-16 / 4.1e-16 / 3.1e-16: FMA
      contraction moves the reference no further than the order of its sums does)
  posegraph_oracle.c (analytic Jacobians) against posegraph_oracle.py (central differences, h = 1e-6)
      H 1.8e-10 max|H|, b 3.1e-10 max|b|, chi2 6.6e-15 chi2; the difference is the finite-difference error of the numpy
      oracle: its Jacobians move by 3.4e-10 of their scale between h and h / 2
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import posegraph_oracle as po  # noqa: E402
import posegraph_oracle_c as pc  # noqa: E402

# ---- the references' own floors (relative; see the module docstring) -------------------------------------------------------
SPREAD_H = 4.5e-16     # C oracle, edges permuted: diagonal blocks / max|diag|, off-diagonal blocks / max|off|
SPREAD_B = 4.5e-16     # ... b / max|b|
SPREAD_CHI2 = 3.5e-15  # ... chi2
O2O_H = 2.0e-10        # C oracle against numpy oracle: H / max|H|
O2O_B = 3.5e-10        # ... b / max|b|
O2O_CHI2 = 1.0e-14     # ... chi2
FD_REL = 5e-10         # numeric_jacobians(h) against (h / 2), relative to the largest Jacobian entry
PCG_TOL = 1e-8         # relative residual at which the library's PCG stops (lslam_pg_set_solve_tolerance default)

# ---- cases: (n, n_extra, seed, fixed, isolated) -----------------------------------------------------------------------------
def _fixed_set(n):
    return sorted({0, n // 2, n - 1})


LIN_CASES = [(n, nx, seed, f, iso)
             for (n, nx, seed, iso) in ((2, 1, 0, False), (3, 2, 1, False), (7, 6, 2, False), (7, 6, 3, True), (64, 100, 4, False),
                                        (65, 100, 5, True), (400, 600, 6, False))
             for f in _fixed_set(n)]


def graph(case, **kw):
    n, nx, seed, fixed, iso = case
    return po.make_graph_se3(n, nx, seed, fixed=fixed, isolated=iso, **kw)


def pairs_of(ij):
    """distinct (min, max) vertex pairs of the edges, sorted: one off-diagonal block each"""
    return np.array(sorted({(min(a, b), max(a, b)) for a, b in np.asarray(ij).tolist()}), np.int32).reshape(-1, 2)


def raw_edge_quaternion_w(g, poses=None):
    """w of q_e = qz* (x) qi* (x) qj before normalisation and sign choice: negative = the sgn = -1 branch"""
    p = g["init"] if poses is None else poses
    E = po.pose_mul(po.pose_inv(g["meas"]), po.pose_mul(po.pose_inv(p[g["ij"][:, 0]]), p[g["ij"][:, 1]]))
    return E[:, 6]


def c_system(g, poses=None, order=None):
    """The C oracle's block system at `poses` (default: the initial estimate), edges taken in `order`."""
    p = g["init"] if poses is None else poses
    o = np.arange(len(g["ij"])) if order is None else order
    pr = pairs_of(g["ij"])
    diag, b, c2 = pc.linearize(p, g["ij"][o], g["meas"][o], g["info"][o], fixed=g["fixed"])
    off = pc.offdiag_blocks(p, g["ij"][o], g["meas"][o], g["info"][o], pr, fixed=g["fixed"])
    return dict(diag=diag, off=off, off_ij=pr, b=b, chi2=c2)


def np_system(g, poses=None):
    """The numpy oracle's system in the same layout (fixed vertex: identity block, zero rhs, zero off-diagonal blocks)."""
    p = g["init"] if poses is None else poses
    H, b, c2 = po.linearize(p, g["ij"], g["meas"], g["info"])
    Hd = H.toarray()
    f = slice(6 * g["fixed"], 6 * g["fixed"] + 6)
    Hd[f, :] = 0.0
    Hd[:, f] = 0.0
    Hd[f, f] = np.eye(6)
    b = b.copy()
    b[f] = 0.0
    n = len(p)
    pr = pairs_of(g["ij"])
    diag = np.stack([Hd[6 * v:6 * v + 6, 6 * v:6 * v + 6] for v in range(n)])
    off = np.stack([Hd[6 * a:6 * a + 6, 6 * c:6 * c + 6] for a, c in pr]) if len(pr) else np.zeros((0, 6, 6))
    return dict(diag=diag, off=off, off_ij=pr, b=b, chi2=c2, H=H)


def differences(got, ref):
    """Largest differences of two systems in the same block order, each relative to the reference's own scale:
    diag / max|diag|, off / max|off|, both / max|H| (`h`), b / max|b|, chi2 / chi2."""
    assert np.array_equal(got["off_ij"], ref["off_ij"])
    sd = np.abs(ref["diag"]).max()
    so = max(np.abs(ref["off"]).max() if ref["off"].size else 0.0, 1e-300)
    dd = np.abs(got["diag"] - ref["diag"]).max()
    do = np.abs(got["off"] - ref["off"]).max() if ref["off"].size else 0.0
    return dict(diag=dd / sd, off=do / so, h=max(dd, do) / max(sd, so), b=np.abs(got["b"] - ref["b"]).max() / np.abs(ref["b"]).max(),
                chi2=abs(got["chi2"] - ref["chi2"]) / ref["chi2"])


def dense_free_matrix(sysd, lam, fixed):
    """(H + lam I) of a block system over the free unknowns, dense, and their indices."""
    n = len(sysd["diag"])
    A = np.zeros((6 * n, 6 * n))
    for v in range(n):
        A[6 * v:6 * v + 6, 6 * v:6 * v + 6] = sysd["diag"][v]
    for (a, c), blk in zip(sysd["off_ij"], sysd["off"]):
        A[6 * a:6 * a + 6, 6 * c:6 * c + 6] = blk
        A[6 * c:6 * c + 6, 6 * a:6 * a + 6] = blk.T
    idx = np.r_[0:6 * fixed, 6 * fixed + 6:6 * n]
    return A[np.ix_(idx, idx)] + lam * np.eye(len(idx)), idx


# ---- LM runs ------------------------------------------------------------------------------------------------------------------
LM_N, LM_EXTRA = 40, 60
LM_START = dict(mild=(0.3, 0.05), gross=(3.0, 0.6))  # (m, quaternion vector) standard deviation of the initial perturbation
# (start, seed, fixed, iterations compared).  Chosen on the CPU: both oracles take the same trials in every one of these
# iterations, and the prefix ends before chi2 stops falling by more than 1e-9 of itself per iteration (decisions on a flat chi2
# are rounding noise).  Trials per iteration, |dq| > 1 updates:
#   mild  0: nine single trials, none        mild 1: six single trials, none        mild 5: nine single trials, none
#   gross 1: [1 x9, 4, 1 x6] (three rejected trials), 26 clamped updates           gross 2: fourteen single trials, 14 clamped
LM_CASES = [("mild", 0, 0, 9), ("mild", 1, 20, 6), ("mild", 5, 39, 9), ("gross", 1, 20, 16), ("gross", 2, 39, 14)]


def lm_graph(start, seed, fixed):
    return po.make_graph_se3(LM_N, LM_EXTRA, seed, fixed=fixed, init_sigma=LM_START[start])


def lm_references(g, iters):
    """Both CPU oracles over `iters` LM iterations -> dict: poses of each, the per-iteration trial counts of each (the C
    oracle's from runs of 1 .. iters iterations: it reports totals), chi2 per iteration (numpy), clamped |dq| > 1 updates,
    the path length sum of max|dx| over the accepted steps, and the poses' and the final chi2's spread under the PCG stopping rule -- the numpy LM
    repeated with every damped solve replaced by A^-1 (b + r), |r| = PCG_TOL |b|, r random: what a solver that stops at that
    residual may return."""
    a = (g["init"], g["ij"], g["meas"], g["info"])
    fixed = g["fixed"]
    path = []
    po.dq_clamped = 0
    P, hist = po.optimize(*a, fixed=fixed, max_iters=iters, on_trial=lambda H, b, lam, dx, acc: path.append(np.abs(dx).max() if acc else 0.0))
    clamped = po.dq_clamped
    cum = []
    for k in range(1, iters + 1):
        out, st = pc.optimize(*a, fixed=fixed, max_iters=k)
        cum.append(st.trials)
    exact = po.solve_damped
    spread, chi_spread, same = 0.0, 0.0, True
    try:
        for rep in range(3):
            rng = np.random.default_rng(rep)

            def stopped_early(H, b, lam, fx):
                r = rng.normal(size=len(b))
                r[6 * fx:6 * fx + 6] = 0.0
                return exact(H, b + r * (PCG_TOL * np.linalg.norm(b) / np.linalg.norm(r)), lam, fx)
            po.solve_damped = stopped_early
            P2, h2 = po.optimize(*a, fixed=fixed, max_iters=iters)
            same = same and [h["trials"] for h in h2] == [h["trials"] for h in hist]
            spread = max(spread, float(np.abs(P2 - P).max()))
            chi_spread = max(chi_spread, abs(h2[-1]["chi2"] - hist[-1]["chi2"]) / hist[-1]["chi2"])
    finally:
        po.solve_damped = exact
    return dict(np_poses=P, c_poses=out, c_stats=st, np_trials=[h["trials"] for h in hist], c_trials=list(np.diff([0] + cum)),
                chi2=[po.chi2(*a)] + [h["chi2"] for h in hist], clamped=clamped, path=float(sum(path)), pcg_spread=spread, pcg_chi2_spread=chi_spread,
                pcg_same_trials=same)
