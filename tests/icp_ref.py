"""Plain references of the coarse alignment (lslam_icp_align, csrc/lslam_icp.hip: PCL's IterativeClosestPoint with its
defaults) and the input families its kernel and host fit are held to them on.  numpy only: nothing here imports the library
under test, its kd-tree or oracle/icp_oracle.py (cKDTree, all float64: the second, looser yardstick).

TEST INFRASTRUCTURE: imported by tests/test_icp_ref.py (CPU) and tests/test_gpu_icp_general.py.

  ref_step      one iteration: the float32 transform with the kernel's association, every source-target squared distance by
                brute force in float32, argmin, the gate, the 17 sums EXACT (products of two float32 values are exact in
                float64; math.fsum), each sum's majorant, and the rigid fit in float64 on the CENTRED cross-covariance
  ref_align     the loop over ref_step with DefaultConvergenceCriteria as the header of lslam_icp.hip states it
  fit_jacobi    the second float64 formulation of the fit (uncentred sums minus n cs ct^T, one-sided Jacobi), for the fit bar
  compare_step / compare_align   the comparisons the GPU tests make, as functions returning the list of what failed -- the CPU
                suite runs them on mutated references to show that each seeded mutation is seen
  cases()       the input families

`variant` applies one of the seeded mutations to a COPY of the reference's steps (never to a kernel).
"""
import math

import numpy as np

import scanmatch_ref as SR

F32 = np.float32
U53 = 2.0 ** -53
DBL_MAX = float(np.finfo(np.float64).max)

VARIANTS = ("H_transposed", "no_det_fix", "compose_right", "t_is_ct_minus_cs", "gate_lt", "gated_in_centroids",
            "drop_last_block", "drop_last_wave", "minus1_reads_point0", "d2_before_gate")


# ---------------------------------------------------------------------------
# one iteration
# ---------------------------------------------------------------------------
def transform32(T, src):
    """pcl::transformPointCloud in float32 with the kernel's association, no FMA: ((R0 x + R1 y) + R2 z) + t."""
    T = np.asarray(T, F32).reshape(4, 4)
    s = np.asarray(src, F32)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    out = np.empty((len(s), 3), F32)
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def gate_d2(gate):
    """The squared gate as the library rounds it: float32 of the float64 square; None / <= 0: no gate."""
    if gate is None or not gate > 0.0:
        return F32(np.finfo(F32).max)
    return F32(float(gate) * float(gate))


def nearest32(tgt, p):
    """Brute force: for every p the float32 squared distance (dx dx + dy dy) + dz dz to every target point.
    -> d2 (n,) float32 the minimum, idx (n,) the first minimiser, mins: list of arrays of all minimisers, tie (n,) bool:
    minimisers with DIFFERENT coordinates exist (which one a tree returns is its visit order)."""
    t = np.asarray(tgt, F32)[:, :3]
    n = len(p)
    d2, idx, mins, tie = np.zeros(n, F32), np.zeros(n, np.int64), [], np.zeros(n, bool)
    for i in range(n):
        d = t - p[i][None, :]
        sq = d * d
        dd = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        assert dd.dtype == F32
        k = int(np.argmin(dd))
        at = np.flatnonzero(dd == dd[k])
        d2[i], idx[i] = dd[k], k
        mins.append(at)
        tie[i] = len(at) > 1 and len(np.unique(t[at], axis=0)) > 1
    return d2, idx, mins, tie


def fit_centred(s, q, variant=None):
    """TransformationEstimationSVD in float64: centroids, H = sum (s - cs)(q - ct)^T, numpy's SVD,
    R = V diag(1, 1, det(V U^T)) U^T, t = ct - R cs.  -> dict(R, t, W, det_sign, cs, ct, H)."""
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    cs, ct = s.mean(0), q.mean(0)
    H = (s - cs).T @ (q - ct)
    if variant == "H_transposed":
        H = H.T
    U, W, Vt = np.linalg.svd(H)
    V = Vt.T
    sign = -1 if np.linalg.det(V @ U.T) < 0 else 1
    R = V @ np.diag([1.0, 1.0, 1.0 if variant == "no_det_fix" else float(sign)]) @ U.T
    t = ct - cs if variant == "t_is_ct_minus_cs" else ct - R @ cs
    return dict(R=R, t=t, W=W, det_sign=sign, cs=cs, ct=ct, H=H)


def objective(R, t, s, q):
    """sum |R s + t - q|^2 in float64, evaluated about the centroids -- r = R (s - cs) - (q - ct) + (R cs + t - ct) -- so that
    its own rounding is relative to the clouds' extent and not to their distance from the origin."""
    s, q, R = np.asarray(s, np.float64), np.asarray(q, np.float64), np.asarray(R, np.float64)
    cs, ct = s.mean(0), q.mean(0)
    r = (s - cs) @ R.T - (q - ct) + (R @ cs + np.asarray(t, np.float64) - ct)
    return math.fsum((r * r).ravel())


def objective_scale(s, q):
    """sum |s - cs|^2 + sum |q - ct|^2: the size of the terms the objective is the difference of (its value at R = 0)."""
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    return float(((s - s.mean(0)) ** 2).sum() + ((q - q.mean(0)) ** 2).sum())


def ref_step(target, source, T, gate=None, variant=None, search=None):
    """One iteration at T (4x4, rounded to float32); search: the `search` entry of an earlier call on the same clouds and T (the
    brute-force part, which no mutation touches).  -> dict:
      p (m, 3) float32 transformed source        d2 (m,) float32 nearest squared distance
      nn (m,) nearest target index               mins / tie        all minimisers / a tie between different coordinates
      pair (m,) nn where kept, -1 where gated out                   keep (m,) bool
      terms (k, 17) float64: the exact terms of the 17 sums, one row per contributing point
      sums (18,) the exactly rounded sums (pad 0)                   maj (18,) sum |term|
      n                                          fit: fit_centred of the kept pairs + obj_min, or None when n < 3"""
    tgt = np.asarray(target, F32)[:, :3]
    src = np.asarray(source, F32)[:, :3]
    m = len(src)
    if search is None:
        p = transform32(T, src)
        search = (p,) + nearest32(tgt, p)
    p, d2, nn, mins, tie = search
    g2 = gate_d2(gate)
    keep = d2 < g2 if variant == "gate_lt" else d2 <= g2
    live = np.ones(m, bool)  # the lanes a mutated reduction still adds
    if variant == "drop_last_block":
        live[(m // 128) * 128:] = False
    if variant == "drop_last_wave":
        live[(m // 64) * 64:] = False
    pair = np.where(keep, nn, -1)
    q_idx = nn.copy()
    rows = keep & live
    if variant == "minus1_reads_point0":  # a gated-out point enters the sums paired with target point 0
        q_idx = np.where(keep, nn, 0)
        rows = live.copy()
    P, Q = p.astype(np.float64), tgt[q_idx].astype(np.float64) if m else np.zeros((0, 3))
    terms = np.zeros((m, 17))
    terms[:, 0] = 1.0
    terms[:, 1] = d2.astype(np.float64)
    terms[:, 2:5], terms[:, 5:8] = P, Q
    terms[:, 8:17] = (P[:, :, None] * Q[:, None, :]).reshape(m, 9)  # exact: 24-bit x 24-bit significands
    w = np.repeat(rows[:, None], 17, axis=1)
    if variant == "gated_in_centroids":
        w[:, 2:8] = live[:, None]
    if variant == "d2_before_gate":
        w[:, 1] = live
    tw = np.where(w, terms, 0.0)
    sums, maj = np.zeros(18), np.zeros(18)
    for k in range(17):
        sums[k] = math.fsum(tw[:, k])
        maj[k] = math.fsum(np.abs(tw[:, k]))
    n = int(sums[0])
    fit = None
    if n >= 3:
        s, q = P[rows], Q[rows]
        if variant in ("gated_in_centroids",):  # the mutated centroids reach the fit through the sums
            fit = fit_from_sums(sums, variant)
        else:
            fit = fit_centred(s, q, variant)
        fit["obj_min"] = objective(fit["R"], fit["t"], s, q) if variant is None else None
        fit["s"], fit["q"] = s, q
    return dict(p=p, d2=d2, nn=nn, mins=mins, tie=tie, pair=pair, keep=keep, terms=tw, sums=sums, maj=maj, n=n, fit=fit, m=m,
                search=search)


def fit_from_sums(sums, variant=None):
    """The centred fit restated on 18 sums (only where a mutation acts on the sums themselves)."""
    n = sums[0]
    cs, ct = sums[2:5] / n, sums[5:8] / n
    H = sums[8:17].reshape(3, 3) - n * np.outer(cs, ct)
    U, W, Vt = np.linalg.svd(H)
    V = Vt.T
    sign = -1 if np.linalg.det(V @ U.T) < 0 else 1
    R = V @ np.diag([1.0, 1.0, float(sign)]) @ U.T
    return dict(R=R, t=ct - R @ cs, W=W, det_sign=sign, cs=cs, ct=ct, H=H)


# ---------------------------------------------------------------------------
# the second formulation of the fit: uncentred sums, one-sided Jacobi
# ---------------------------------------------------------------------------
def svd_jacobi(A):
    """One-sided (Hestenes) Jacobi SVD of a 3x3 float64 matrix, A = U diag(W) V^T, W descending; columns of U that belong to a
    vanishing singular value are completed to an orthonormal basis."""
    B = np.array(A, np.float64)
    V = np.eye(3)
    for _ in range(80):
        rotated = False
        for i, j in ((0, 1), (0, 2), (1, 2)):
            a, b, g = B[:, i] @ B[:, i], B[:, j] @ B[:, j], B[:, i] @ B[:, j]
            if g == 0.0 or abs(g) <= 1e-17 * math.sqrt(a * b):
                continue
            rotated = True
            zeta = (b - a) / (2.0 * g)
            tn = math.copysign(1.0, zeta) / (abs(zeta) + math.hypot(1.0, zeta))
            c = 1.0 / math.hypot(1.0, tn)
            s = c * tn
            G = np.array([[c, s], [-s, c]])
            B[:, (i, j)] = B[:, (i, j)] @ G
            V[:, (i, j)] = V[:, (i, j)] @ G
        if not rotated:
            break
    W = np.linalg.norm(B, axis=0)
    order = np.argsort(-W, kind="stable")
    B, V, W = B[:, order], V[:, order], W[order]
    U = np.zeros((3, 3))
    have = []
    for j in range(3):
        if W[j] > 1e-300:
            U[:, j] = B[:, j] / W[j]
            have.append(j)
    for j in range(3):  # Gram-Schmidt against the unit axes for what is missing
        if j in have:
            continue
        best = None
        for e in np.eye(3):
            v = e - sum((U[:, k] @ e) * U[:, k] for k in have)
            if best is None or np.linalg.norm(v) > np.linalg.norm(best):
                best = v
        U[:, j] = best / np.linalg.norm(best)
        have.append(j)
    return U, W, V


def fit_jacobi(sums):
    """The fit from the 18 sums as an implementation on a device's output has to make it: cs, ct = sums / n,
    H = sum s t^T - n cs ct^T, Jacobi SVD, det fix.  -> dict(R, t, W, det_sign)."""
    sums = np.asarray(sums, np.float64)
    n = sums[0]
    cs, ct = sums[2:5] / n, sums[5:8] / n
    H = sums[8:17].reshape(3, 3) - n * np.outer(cs, ct)
    U, W, V = svd_jacobi(H)
    sign = -1 if np.linalg.det(V @ U.T) < 0 else 1
    R = V @ np.diag([1.0, 1.0, float(sign)]) @ U.T
    return dict(R=R, t=ct - R @ cs, W=W, det_sign=sign, H=H)


def sums_bound(n, maj):
    """|any fp64 summation of n terms - exact| <= (n - 1) 2^-53 sum |term| (first order; every order of summation)."""
    return max(n - 1, 0) * U53 * np.asarray(maj, np.float64)


def objective_spread(ref):
    """The rank-deficient counterpart of fit_spread: |objective of the Jacobi formulation's (R, t) - the centred fit's minimum|
    over objective_scale."""
    f = ref["fit"]
    j = fit_jacobi(ref["sums"])
    return abs(objective(j["R"], j["t"], f["s"], f["q"]) - f["obj_min"]) / objective_scale(f["s"], f["q"])


def fit_spread(ref, rng, trials=4):
    """How far float64 formulations of one fit lie apart: centred + numpy's SVD (ref['fit']) against uncentred sums + Jacobi,
    and against the same with every entry of sum s t^T (hence of H) moved by its derived bound, random signs.  -> (spread in R, spread in t)."""
    f = ref["fit"]
    dR = dt = 0.0
    b = sums_bound(ref["n"], ref["maj"])
    for k in range(trials + 1):
        sums = ref["sums"].copy()
        if k:
            sums[8:17] += rng.choice((-1.0, 1.0), 9) * b[8:17]
        j = fit_jacobi(sums)
        dR = max(dR, np.abs(j["R"] - f["R"]).max())
        dt = max(dt, np.abs(j["t"] - f["t"]).max())
    return dR, dt


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
def compose(R, t, T):
    """[R | t] T in float64 with the host's association: (R0 T0c + R1 T1c) + R2 T2c, then + t on the last column."""
    R, t, T = np.asarray(R, np.float64), np.asarray(t, np.float64), np.asarray(T, np.float64).reshape(4, 4)
    out = np.eye(4)
    for r in range(3):
        for c in range(4):
            out[r, c] = (R[r, 0] * T[0, c] + R[r, 1] * T[1, c]) + R[r, 2] * T[2, c]
        out[r, 3] += t[r]
    return out


def ref_align(target, source, guess, max_iterations=10, transformation_epsilon=0.0, gate=None, variant=None):
    """The whole alignment: -> dict(T float64 4x4 (the library returns its float32 rounding), converged, iterations, fitness,
    trace: per iteration (mse, |mse - prev|, |mse - prev| / prev)).  The running transform is kept in float64 and rounded to
    float32 for every step, as the device rounds it when it fills the kernel's arguments."""
    T = np.asarray(guess, F32).reshape(4, 4).astype(np.float64)
    trace = []
    if len(target) == 0:
        return dict(T=T, converged=False, iterations=0, fitness=0.0, trace=trace)
    max_it = max_iterations if max_iterations > 0 else 10
    prev, it, converged = DBL_MAX, 0, False
    while True:
        st = ref_step(target, source, T.astype(F32), gate, variant)
        if st["n"] < 3:
            break
        f = st["fit"]
        if variant == "compose_right":
            inc = np.eye(4)
            inc[:3, :3], inc[:3, 3] = f["R"], f["t"]
            T = T @ inc
        else:
            T = compose(f["R"], f["t"], T)
        it += 1
        mse = st["sums"][1] / st["n"]
        trace.append((mse, abs(mse - prev), abs(mse - prev) / prev if prev > 0 else math.inf))
        if it >= max_it:
            converged = True
            break
        if 0.5 * (np.trace(f["R"]) - 1.0) >= 1.0 - transformation_epsilon and float(f["t"] @ f["t"]) <= transformation_epsilon:
            converged = True
            break
        if abs(mse - prev) < 1e-12 or abs(mse - prev) / prev < 1e-5:
            converged = True
            break
        prev = mse
    last = ref_step(target, source, T.astype(F32), gate, variant)
    fitness = last["sums"][1] / last["n"] if last["n"] > 0 else DBL_MAX
    return dict(T=T, converged=converged, iterations=it, fitness=fitness, trace=trace)


# ---------------------------------------------------------------------------
# the comparisons of the GPU tests
# ---------------------------------------------------------------------------
def as_device(ref):
    """A reference step (mutated or not) in the shape of the tap's output."""
    f = ref["fit"]
    out = dict(idx=ref["pair"].astype(np.int32), d2=ref["d2"], sums=ref["sums"].copy(), fitted=f is not None)
    if f is not None:
        out.update(R=f["R"], t=f["t"], W=f["W"], det_sign=f["det_sign"])
    return out


def sum_errors(dev_sums, ref):
    """|device sum - exact sum| per entry, the subtraction exact too (fsum over the terms and the negated device value)."""
    return np.array([abs(math.fsum(list(ref["terms"][:, k]) + [-float(dev_sums[k])])) for k in range(17)])


# below this W2 / W0 the third singular vectors are rounding noise and so is the sign of det(V U^T) (the fix makes R the same)
DET_MEANINGFUL = 1e-9
RIGID_TOL = 1e-12   # orthonormality of a float64 R on the rank-deficient families (issue)


def compare_step(dev, ref, bar_R, bar_t, degenerate=False):
    """The step-level comparisons: index, distance, count, sums, fit.  dev: the tap's dict (or as_device of a reference);
    ref: ref_step's.  -> list of the comparisons that failed (empty: the step agrees)."""
    bad = []
    idx = np.asarray(dev["idx"])
    for i in range(ref["m"]):
        want = ref["pair"][i]
        if want < 0 and idx[i] != -1:
            bad.append("index %d: %d, gated out in the reference" % (i, idx[i]))
        elif want >= 0 and idx[i] not in ref["mins"][i]:
            bad.append("index %d: %d, reference %d" % (i, idx[i], want))
    if not np.array_equal(np.asarray(dev["d2"], F32).view(np.uint32), ref["d2"].view(np.uint32)):
        bad.append("d2 bits")
    if dev["sums"][0] != ref["n"]:
        bad.append("n %r, reference %d" % (dev["sums"][0], ref["n"]))
    err, bound = sum_errors(dev["sums"], ref), sums_bound(ref["n"], ref["maj"])
    for k in range(1, 17):
        if not err[k] <= bound[k]:
            bad.append("sum %d: off by %.3g > bound %.3g" % (k, err[k], bound[k]))
    if dev["sums"][17] != 0.0:
        bad.append("pad")
    f = ref["fit"]
    if bool(dev["fitted"]) != (f is not None):
        bad.append("fitted")
    elif f is not None:
        R, t = np.asarray(dev["R"], np.float64).reshape(3, 3), np.asarray(dev["t"], np.float64)
        if not degenerate:
            if not np.abs(R - f["R"]).max() <= bar_R:
                bad.append("R off by %.3g > %.3g" % (np.abs(R - f["R"]).max(), bar_R))
            if not np.abs(t - f["t"]).max() <= bar_t:
                bad.append("t off by %.3g > %.3g" % (np.abs(t - f["t"]).max(), bar_t))
            if f["W"][2] > DET_MEANINGFUL * f["W"][0] and dev["det_sign"] != f["det_sign"]:
                bad.append("det sign")
        else:
            bad += rigid_fit_failures(R, t, f["s"], f["q"], f["obj_min"], bar_R)
    return bad


def rigid_fit_failures(R, t, s, q, obj_min, bar):
    """Where R is not unique (rank-deficient H): R orthonormal to 1e-12 with det +1, t = ct - R cs, and the objective it
    reaches within bar x objective_scale of the reference's minimum (which is unique where R is not)."""
    bad = []
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return ["not finite"]
    if not np.abs(R @ R.T - np.eye(3)).max() <= RIGID_TOL:
        bad.append("R R^T - I = %.3g" % np.abs(R @ R.T - np.eye(3)).max())
    if not abs(np.linalg.det(R) - 1.0) <= 3 * RIGID_TOL:
        bad.append("det R = %r" % np.linalg.det(R))
    cs, ct = s.mean(0), q.mean(0)
    scale_t = np.abs(ct).max() + np.abs(cs).sum() + 1.0
    if not np.abs(t - (ct - R @ cs)).max() <= RIGID_TOL * scale_t:
        bad.append("t != ct - R cs by %.3g" % np.abs(t - (ct - R @ cs)).max())
    obj = objective(R, t, s, q)
    if not abs(obj - obj_min) <= bar * objective_scale(s, q) + 1e-300:
        bad.append("objective %.17g, minimum %.17g" % (obj, obj_min))
    return bad


def align_tolerance(T_ref, iterations, bar_R, bar_t):
    """Per-entry distance allowed between a float32 transform of the library and ref_align's float64 one after `iterations`
    compositions: the fit bar per iteration (an increment's R error reaches the translation through the running translation)
    plus one float32 rounding."""
    T_ref = np.asarray(T_ref, np.float64)
    tol = np.zeros((4, 4))
    its = max(iterations, 1)
    tol[:3, :3] = its * bar_R + 2.0 ** -23 * np.abs(T_ref[:3, :3])
    tol[:3, 3] = its * (bar_t + bar_R * np.abs(T_ref[:3, 3]).sum()) + 2.0 ** -23 * np.abs(T_ref[:3, 3])
    return tol


def compare_align(T, converged, iterations, ref, bar_R, bar_t):
    """The whole-loop comparisons: iteration count and converged flag exact, the transform within align_tolerance."""
    bad = []
    if iterations != ref["iterations"]:
        bad.append("iterations %d, reference %d" % (iterations, ref["iterations"]))
    if bool(converged) != ref["converged"]:
        bad.append("converged")
    d = np.abs(np.asarray(T, np.float64).reshape(4, 4) - ref["T"])
    if not (d <= align_tolerance(ref["T"], ref["iterations"], bar_R, bar_t)).all():
        bad.append("T off by %.3g (rotation) %.3g (translation)" % (d[:3, :3].max(), d[:3, 3].max()))
    return bad


# ---------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------
BASE_ANGLES = (0.4, -0.3, 2.5)            # the room's orientation in the target frame (roll, pitch, yaw)
BASE_OFFSET = (340.0, 175.0, 3.0)         # and where it stands
PLANE_OFFSET = (34.0, -17.5, 3.0)         # the tilted plane's place
STEP_ANGLES = (0.43, -0.325, 2.535)       # the guess: 2 - 3 degrees off the truth ...
STEP_SHIFT = (0.2, -0.2, 0.1)             # ... and 0.3 m
POSE_NAMES = SR.FAMILY_NAMES
SOURCE_SIZES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 321)
TARGET_SIZES = (1, 2, 3, 4, 5, 6, 11, 1600)
STRIDES = (12, 16, 32)
SEED = 11
# the three general poses whole loops start from (and the deep target's): those whose reference loop takes every convergence
# decision away from its thresholds (tests/test_icp_ref.py asserts it for each)
LOOP_POSES = ("rand1", "rand2", "yaw_pi")
DEEP_POSE = 2  # rand1


def _room(rng, n):
    import test_icp
    return test_icp._room(rng, n)


def _cloud4(xyz):
    out = np.zeros((len(xyz), 4), F32)
    out[:, :3] = np.asarray(xyz, np.float64).astype(F32)
    return out


def _T(Rm, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, t
    return T.astype(F32)


def pose_angles(seed=3):
    """The seven rotations of scanmatch_ref.general_pose_family, with STEP_ANGLES as the initial pose."""
    rng = np.random.default_rng(seed)
    init = np.array(STEP_ANGLES)
    out = [init]
    for _ in range(4):
        roll, pitch = rng.uniform(-1.3, 1.3, 2)
        out.append(np.array([roll, pitch, rng.uniform(-np.pi, np.pi)]))
    out.append(np.array([init[0], init[1], np.pi - 1e-3]))
    out.append(np.array([init[0], np.pi / 2 - 0.02, init[2]]))
    return out


def base_clouds():
    """-> target (1 600, 4) float32 in the target frame, source (321, 4) float32 in the room's own frame (a subset, in the
    target's order), the room-frame cloud."""
    rng = np.random.default_rng(SEED)
    room = _room(rng, 600)
    A = SR.rot_zyx(BASE_ANGLES)
    tgt = _cloud4(room[:, :3].astype(np.float64) @ A.T + np.array(BASE_OFFSET))
    pick = np.sort(rng.choice(len(room), 321, replace=False))
    return tgt, room[pick].copy(), room


# Whole loops of a case: (max_iterations, the all-float64 oracle takes the same number of iterations).  The base clouds stand
# 340 m from the origin, where a float32 coordinate has a quantum of 3e-5 m: the mean squared distance of the aligned clouds
# cannot fall below ~1e-11 m^2 and moves by 1e-12 .. 1e-11 from one iteration to the next for as long as the float32 transform
# changes in its last bits.  PCL's absolute criterion (1e-12) is met there when that noise stops, 1 - 3 iterations after an
# all-float64 restatement, which has no such floor, meets it (iteration 7).  So the base loops run twice: stopped by the cap
# at 5 iterations, where every formulation agrees, and with the default 10, where ref_align -- float32 where PCL and the
# device are -- is the yardstick for the count and the oracle for the transform alone.
LOOP_DEFAULT = ((10, True),)
LOOP_FAR = ((5, True), (10, False))


def case(name, family, target, source, T, gate=None, degenerate=False, loop=(), deep=False):
    loop = LOOP_DEFAULT if loop is True else tuple(loop)
    return dict(name=name, family=family, target=np.ascontiguousarray(target, F32), source=np.ascontiguousarray(source, F32),
                T=np.asarray(T, F32).reshape(4, 4), gate=gate, degenerate=degenerate, loop=loop, deep=deep)


def base_pose_members():
    """The base clouds under the seven rotations: the source re-expressed for each so that it lands where it lands under the
    initial one.  -> list of (name, target, source, T)."""
    tgt, src0, _ = base_clouds()
    t = np.array(BASE_OFFSET) + np.array(STEP_SHIFT)
    angles = pose_angles()
    R0 = SR.rot_zyx(angles[0])
    out = []
    for name, a in zip(POSE_NAMES, angles):
        Rk = SR.rot_zyx(a)
        src = src0.copy()
        if name != "init":
            src[:, :3] = (src0[:, :3].astype(np.float64) @ (Rk.T @ R0).T).astype(F32)
        out.append((name, tgt, src, _T(Rk, t)))
    return out


def exact_gate(target, source, T, k):
    """A subset of the source and a gate that keeps exactly k of it, every nearest distance at least 2 mm from the gate: of
    the 40 source points nearest to the target the k that span the largest triangle (k = 2: segment) -- three points close to
    a line would make the fit ill-conditioned -- and every point more than 4 mm beyond the farthest of them."""
    import itertools
    st = ref_step(target, source, T)
    d = np.sqrt(st["d2"].astype(np.float64))
    near = np.argsort(d, kind="stable")[:40]
    P = st["p"].astype(np.float64)

    def span(c):
        a = P[list(c)]
        return np.linalg.norm(np.cross(a[1] - a[0], a[2] - a[0])) if k == 3 else np.linalg.norm(a[1] - a[0])
    best = max(itertools.combinations(near, k), key=span)
    edge = max(d[j] for j in best)
    sel = np.sort(np.array(list(best) + [j for j in range(len(d)) if d[j] > edge + 4e-3], np.int64))
    return source[sel].copy(), float(edge + 2e-3)


def plane_clouds(seed, n_t=800, n_s=321, thickness=0.0):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-10, 10, n_t), rng.uniform(-6, 6, n_t),
                    3.0 + (rng.uniform(-0.5, 0.5, n_t) * thickness if thickness else np.zeros(n_t))], 1)
    pick = np.sort(rng.choice(n_t, n_s, replace=False))
    return xyz, pick


def deep_target():
    """The base target with the far clusters of tests/test_gpu_stack_shapes.py: a tree deeper than the 33 levels of the LDS
    stack; the base target is its prefix."""
    import test_gpu_stack_shapes
    tgt, _, _ = base_clouds()
    return test_gpu_stack_shapes._deepen(tgt, 34, 5)


def cases():
    """Every input of the step-level tests.  -> list of case()."""
    out = []
    members = base_pose_members()
    tgt, src0, room = base_clouds()
    # seven rotations of the running transform, without and with the 0.6 m gate
    for name, t, s, T in members:
        out.append(case("pose_" + name, "base", t, s, T, loop=LOOP_FAR if name in LOOP_POSES else ()))
        out.append(case("pose_%s_gate0.6" % name, "base", t, s, T, gate=0.6))
    _, t, s, T = members[0]
    _, _, s_tilt, T_tilt = members[SR.TILTED]
    # source sizes: empty, fewer than 3 correspondences, one wave, one block and their tails
    for m in SOURCE_SIZES[:-1]:
        out.append(case("source_%d" % m, "base", t, s[:m], T))
        if m >= 63:
            out.append(case("source_%d_tilted_gate0.6" % m, "base", t, s_tilt[:m], T_tilt, gate=0.6))
    # target sizes: the -1 slots of the 5-NN, tiny trees (a spread subset of the target, not its first points)
    rng = np.random.default_rng(SEED + 1)
    spread = rng.permutation(len(t))
    for m in TARGET_SIZES[:-1]:
        out.append(case("target_%d" % m, "tiny_target", t[spread[:m]], s[:129], T, degenerate=m < 3))
    # gates leaving exactly 2 and exactly 3 correspondences
    for k in (2, 3):
        sg, g = exact_gate(t, s, T, k)
        out.append(case("gate_keeps_%d" % k, "gate_keeps_3", t, sg, T, gate=g))
    # the constructed equality d2 == float32(gate^2): kept, as PCL keeps distance <= max
    eq_t = np.array([[0, 0, 0], [3, 1, 0], [-2, 4, 1], [1, -3, 2], [4, 4, -1], [-3, -2, 3]], np.float64)
    eq_s = eq_t + np.array([[0.5, 0, 0], [0.1, -0.05, 0.02], [-0.2, 0.1, 0.05], [0.05, 0.2, -0.1], [-0.1, -0.1, 0.2], [0.3, 0.0, -0.2]])
    out.append(case("gate_equality", "equality", _cloud4(eq_t), _cloud4(eq_s), np.eye(4), gate=0.5))
    # deep target: the overflow-stack instantiation; the same input without the clusters is pose_rand1
    _, _, s_d, T_d = members[DEEP_POSE]
    out.append(case("deep", "base", deep_target(), s_d, T_d, loop=LOOP_FAR, deep=True))
    out.append(case("deep_gate0.6", "base", deep_target(), s_d, T_d, gate=0.6, deep=True))
    # planar clouds
    xyz, pick = plane_clouds(SEED + 2)
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = SR.rot_zyx((0.02, -0.015, 0.03)), (0.15, -0.1, 0.05)     # source -> target, the truth
    Ei = np.linalg.inv(E)
    src_p = _cloud4(xyz[pick] @ Ei[:3, :3].T + Ei[:3, 3])
    G = _T(SR.rot_zyx((0.0, 0.0, 0.01)), (0.05, 0.02, 0.0))                         # the guess
    out.append(case("plane_z3", "planar", _cloud4(xyz), src_p, G, loop=True))
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = SR.rot_zyx(BASE_ANGLES), PLANE_OFFSET
    xyz_t = (xyz - np.array([0, 0, 3.0])) @ A[:3, :3].T + A[:3, 3]
    src_local = xyz[pick] - np.array([0, 0, 3.0])
    src_t = _cloud4(src_local @ Ei[:3, :3].T + Ei[:3, 3])
    Tt = A @ E @ np.linalg.inv(_T(SR.rot_zyx((0.0, 0.0, 0.01)), (0.05, 0.02, 0.0)).astype(np.float64))
    out.append(case("plane_tilted", "planar_tilted", _cloud4(xyz_t), src_t, Tt.astype(F32), loop=True))
    slab, _ = plane_clouds(SEED + 3, n_t=600, thickness=0.01)
    mirrored = slab.copy()
    mirrored[:, 2] = 6.0 - slab[:, 2]
    out.append(case("slab_mirrored", "slab", _cloud4(slab), _cloud4(mirrored), np.eye(4), loop=True))
    # rank-deficient targets: R is not unique
    rng = np.random.default_rng(SEED + 4)
    blob = rng.normal(0, 0.5, (100, 3))
    line = np.stack([rng.uniform(-10, 10, 400), np.full(400, 7.0), np.full(400, -2.0)], 1)
    out.append(case("line_axis", "rank_deficient", _cloud4(line), _cloud4(line[::4] + rng.normal(0, 0.05, (100, 3)) + [0.1, 0.2, -0.1]),
                    np.eye(4), degenerate=True))
    on_x = line * np.array([1.0, 0.0, 0.0])    # y = z = 0: sum s t^T has two columns of exact zeros, H has exact rank 1
    out.append(case("line_x_axis", "rank_deficient", _cloud4(on_x), _cloud4(on_x[::4] + rng.normal(0, 0.05, (100, 3)) + [0.1, 0.2, -0.1]),
                    np.eye(4), degenerate=True))
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    gl = np.array([34.0, -17.5, 3.0]) + rng.uniform(-10, 10, 400)[:, None] * u
    out.append(case("line_general", "rank_deficient", _cloud4(gl), _cloud4(gl[::4] + rng.normal(0, 0.05, (100, 3)) + [0.1, 0.2, -0.1]),
                    np.eye(4), degenerate=True))
    out.append(case("two_points", "rank_deficient", _cloud4([[3, -2, 1], [5, 1, 0.5]]), _cloud4(blob * 3 + [4, 0, 1]), np.eye(4), degenerate=True))
    out.append(case("one_point", "rank_deficient", _cloud4([[3, -2, 1]]), _cloud4(blob + [3.2, -2.1, 0.8]), np.eye(4), degenerate=True))
    out.append(case("one_point_origin", "rank_deficient", _cloud4([[0, 0, 0]]), _cloud4(blob), np.eye(4), degenerate=True))
    # identical clouds: the source a subset of the target, identity guess
    out.append(case("identical", "identical", room, room[::5], np.eye(4), loop=True))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def with_stride(cloud, stride):
    """The (n, 4) cloud as an (n, stride / 4) array: x, y, z first, the rest filled with a value a reader must not use."""
    c = np.asarray(cloud, F32)
    out = np.full((len(c), stride // 4), 1e30, F32)
    out[:, :3] = c[:, :3]
    return out
