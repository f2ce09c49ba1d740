"""float64 statement of the Gauss-Newton solve step (ScanMatch.cpp:206-260) with its degenerate branch, the committed 6x6
systems it is compared on, and the corridor scenes of the degenerate loop tests.  numpy only: nothing here imports the library
under test or its oracle.

TEST INFRASTRUCTURE: imported by tests/test_degenerate_ref.py (CPU) and tests/test_gpu_degenerate.py, test_gpu_parity.py,
test_gpu_odom_general.py (device).

The branch (quirk Q2): at iteration 0 the reference takes the eigenvectors of A^T A as the COLUMNS of matV, zeroes the ROWS of a
copy whose eigenvalue is below the threshold (ascending, stopping at the first that is not) and keeps matP = matV^-1 matV2 for
the whole loop; every iteration's update is matP x.  With V orthogonal that is

    P0 = V^T diag(0^k, 1^(6-k)) V,        E, V = numpy.linalg.eigh(A64)

which is NOT the orthogonal projector V[:, k:] V[:, k:]^T (that would need the columns zeroed), and which depends on the sign an
eigensolver gives each eigenvector: flipping eigenvector j flips row and column j of P0.  matP is therefore one of the 32
matrices S P0 S, S = diag(+-1) with the first sign fixed (family()); which one is read off the implementation's matP
(nearest()), and the conditions below make that reading unambiguous.

Units.  unit_P(E) = 2^-24 lambda_max / (smallest gap between neighbouring eigenvalues): the first-order error of a float32
eigenvector, of which P0 is a product.  unit_x(A64, x_qr64) = 2^-24 cond(A64) max|x_qr64|: the plain solve's error, which the
projected step inherits through a P whose entries are at most 1 in magnitude.  delta_r and delta_t are norms of three
components of x scaled to degrees and centimetres: their unit is sqrt(3) times the scaled unit_x plus two float32 roundings of
the value itself (the rounded conversion and the rounded square root).

K_P and K_X are ten times the largest distance the CPU oracle shows on systems() (tests/test_degenerate_ref.py measures them
and says what it measured).
"""
import numpy as np

EPS32 = 2.0 ** -24

# ten times the float32 floors measured by tests/test_degenerate_ref.py::test_floors (its docstring has the figures)
K_P = 12.91
K_X = 17.45

POSE_IN = np.array([0.03, 0.5, -0.02, 0.2, 0.1, 1.0], np.float32)


def count_below(E, eig_thresh):
    """ScanMatch.cpp:224-233: eigenvalues ascending; zeroing stops at the first one not below the threshold."""
    k = 0
    for e in E:
        if e < eig_thresh:
            k += 1
        else:
            break
    return k


def projector(V, k):
    """matV^-1 matV2 with rows 0..k-1 of matV2 zeroed, V's columns the eigenvectors (ascending)."""
    D = np.diag([0.0] * k + [1.0] * (6 - k))
    return V.T @ D @ V


def family(P0):
    """The 32 sign variants S P0 S, S = diag(+-1), first sign +1 -> (32, 6, 6)."""
    out = []
    for m in range(32):
        s = np.array([1.0] + [(-1.0 if (m >> b) & 1 else 1.0) for b in range(5)])
        out.append(P0 * s[:, None] * s[None, :])
    return np.array(out)


def nearest(P, fam):
    """-> (distance to the nearest member, distance to the nearest member that differs from it -- inf when the family is a
    single matrix --, index of the nearest member); distances are the largest absolute entry difference."""
    P = np.asarray(P, np.float64).reshape(6, 6)
    d = np.abs(fam - P[None]).max(axis=(1, 2))
    i = int(np.argmin(d))
    other = np.abs(fam - fam[i][None]).max(axis=(1, 2)) > 0
    return float(d[i]), (float(d[other].min()) if other.any() else np.inf), i


def unit_P(E):
    return EPS32 * float(E[-1]) / float(np.min(np.diff(E)))


def unit_x(A64, x_qr64):
    return EPS32 * float(np.linalg.cond(A64)) * float(np.abs(x_qr64).max())


def unit_x_of(AtA, Atb):
    """unit_x of a float32 system; inf where the float64 solve itself refuses (an exactly singular matrix)."""
    A = np.asarray(AtA, np.float32).astype(np.float64).reshape(6, 6)
    try:
        return unit_x(A, np.linalg.solve(A, np.asarray(Atb, np.float32).astype(np.float64)))
    except np.linalg.LinAlgError:
        return np.inf


def deltas(x):
    """ScanMatch.cpp:249-253 in float64 -> (delta_r [deg], delta_t [cm])."""
    x = np.asarray(x, np.float64)
    return float(np.sqrt(np.sum(np.degrees(x[:3]) ** 2))), float(np.sqrt(np.sum((x[3:] * 100.0) ** 2)))


def delta_units(ux, dR, dT):
    """Units of delta_r and delta_t that belong to a unit ux of x (module docstring)."""
    return np.sqrt(3.0) * np.degrees(ux) + 2 * EPS32 * dR, np.sqrt(3.0) * 100.0 * ux + 2 * EPS32 * dT


def step64(AtA, Atb, it, pose, P, degenerate, eig_thresh=100.0, dr=0.05, dt=0.05):
    """ScanMatch.cpp:206-260 on the float32 inputs taken as float64.

    it == 0: the decision, k and P0 come from the eigen-decomposition; `P`, when given, is the matP an implementation returned
    and only selects the family member (the eigenvectors' signs) the projection uses; None selects P0 itself.
    it > 0: `P` and `degenerate` are the carried state and are used as they are.
    -> dict(x_qr, x, pose, delta_r, delta_t, converged, degenerate, P, and at it == 0: E, V, k, P0, dist = nearest()'s pair, member = the
    chosen member's index in family(P0))."""
    A = np.asarray(AtA, np.float32).astype(np.float64).reshape(6, 6)
    b = np.asarray(Atb, np.float32).astype(np.float64).reshape(6)
    pose = np.asarray(pose, np.float32).astype(np.float64).reshape(6)
    out = {}
    x_qr = np.linalg.solve(A, b)
    if it == 0:
        E, V = np.linalg.eigh(A)
        k = count_below(E, eig_thresh)
        P0 = projector(V, k)
        fam = family(P0)
        if P is None:
            chosen, dist, i = P0, (0.0, nearest(P0, fam)[1]), 0
        else:
            d0, d1, i = nearest(P, fam)
            chosen, dist = fam[i], (d0, d1)
        degenerate = k > 0
        out.update(E=E, V=V, k=k, P0=P0, dist=dist, member=i)
        P = chosen
    else:
        P = np.asarray(P, np.float32).astype(np.float64).reshape(6, 6)
    x = P @ x_qr if degenerate else x_qr
    dR, dT = deltas(x)
    out.update(x_qr=x_qr, x=x, pose=pose + x, delta_r=dR, delta_t=dT, converged=bool(dR < dr and dT < dt),
               degenerate=bool(degenerate), P=P, A=A)
    return out


def compare(got, s, k_p=None, k_x=None, check_x=True):
    """An implementation's step `got` (the dict oracle.gn_step / Context.gn_step return, iteration 0) against step64's `s`
    made with P = got["matP"].  -> dict of the distances in units (P, x, pose, delta_r, delta_t; nan where not compared) and
    ok: the decision, converged and every distance within k_p / k_x units (K_P / K_X)."""
    k_p = K_P if k_p is None else k_p
    k_x = K_X if k_x is None else k_x
    d = dict(P=np.nan, x=np.nan, pose=np.nan, delta_r=np.nan, delta_t=np.nan)
    ok = bool(got["degenerate"]) == s["degenerate"]
    if s["degenerate"]:
        d["P"] = s["dist"][0] / unit_P(s["E"])
        ok = ok and d["P"] <= k_p
    if check_x:
        ux = unit_x(s["A"], s["x_qr"])
        ur, ut = delta_units(ux, s["delta_r"], s["delta_t"])
        if ux > 0:
            d["x"] = float(np.abs(np.asarray(got["x"], np.float64) - s["x"]).max()) / ux
            # the pose is one more float32 addition: half an ulp of the sum on top
            perr = np.abs(np.asarray(got["pose"], np.float64) - s["pose"]) - EPS32 * np.abs(s["pose"])
            d["pose"] = float(np.maximum(perr, 0.0).max()) / ux
            d["delta_r"] = abs(float(got["delta_r"]) - s["delta_r"]) / ur
            d["delta_t"] = abs(float(got["delta_t"]) - s["delta_t"]) / ut
            ok = ok and max(d["x"], d["pose"], d["delta_r"], d["delta_t"]) <= k_x
        else:  # x = 0 exactly (every row zeroed, or a zero right-hand side)
            zero = not np.asarray(got["x"]).any() and float(got["delta_r"]) == 0.0 and float(got["delta_t"]) == 0.0
            d["x"] = d["pose"] = d["delta_r"] = d["delta_t"] = 0.0 if zero else np.inf
            ok = ok and zero and np.array_equal(np.asarray(got["pose"], np.float32), s["pose"].astype(np.float32))
        ok = ok and bool(got["converged"]) == s["converged"]
    d["ok"] = bool(ok)
    return d


def dot6_bound(P, x_qr):
    """Per-component bound of a six-term float32 dot product, fused or not, against the float64 product of the same float32
    factors: 6 * 2^-24 * sum_k |P[r, k] x_qr[k]| (five additions and up to six product roundings, each at most one unit of
    the running majorant, to first order).  -> (float64 product, bound)."""
    P = np.asarray(P, np.float32).astype(np.float64).reshape(6, 6)
    x = np.asarray(x_qr, np.float32).astype(np.float64)
    return P @ x, 6 * EPS32 * (np.abs(P) @ np.abs(x))


# ---------------------------------------------------------------------------
# the committed systems
# ---------------------------------------------------------------------------
# name, eigenvalues, seed of Q and of the step, scale of the step A^T b is made from, x compared with step64
_SYSTEMS = [
    ("k1_min5_max3e2", [5.0, 130.0, 180.0, 220.0, 260.0, 300.0], 1, 0.02, True),
    ("k1_min90_max1e4", [90.0, 400.0, 1500.0, 3000.0, 6000.0, 1.0e4], 2, 0.02, True),
    ("k2_max3e2", [5.0, 60.0, 140.0, 200.0, 250.0, 300.0], 3, 0.02, True),
    ("k2_max1e4", [8.0, 40.0, 800.0, 2500.0, 5000.0, 1.0e4], 4, 0.02, True),
    ("k3_max1e4", [20.0, 50.0, 90.0, 1000.0, 4000.0, 1.0e4], 5, 0.02, True),
    ("k5_max3e2", [5.0, 25.0, 45.0, 70.0, 90.0, 300.0], 6, 0.02, True),
    ("k6_all_below", [30.0, 45.0, 60.0, 75.0, 88.0, 95.0], 7, 0.02, True),
    ("k1_small_step", [5.0, 130.0, 180.0, 220.0, 260.0, 300.0], 8, 2.0e-4, True),  # converges with a non-zero update
    ("singular", [0.0, 242.0, 300.0, 400.0, 500.0, 600.0], 9, 0.02, False),
]
THRESHOLDS = (100.0, 10.0)
MIN_GAP = 3.0
MAX_COND = 2.0e3
MIN_SEPARATION_UNITS = 1.0e3
THRESH_MARGIN = 0.01


def systems():
    """-> list of dict(name, lam, AtA float32 (6, 6), Atb float32 (6,), pose float32 (6,), check_x).  A = Q diag(lam) Q^T
    symmetrised and rounded to float32; A^T b = A x_true rounded, x_true a step of the given scale."""
    out = []
    for name, lam, seed, scale, check_x in _SYSTEMS:
        rng = np.random.default_rng(1000 + seed)
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = (Q * np.array(lam)) @ Q.T
        AtA = ((A + A.T) / 2).astype(np.float32)
        x_true = rng.uniform(0.5, 1.0, 6) * rng.choice([-1.0, 1.0], 6) * scale
        Atb = (AtA.astype(np.float64) @ x_true).astype(np.float32)
        out.append(dict(name=name, lam=np.array(lam), AtA=AtA, Atb=Atb, pose=POSE_IN.copy(), check_x=check_x))
    return out


def assert_conditions(sy, eig_thresh):
    """The conditions on a system, of the float64 side alone (they keep a comparison from passing for the wrong reason).
    -> step64's dict at P = None."""
    s = step64(sy["AtA"], sy["Atb"], 0, sy["pose"], None, False, eig_thresh)
    E = s["E"]
    singular = not sy["check_x"]
    assert np.diff(E).min() >= MIN_GAP, (sy["name"], E)
    assert (np.abs(E - eig_thresh) > THRESH_MARGIN * eig_thresh).all(), (sy["name"], E, eig_thresh)
    if singular:
        assert abs(E[0]) <= EPS32 * E[-1], (sy["name"], E)
    else:
        assert np.linalg.cond(s["A"]) <= MAX_COND, (sy["name"], np.linalg.cond(s["A"]))
        dR, dT = s["delta_r"], s["delta_t"]  # the convergence flag is not decided by rounding
        ur, ut = delta_units(unit_x(s["A"], s["x_qr"]), dR, dT)
        assert abs(dR - 0.05) > 100 * K_X * ur or dT >= 0.05 + 100 * K_X * ut or s["k"] == 6, (sy["name"], dR, dT)
        assert abs(dT - 0.05) > 100 * K_X * ut or dR >= 0.05 + 100 * K_X * ur or s["k"] == 6, (sy["name"], dR, dT)
    if 0 < s["k"] < 6:  # the 32 members are told apart
        assert s["dist"][1] >= MIN_SEPARATION_UNITS * unit_P(E), (sy["name"], s["dist"][1] / unit_P(E))
        assert len({m.tobytes() for m in family(s["P0"])}) == 32, sy["name"]
    return s


# ---------------------------------------------------------------------------
# the scenes: one corridor, closed at its far end, and four scans of it
# ---------------------------------------------------------------------------
LANE, GRID = 1, 3
SCENE_NAMES = ("a_open", "b_end_wall", "c_thinned", "d_too_few")
EXPECT_DEGENERATE = [1, 0, 1, 0]
TOO_FEW_MATCHES = 5
END_WALL_POINTS = 250
THIN_SURF, THIN_CORNER = 12, 2  # scene c keeps every 12th floor / ceiling point and every 2nd corner point of scene a


def _truth(k):
    return np.array([(0.03, 0.5, -0.02, 0.2, 0.1, 1.0), (-0.02, 0.45, 0.03, -0.3, 0.15, 0.5), (0.01, 0.52, 0.02, 0.1, -0.1, -0.6),
                     (0.0, 0.5, 0.0, 0.0, 0.0, 0.0)][k], np.float32)


# an initial pose about 5 cm and 0.3 degrees from the truth
_OFFSET = np.array([0.003, -0.003, 0.003, 0.03, -0.03, 0.03], np.float32)
# Scene a starts where the oracle's third update lands on the convergence threshold: the loop stops there or runs four more
# iterations, and one ulp on the scan's coordinates decides which (tests/test_degenerate_ref.py measures it).  Found by stepping
# the scale of the offset in 1e-4; with the signs of _OFFSET itself the same scene never converges and is as insensitive as b.
_OFFSET_A = np.float32(0.9309) * np.array([0.003, -0.003, 0.003, 0.03, 0.03, -0.03], np.float32)


def scenes():
    """-> dict(map=(corner, surf), scans=[dict(name, corner, surf, gt_pose, init_pose)] in SCENE_NAMES order).  Map: the
    corridor of tests/test_gpu_edge_information.py with its far end closed.  Scans in their sensor frames:
      a  clear of the closed end: nothing constrains the motion along the axis
      b  reaches the closed end
      c  scan a with every THIN_SURF-th floor / ceiling point and every THIN_CORNER-th corner point kept: the vertical direction
         is left weakly constrained as well, and a second eigenvalue falls below 100
      d  so few points that fewer than 50 rows match
    """
    from test_gpu_edge_information import CLEAR, CORR_FACES, CORR_HI, CORR_LO, box_clouds, to_sensor
    from scanmatch_ref import rot_zyx
    closed = CORR_FACES + [(2, 1)]
    rng = np.random.default_rng(30)
    map_c, map_s = box_clouds(rng, CORR_LO, CORR_HI, closed, margin=CLEAR)

    def isometry(pose):
        T = np.eye(4)
        T[:3, :3] = rot_zyx(pose[:3].astype(np.float64))
        T[:3, 3] = pose[3:].astype(np.float64)
        return T.astype(np.float32)

    def world(faces, z_hi, n_surf, n_corner, seed):
        lo, hi = np.array(CORR_LO), np.array(CORR_HI)
        lo[2], hi[2] = -8.0, z_hi
        return box_clouds(np.random.default_rng(seed), lo, hi, faces, n_surf=n_surf, n_corner=n_corner, noise=0.01, margin=CLEAR)

    wa = world(CORR_FACES, 8.0, 600, 160, 31)
    wb = world(closed, CORR_HI[2], 600, 160, 32)
    # by area the end wall gets a dozen of the 600 points; END_WALL_POINTS more put the axis' eigenvalue above the threshold
    end = world([(2, 1)], CORR_HI[2], END_WALL_POINTS, 0, 33)
    wb = (wb[0], np.concatenate([wb[1], end[1]]))
    wc = world(CORR_FACES, 8.0, 600, 160, 31)
    wc = _thin(wc)
    wd = world(CORR_FACES, 8.0, 30, 12, 34)
    scans = []
    for k, (name, (corner, surf)) in enumerate(zip(SCENE_NAMES, (wa, wb, wc, wd))):
        gt = _truth(k)
        T = isometry(gt)
        scans.append(dict(name=name, corner=to_sensor(corner, T), surf=to_sensor(surf, T), gt_pose=gt, init_pose=(gt + (_OFFSET_A if k == 0 else _OFFSET)).astype(np.float32)))
    return dict(map=(map_c, map_s), scans=scans)


def _thin(w):
    """Scene c from scene a's world points: see scenes()."""
    from test_gpu_edge_information import CORR_HI, CORR_LO
    corner, surf = w
    level = (np.abs(surf[:, 1] - CORR_LO[1]) < 0.1) | (np.abs(surf[:, 1] - CORR_HI[1]) < 0.1)  # floor and ceiling
    keep = ~level
    keep[np.flatnonzero(level)[::THIN_SURF]] = True
    return corner[::THIN_CORNER], surf[keep]


def tap_system(sums):
    """(AtA float32 (6, 6) symmetrised from a sweep tap's 21 sums, Atb float32 (6,))."""
    from scanmatch_ref import PAIRS
    s = np.asarray(sums, np.float32)
    AtA = np.zeros((6, 6), np.float32)
    for k, (i, j) in enumerate(PAIRS):
        AtA[i, j] = AtA[j, i] = s[k]
    return AtA, s[21:27].copy()
