"""float64 reference of the scan-match normal equations (ScanMatch.cpp:185-208) and the family of general poses the
scan-match kernels are held to it on.  numpy only: nothing here imports the library under test or its oracle.

TEST INFRASTRUCTURE: imported by tests/test_scanmatch_ref.py (CPU) and the GPU tests that compare normal-equation sums.

The reference takes what the kernels take -- the float32 scan points, the float32 coefficients of the sweep's tap, the float32
pose angles -- and evaluates the row formula and the 21 + 6 sums in float64.  Beside every value it carries a MAJORANT: the
same expression with every subterm replaced by its absolute value.  For a row entry J the majorant Jh bounds every
intermediate of any evaluation order, so a rounded evaluation is off by at most (number of roundings) * eps * Jh whatever
cancels inside; for a sum, M[k] = sum Jh_i Jh_j (sum Jh_i |b| for J^T r) does the same for the accumulation.  The unit of
tolerance of entry k is u[k] = 2**-24 * M[k]: per entry, and aware of cancellation in the row and in the sum.

The formula is the reference's, as written, including quirk Q1 (SURVEY: the unparenthesised `crz*sry*crx + srz*srx*pz` in
arz).  `variant` applies one of the recorded mutations to a COPY of the reference (never to a kernel): what a test built on
this module can and cannot see is measured in tests/test_scanmatch_ref.py.
"""
import numpy as np

EPS32 = 2.0 ** -24  # unit roundoff of float32

ROW_VARIANTS = ("q1_parenthesised", "ary_srx_sign")
SUM_VARIANTS = ("swap_translation_entries", "swap_jtr_3_5", "drop_last_row", "negate_jtr")

# packed upper triangle, row-major: entry (i, j), i <= j, is TRI[i][j]
TRI = np.zeros((6, 6), np.int64)
_k = 0
for _i in range(6):
    for _j in range(_i, 6):
        TRI[_i, _j] = TRI[_j, _i] = _k
        _k += 1
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def sincos64(pose32):
    """{srx, crx, sry, cry, srz, crz} of the FLOAT32 pose angles, evaluated in float64."""
    a = np.asarray(pose32, np.float32).astype(np.float64)
    return np.array([np.sin(a[0]), np.cos(a[0]), np.sin(a[1]), np.cos(a[1]), np.sin(a[2]), np.cos(a[2])])


def _rows(sc, q, coeff, majorant, variant=None):
    """ScanMatch.cpp:185-203.  majorant: every leaf by its absolute value and every minus sign a plus."""
    q = np.asarray(q)[:, :3].astype(np.float64)
    c = np.asarray(coeff).astype(np.float64)
    sc = np.asarray(sc, np.float64)
    if majorant:
        q, c, sc = np.abs(q), np.abs(c), np.abs(sc)
    n = 1.0 if majorant else -1.0  # a minus sign of the formula
    srx, crx, sry, cry, srz, crz = sc
    px, py, pz = q[:, 0], q[:, 1], q[:, 2]
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    f = n if variant == "ary_srx_sign" else 1.0  # mutation: the sign of one ary subterm that carries srx
    arx = (((crz * sry * crx + srz * srx) * py + (srz * crx + n * crz * sry * srx) * pz) * cx
           + ((srz * sry * crx + n * crz * srx) * py + n * (srz * sry * srx + crz * crx) * pz) * cy
           + (cry * crx * py + n * cry * srx * pz) * cz)
    ary = ((n * crz * sry * px + f * crz * cry * srx * py + crz * cry * crx * pz) * cx
           + (n * srz * sry * px + srz * cry * srx * py + srz * cry * crx * pz) * cy
           + (n * cry * px + n * sry * srx * py + n * sry * crx * pz) * cz)
    if variant == "q1_parenthesised":  # mutation: what the author meant
        q1 = (crz * sry * crx + srz * srx) * pz
    else:                              # as written (quirk Q1): pz multiplies the second product only
        q1 = crz * sry * crx + srz * srx * pz
    arz = ((n * srz * cry * px + n * (srz * sry * srx + crz * crx) * py + (crz * srx + n * srz * sry * crx) * pz) * cx
           + (crz * cry * px + (crz * sry * srx + n * srz * crx) * py + q1) * cy)
    J = np.stack([arx, ary, arz, cx, cy, cz], 1)
    b = np.abs(c[:, 3]) if majorant else -c[:, 3]
    return J, b


def rows64(pose32, q, coeff, variant=None):
    """-> J (n, 6), b (n,) in float64: the six Jacobian entries and b = -coeff[3] of every point."""
    return _rows(sincos64(pose32), q, coeff, False, variant)


def majorant(pose32, q, coeff):
    """-> Jh (n, 6), |b| (n,): rows64 with every subterm replaced by its absolute value."""
    return _rows(sincos64(pose32), q, coeff, True)


def sums64(J, b, keep, Jh=None, bh=None, variant=None):
    """The 21 J^T J (packed upper triangle) + 6 J^T r sums over the rows `keep` selects, float64 -> (S[27], M[27]); M from the
    majorant rows (Jh, bh; |J|, |b| when none is given).  u[k] = EPS32 * M[k]."""
    keep = np.asarray(keep, bool)
    Jh = np.abs(J) if Jh is None else Jh
    bh = np.abs(b) if bh is None else bh
    if variant == "drop_last_row":  # mutation: the last kept row of the scan never reaches the sum
        keep = keep.copy()
        keep[np.flatnonzero(keep)[-1]] = False
    J, b, Jh, bh = J[keep], b[keep], Jh[keep], bh[keep]
    S, M = np.zeros(27), np.zeros(27)
    for k, (i, j) in enumerate(PAIRS):
        S[k] = np.sum(J[:, i] * J[:, j])
        M[k] = np.sum(Jh[:, i] * Jh[:, j])
    for i in range(6):
        S[21 + i] = np.sum(J[:, i] * b)
        M[21 + i] = np.sum(Jh[:, i] * bh)
    if variant == "swap_translation_entries":  # mutation: (3,4) and (4,5) of the translation block change places
        a, c = TRI[3, 4], TRI[4, 5]
        S[[a, c]] = S[[c, a]]
    elif variant == "swap_jtr_3_5":
        S[[24, 26]] = S[[26, 24]]
    elif variant == "negate_jtr":
        S[21:27] = -S[21:27]
    return S, M


def reference_sums(pose32, q, coeff, flags=None, variant=None, keep=None, b=None):
    """(S[27], u[27]) of one sweep from its taps: q (n, >=3) the scan points in tap order (corner then surf), coeff (n, 4)
    and flags (n,) the tap's; kept rows are those with flags & 4.  keep (n,) bool: the kept rows given directly (a tap
    without flag bits).  b (n,): the right-hand side where it is not -coeff[3] (variant B scales it, tests/odom_ref.py); its
    majorant is |b|."""
    rv = variant if variant in ROW_VARIANTS else None
    sv = variant if variant in SUM_VARIANTS else None
    J, b0 = rows64(pose32, q, coeff, rv)
    Jh, bh = majorant(pose32, q, coeff)
    if b is not None:
        b0 = np.asarray(b, np.float64)
        bh = np.abs(b0)
    keep = (np.asarray(flags) & 4) != 0 if keep is None else np.asarray(keep, bool)
    S, M = sums64(J, b0, keep, Jh, bh, sv)
    return S, EPS32 * M


def units(got, S, u):
    """|got - S| / u per entry (0 where both the difference and the unit are 0: an entry no row contributes to)."""
    d = np.abs(np.asarray(got, np.float64)[:27] - S)
    out = np.zeros(27)
    nz = u > 0
    out[nz] = d[nz] / u[nz]
    out[~nz & (d > 0)] = np.inf
    return out


def rows32_pairwise_sums(pose32, q, coeff, flags=None, keep=None, b=None):
    """Floor (a): the same formula in numpy float32 (float32 sin/cos, float32 rows and products), summed with numpy's pairwise
    float32 sum -> S32[27].  What a careful fp32 implementation gives; reference side only.  keep / b as in reference_sums
    (b float32)."""
    a = np.asarray(pose32, np.float32)
    sc = np.array([np.sin(a[0]), np.cos(a[0]), np.sin(a[1]), np.cos(a[1]), np.sin(a[2]), np.cos(a[2])], np.float32)
    q = np.asarray(q, np.float32)[:, :3]
    c = np.asarray(coeff, np.float32)
    srx, crx, sry, cry, srz, crz = sc
    px, py, pz = q[:, 0], q[:, 1], q[:, 2]
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    arx = (((crz * sry * crx + srz * srx) * py + (srz * crx - crz * sry * srx) * pz) * cx
           + ((srz * sry * crx - crz * srx) * py - (srz * sry * srx + crz * crx) * pz) * cy
           + (cry * crx * py - cry * srx * pz) * cz)
    ary = ((-crz * sry * px + crz * cry * srx * py + crz * cry * crx * pz) * cx
           + (-srz * sry * px + srz * cry * srx * py + srz * cry * crx * pz) * cy
           + (-cry * px - sry * srx * py - sry * crx * pz) * cz)
    arz = ((-srz * cry * px - (srz * sry * srx + crz * crx) * py + (crz * srx - srz * sry * crx) * pz) * cx
           + (crz * cry * px + (crz * sry * srx - srz * crx) * py + crz * sry * crx + srz * srx * pz) * cy)
    J = np.stack([arx, ary, arz, cx, cy, cz], 1)
    assert J.dtype == np.float32
    keep = (np.asarray(flags) & 4) != 0 if keep is None else np.asarray(keep, bool)
    J, b = J[keep], (-c[keep, 3] if b is None else np.asarray(b, np.float32)[keep])
    S = np.zeros(27, np.float32)
    for k, (i, j) in enumerate(PAIRS):
        S[k] = np.sum(J[:, i] * J[:, j], dtype=np.float32)
    for i in range(6):
        S[21 + i] = np.sum(J[:, i] * b, dtype=np.float32)
    return S


# ---------------------------------------------------------------------------
# the tolerance: K units per entry
# ---------------------------------------------------------------------------
# floor (a), max over entries and family poses: 1.66 measured by tests/test_scanmatch_ref.py::test_floors (1.25 at init_pose)
FLOOR_PAIRWISE = 1.7


ROW_UNITS = 4 + 8  # worst-case distance of a correct fp32 row entry from rows64, in units 2**-24 * Jh (k_apriori)


def k_apriori():
    """Worst-case distance, in units u[k], of the device's fp32 sums from sums64 -- read out of the code
    (csrc/lslam_device.hpp jacobian_row, csrc/lslam_sweep_dev.hpp block_accumulate, csrc/lslam_solve_dev.hpp
    reduce_partials; the library is built without FMA contraction, which could only remove roundings):

      row entry   4   sin/cos: each leaf carries up to three of them, libm's float32 results within 0.56 ulp (1.12 units at
                      worst) each of the float64 values sums64 uses: 3.4, counted as 4
                + 8   rounded operations on the longest path of arx / ary / arz (two products of sin/cos, the sum in the
                      bracket, the product with p, the sum over p, the product with the coefficient, two sums over the
                      coefficients); the translation entries and b are copies
      product     2 * 12 + 1 (the VALU path rounds the product; the MFMA's fused multiply-add does not)
      wavefront   VALU: 6 shuffle levels.  MFMA: the 64 rows of a wavefront are one fma chain in row order, 63 roundings,
                  each at most one unit of the chain's running majorant
      block       3 additions (four wavefronts in fixed order) + 1 where a second pass adds onto the first's record (grid)
      across      blocks are added in float64; one rounding to the float32 the tap returns

    VALU: 25 + 6 + 4 + 1 = 36.  MFMA: 24 + 63 + 4 + 1 = 92.  Every rounding is counted at its worst and as if all were
    aligned, so this bounds what correct code can do; it is not what it typically does (measured values are in the tests'
    docstrings)."""
    row = ROW_UNITS
    valu = (2 * row + 1) + 6 + 4 + 1
    mfma = 2 * row + 63 + 4 + 1
    return float(max(valu, mfma))


K = max(10.0 * FLOOR_PAIRWISE, k_apriori())  # = 92: the derived value, because it exceeds ten times the floor


# ---------------------------------------------------------------------------
# the stereo term: sums of given fp32 rows
# ---------------------------------------------------------------------------
def stereo_sums64(rows):
    """rows (n, 3, 7) float32 = the oracle's scaled [J | b] rows (unused rows are zero) -> (S[27], u[27]) in float64."""
    r = np.asarray(rows).astype(np.float64).reshape(-1, 7)
    S, M = np.zeros(27), np.zeros(27)
    for k, (i, j) in enumerate(PAIRS):
        S[k] = np.sum(r[:, i] * r[:, j])
        M[k] = np.sum(np.abs(r[:, i] * r[:, j]))
    for i in range(6):
        S[21 + i] = np.sum(r[:, i] * r[:, 6])
        M[21 + i] = np.sum(np.abs(r[:, i] * r[:, 6]))
    return S, EPS32 * M


def stereo_pairwise32(rows):
    r = np.asarray(rows, np.float32).reshape(-1, 7)
    S = np.zeros(27, np.float32)
    for k, (i, j) in enumerate(PAIRS):
        S[k] = np.sum(r[:, i] * r[:, j], dtype=np.float32)
    for i in range(6):
        S[21 + i] = np.sum(r[:, i] * r[:, 6], dtype=np.float32)
    return S


# pairwise fp32 sum of the oracle's rows against float64, max over sizes, gates and poses: 1.98 measured (test_scanmatch_ref.py)
FLOOR_STEREO = 2.0


def ks_apriori():
    """The device forms the oracle's rows (same fp32 operations, no contraction) and contracts the 3 x 64 rows of a wavefront
    in one MFMA fma chain (csrc/lslam_stereo.hip: 48 instructions of 4 rows): 191 roundings, then 3 additions over the block's
    wavefronts; blocks are added in float64 and the tap returns float64."""
    return 191.0 + 3.0


K_S = max(10.0 * FLOOR_STEREO, ks_apriori())


# ---------------------------------------------------------------------------
# general poses
# ---------------------------------------------------------------------------
def rot_zyx(angles):
    """R = Rz Ry Rx (util/transform_utils.h:288-299), float64."""
    rx, ry, rz = (float(v) for v in angles)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def reexpress(cloud, pose_from, pose_to):
    """The sensor-frame cloud that lands, under pose_to's rotation, where `cloud` lands under pose_from's: q' = (Rn^T R0) q
    with the rotations of the float32 angles, in float64, rounded once to float32; further columns (intensity) are kept."""
    c = np.asarray(cloud, np.float32)
    A = rot_zyx(np.asarray(pose_to, np.float32)[:3].astype(np.float64)).T @ rot_zyx(np.asarray(pose_from, np.float32)[:3].astype(np.float64))
    out = c.copy()
    out[:, :3] = (c[:, :3].astype(np.float64) @ A.T).astype(np.float32)
    return out


FAMILY_NAMES = ("init", "rand0", "rand1", "rand2", "rand3", "yaw_pi", "pitch_half_pi")
TILTED = 1            # index of a tilted member used where one is enough
RAGGED = ((1, 0), (0, 1), (1, 777), (130, 0), (63, 65), (129, 4099))


def general_pose_family(problem, seed=3):
    """Seven poses with the scan of `problem` re-expressed for each: q' = (Rn^T R0) q with R0 the rotation of init_pose and
    the translation kept, computed in float64 and rounded once to float32 -- so every point lands in the map where it landed
    at init_pose (to fp32 rounding), the neighbourhoods stay dense, and each member's pose is as far from the pose at which
    its scan matches the map as init_pose is from gt_pose.  Raycasting from a tilted sensor would change which points exist.
    -> list of dict(name, pose float32 [6], corner, surf float32 (n, 4))."""
    init = np.asarray(problem["init_pose"], np.float32)
    rng = np.random.default_rng(seed)
    angles = [init[:3].astype(np.float64)]
    for _ in range(4):
        roll, pitch = rng.uniform(-1.3, 1.3, 2)
        angles.append(np.array([roll, pitch, rng.uniform(-np.pi, np.pi)]))
    angles.append(np.array([init[0], init[1], np.pi - 1e-3], np.float64))
    angles.append(np.array([init[0], np.pi / 2 - 0.02, init[2]], np.float64))
    out = []
    for name, a in zip(FAMILY_NAMES, angles):
        pose = np.concatenate([a, init[3:].astype(np.float64)]).astype(np.float32)
        if name == "init":
            corner, surf = np.array(problem["corner"], np.float32), np.array(problem["surf"], np.float32)
        else:
            corner, surf = reexpress(problem["corner"], init, pose), reexpress(problem["surf"], init, pose)
        out.append(dict(name=name, pose=pose, corner=corner, surf=surf))
    return out


def ragged_subset(member, flags, n_corner, n_surf):
    """(corner[:n_corner], surf[:n_surf]) of the member's clouds reordered kept-rows-first (`flags`: a sweep's flags of the
    whole member at its pose, corner then surf; whether a point is kept does not depend on the other scan points).  So
    (1, 0) is one lane with a non-zero row in its block and (63, 65) two partly filled wavefronts of non-zero rows."""
    nc = len(member["corner"])
    kept = (np.asarray(flags) & 4) != 0
    oc = np.argsort(~kept[:nc], kind="stable")
    os_ = np.argsort(~kept[nc:], kind="stable")
    return member["corner"][oc[:n_corner]].copy(), member["surf"][os_[:n_surf]].copy()


def assert_sums_per_entry(sums, pose32, corner, surf, coeff, flags, label=None, k=None):
    """Every one of the 27 sums of a device sweep within k (default K) units u[k] of the float64 reference built from the
    sweep's own taps.  -> the distances in units, for the caller to print."""
    k = K if k is None else k
    S, u = reference_sums(pose32, np.concatenate([corner, surf]), coeff, flags)
    un = units(sums, S, u)
    assert un.max() <= k, (label, "entry %d: %.1f units > %.0f" % (un.argmax(), un.max(), k), un.round(1).tolist())
    return un
