"""Plain references of one iteration of scan-to-scan odometry (variant B, LaserOdometry::scanMatch,
odometry/LaserOdometry.cpp:328-647) and the input families the odometry kernels are held to them on.  numpy only: nothing
here imports the library under test or its oracle, and nothing is shared with the kd-tree or the hashed grids.

TEST INFRASTRUCTURE: imported by tests/test_odom_ref.py (CPU) and tests/test_gpu_odom_general.py.

  corr_ref       the correspondences of :357-483 by brute force, in float32 with the reference's operation order -- exact,
                 not tolerant: given the de-skewed queries the answer is a deterministic fp32 function of the clouds
  to_start64     transformToStart (:135-142) in float64 from the float32 pose and point
  coeff64        point-to-line / point-to-plane distance and direction in float64, from the geometry, with both weight rules
  sums64_odom    the 27 sums from the step's own taps (rows of scanmatch_ref, b = float32(-0.05 d)), with the units u[k]
  k_odom_apriori the worst-case distance of the device's sums from sums64_odom, read out of the reduction's structure

`variant` applies one of the seeded mutations to a COPY of a reference (never to a kernel); tests/test_odom_ref.py measures
that each is seen.
"""
import numpy as np

import scanmatch_ref as R

EPS32 = R.EPS32
F32 = np.float32

CORR_VARIANTS = ("q5_bound_is_cloud_size", "ring_window_1", "flat_second_point_any_ring", "tie_takes_last")
COEFF_VARIANTS = ("no_weight_from_iter_5",)
SUM_VARIANTS = ("b_is_minus_d",)
VARIANTS = CORR_VARIANTS + COEFF_VARIANTS + SUM_VARIANTS


# ---------------------------------------------------------------------------
# correspondences
# ---------------------------------------------------------------------------
def _d2_f32(cloud_xyz, sel):
    """Squared distance of every cloud point from sel, float32: the differences per axis, their squares, (x + y) + z.
    nanoflann's L2 adaptor (nanoflann.hpp:364-372: result += diff * diff, x, y, z) and calcSquaredDiff
    (math_utils.h:47-54: dx*dx + dy*dy + dz*dz) round alike -- the difference's sign does not reach the square."""
    d = cloud_xyz - sel[None, :]
    assert d.dtype == F32
    sq = d * d
    return (sq[:, 0] + sq[:, 1]) + sq[:, 2]


def _first_min(d, mask, start, last=False):
    """(distance, position) of the first strictly smaller distance than `start` among mask, in the order given -- the walk's
    `if (d < min) { min = d; ind = j; }` run over the positions: the smallest value, and of equal ones the one met first
    (last=True: the mutation `<=`, which keeps the one met last -- also across the two walks).  -> (start, -1) when none is
    smaller."""
    if not mask.any():
        return start, -1
    dm = np.where(mask, d, F32(np.inf))
    k = int(np.argmin(dm)) if not last else int(len(dm) - 1 - np.argmin(dm[::-1]))
    if dm[k] < start or (last and dm[k] == start and start < F32(25.0)):
        return dm[k], k
    return start, -1


def _corr_one(xyz, ring, sel, n_queries, is_flat, variant):
    n = len(xyz)
    d = _d2_f32(xyz, sel)
    dmin = d.min()
    at = np.flatnonzero(d == dmin)
    tie = len(at) > 1
    i1 = int(at[-1] if variant == "tie_takes_last" else at[0])
    if not (dmin < F32(25.0)):  # :363 / :429
        return -1, -1, -1, False
    last = variant == "tie_takes_last"
    half = 1.5 if variant == "ring_window_1" else 2.5
    scan = int(ring[i1])
    m2, m3 = F32(25.0), F32(25.0)
    i2 = i3 = -1
    # forwards: j = i1 + 1 .. while j < n_queries (quirk Q5, :370 / :434: the QUERY count) and inside the cloud
    hi = n if variant == "q5_bound_is_cloud_size" else min(n_queries, n)
    if i1 + 1 < hi:
        r = ring[i1 + 1:hi]
        brk = r > scan + half
        stop = int(np.argmax(brk)) if brk.any() else len(r)
        r, dd = r[:stop], d[i1 + 1:i1 + 1 + stop]
        if not is_flat:
            m2, k = _first_min(dd, r > scan, m2, last)
            i2 = i1 + 1 + k if k >= 0 else i2
        else:
            c2 = np.ones(len(r), bool) if variant == "flat_second_point_any_ring" else r <= scan
            m2, k = _first_min(dd, c2, m2, last)
            i2 = i1 + 1 + k if k >= 0 else i2
            m3, k = _first_min(dd, ~(r <= scan), m3, last)
            i3 = i1 + 1 + k if k >= 0 else i3
    # backwards: j = i1 - 1 .. 0
    if i1 > 0:
        r = ring[:i1][::-1]
        brk = r < scan - half
        stop = int(np.argmax(brk)) if brk.any() else len(r)
        r, dd = r[:stop], d[:i1][::-1][:stop]
        if not is_flat:
            m2, k = _first_min(dd, r < scan, m2, last)
            i2 = i1 - 1 - k if k >= 0 else i2
        else:
            c2 = np.ones(len(r), bool) if variant == "flat_second_point_any_ring" else r >= scan
            m2, k = _first_min(dd, c2, m2, last)
            i2 = i1 - 1 - k if k >= 0 else i2
            m3, k = _first_min(dd, ~(r >= scan), m3, last)
            i3 = i1 - 1 - k if k >= 0 else i3
    return i1, i2, i3, tie


def corr_ref(last_c, last_s, sel_sharp, sel_flat, n_sharp, n_flat, variant=None):
    """The correspondences of :357-483 for de-skewed queries against the last clouds, by brute force.
    last_c / last_s (n, 4) float32 {x, y, z, ring + relTime}; sel_sharp / sel_flat (m, 3) float32; n_sharp / n_flat: the
    query counts the forward walks are bounded by (quirk Q5).
    -> ind (3, m_sharp + m_flat) int32 {closest, second, third}, -1: none (a sharp query has no third point);
       tie (m_sharp + m_flat,) bool: two different points lie at the winning (nearest) distance, inside the gate -- which of
       them nearestKSearch returns is nanoflann's visit order, which this reference does not have (it names the first)."""
    ms, mf = len(sel_sharp), len(sel_flat)
    ind = np.full((3, ms + mf), -1, np.int32)
    tie = np.zeros(ms + mf, bool)
    for c, (cloud, sel, nq, off) in enumerate(((last_c, sel_sharp, n_sharp, 0), (last_s, sel_flat, n_flat, ms))):
        cloud = np.asarray(cloud, F32)
        xyz = np.ascontiguousarray(cloud[:, :3])
        ring = cloud[:, 3].astype(np.int64)  # (int)intensity: truncation
        sel = np.asarray(sel, F32).reshape(-1, 3)
        for i in range(len(sel)):
            i1, i2, i3, t = _corr_one(xyz, ring, sel[i], int(nq), c == 1, variant)
            ind[:, off + i] = (i1, i2, i3)
            tie[off + i] = t
    return ind, tie


# ---------------------------------------------------------------------------
# transformToStart
# ---------------------------------------------------------------------------
def _rel(q):
    """s = 10 * (intensity - int(intensity)) of float32 points, in float64 (the subtraction is exact in either format)."""
    w = np.asarray(q, F32)[:, 3].astype(np.float64)
    return 10.0 * (w - np.trunc(w))


def to_start64(pose32, q):
    """transformToStart (:135-142) in float64 from the float32 pose and points: sel = R(s * rot) q + s * pos with
    R = Rz Ry Rx (transform_utils.h:288-299).  -> sel (n, 3), mag (n, 3) = sum_j |R_ij| |q_j| + |t_i|, the majorant the
    float32 evaluation's error is counted in."""
    p = np.asarray(pose32, F32).astype(np.float64)
    q = np.asarray(q, F32)
    s = _rel(q)
    x = q[:, :3].astype(np.float64)
    sel, mag = np.zeros((len(q), 3)), np.zeros((len(q), 3))
    for i in range(len(q)):
        Rm = R.rot_zyx(p[:3] * s[i])
        t = p[3:] * s[i]
        sel[i] = Rm @ x[i] + t
        mag[i] = np.abs(Rm) @ np.abs(x[i]) + np.abs(t)
    return sel, mag


def sel_units(sel32, sel64, mag):
    """|sel32 - sel64| in units 2**-24 * mag per coordinate (0 where both the difference and the majorant are 0)."""
    d = np.abs(np.asarray(sel32, np.float64) - sel64)
    out = np.zeros_like(d)
    nz = mag > 0
    out[nz] = d[nz] / (EPS32 * mag[nz])
    out[~nz & (d > 0)] = np.inf
    return out


# Roundings on the longest path of the float32 transformToStart (oracle_pose_to_Rt's quaternion route), each counted as one
# unit 2**-24 of the majorant:
#   s = 10 * frac (1), angle * s (1), sin / cos of the half angle (1), two quaternion products (1 product + 3 additions each:
#   8) = 11 per quaternion component; a rotation entry is quadratic in them: 2 * 11, + the product (1), the sum of two (1),
#   1 - (.) on the diagonal (1) = 25; the row: product with q (1), two additions (2), + t (1) = 29.
# (t_i = pos * s carries 2.)  Counted for angle * s below 1 rad, where no entry of R is formed by cancellation.
SEL_UNITS = 29.0


# ---------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------
def coeff64(A, B, C, X, it, is_flat, variant=None):
    """Distance and direction of X from the line AB (is_flat False; C unused) or the plane ABC (True), float64, with the
    weights of feature_utils.h: none before iteration 5, then 1 - 1.8 d (line) / 1 - 1.8 d / sqrt(|X|) (plane).
    A, B, C, X (n, 3).  -> coeff (n, 4) = {w * direction, w * d}, kept (n,) = w > 0.1 and d != 0, d (n,)."""
    A, B, X = (np.asarray(v, np.float64).reshape(-1, 3) for v in (A, B, X))
    if not is_flat:
        u = B - A
        L = np.linalg.norm(u, axis=1)
        u = u / L[:, None]
        r = X - A
        d = np.linalg.norm(np.cross(r, u), axis=1)           # |r x u|: the distance from the line
        perp = r - np.sum(r * u, axis=1)[:, None] * u       # from the line to X
        with np.errstate(invalid="ignore", divide="ignore"):
            direction = np.where(d[:, None] > 0, perp / d[:, None], 0.0)  # (X on the line: no direction, the row is dropped)
        w = 1.0 - 1.8 * d
    else:
        C = np.asarray(C, np.float64).reshape(-1, 3)
        nrm = np.cross(B - A, C - A)
        ln = np.linalg.norm(nrm, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = np.where(ln[:, None] > 0, nrm / ln[:, None], 0.0)  # (A, B, C on one line: no plane, d = 0, the row is dropped)
        sd = np.sum((X - A) * nrm, axis=1)
        direction = np.where(sd[:, None] < 0, -nrm, nrm)     # towards X
        d = np.abs(sd)
        w = 1.0 - 1.8 * d / np.sqrt(np.linalg.norm(X, axis=1))
    if it < 5 or variant == "no_weight_from_iter_5":
        w = np.ones(len(X))
    coeff = np.concatenate([direction * w[:, None], (d * w)[:, None]], axis=1)
    return coeff, (w > 0.1) & (d != 0), d


def coeff64_step(last_c, last_s, sel, ind, n_sharp, it, variant=None):
    """coeff64 of a whole step: sel (n, 3) and ind (3, n) in tap order (sharp then flat).  -> coeff (n, 4), kept (n,),
    d (n,), have (n,) = the query has all its points; rows without are zero / False."""
    n = len(sel)
    coeff, kept, d = np.zeros((n, 4)), np.zeros(n, bool), np.zeros(n)
    flat = np.arange(n) >= n_sharp
    have = (ind[0] >= 0) & (ind[1] >= 0) & (~flat | (ind[2] >= 0))
    for is_flat, cloud in ((False, last_c), (True, last_s)):
        m = have & (flat == is_flat)
        if not m.any():
            continue
        xyz = np.asarray(cloud, F32)[:, :3]
        Cc = xyz[ind[2][m]] if is_flat else None
        coeff[m], kept[m], d[m] = coeff64(xyz[ind[0][m]], xyz[ind[1][m]], Cc, np.asarray(sel)[m], it, is_flat, variant)
    return coeff, kept, d, have


def coeff_distance(c32, c64, d, X):
    """Largest |c32 - c64| over the four entries, relative to max(|d|, 2**-24 |X|), per point."""
    scale = np.maximum(np.abs(d), EPS32 * np.linalg.norm(np.asarray(X, np.float64), axis=1))
    return np.abs(np.asarray(c32, np.float64) - c64).max(axis=1) / np.maximum(scale, 1e-300)


# Largest distance of the C oracle's float32 coefficients from coeff64, relative to max(|d|, 2**-24 |X|), per family: measured
# by tests/test_odom_ref.py::test_coefficient_conditioning_per_family (against the oracle at its own sel, never a device).  The GPU test's bar
# for the independent coefficient check is COEFF_BAR_FACTOR times the family's value: room for the device's other sel bits and
# for the few points a family does not sample.  (The measurements, rounded up by a percent.)
COEFF_BAR_FACTOR = 4.0
COEFF_COND = {
    "ragged_1_0": 7.68e-07,
    "ragged_0_1": 1.05e-07,
    "ragged_63_65": 1.34e-05,
    "ragged_255_257": 0.000451,
    "ragged_256_256": 0.000451,
    "ragged_256_16128": 0.0128,
    "ragged_300_16200": 0.0128,
    "q5_few_sharp": 2.48e-05,
    "q5_more_sharp_than_cloud": 4.75e-05,
    "guard_edge": 3.39e-05,
    "pose_zero": 3.47e-05,
    "pose_drive": 0.0013,
    "pose_large": 4.35e-05,
    "reltime_0": 1.83e-05,
    "reltime_0999": 0.00108,
    "rings_64": 0.00282,
    "empty_rings": 0.0013,
    "rings_0_to_255": 0.0013,
    "not_ring_order": 0.0013,
    "rings_above_255": 0.00208,
    "sparse_2_to_4.9m": 2.13e-05,
    "walk_ties": 3.48e-05,
    "far_3km": 1.94e-05,
    "far_10km": 3.01e-05,
    "far_50km": 1.85e-05,
}


# ---------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------
def odom_b(coeff, variant=None):
    """:575: b = float32(-0.05 * float64(coeff[3]))."""
    c3 = np.asarray(coeff, F32)[:, 3].astype(np.float64)
    return (-c3 if variant == "b_is_minus_d" else -0.05 * c3).astype(F32)


def sums64_odom(pose32, q, coeff, keep, variant=None):
    """(S[27], u[27]) of one step from its taps: q (n, >= 3) the sharp then flat queries, coeff (n, 4) float32 and keep (n,)
    the tap's.  Rows, majorant, sums and units are scanmatch_ref's; only b is variant B's."""
    return R.reference_sums(pose32, q, coeff, keep=keep, b=odom_b(coeff, variant))


def pairwise32_odom(pose32, q, coeff, keep):
    """The fp32 floor: scanmatch_ref's float32 rows with numpy's pairwise float32 sums, b of variant B."""
    return R.rows32_pairwise_sums(pose32, q, coeff, keep=keep, b=odom_b(coeff))


# fp32 rows + numpy pairwise fp32 sum against sums64_odom, max over entries and families: measured by
# tests/test_odom_ref.py::test_fp32_floor_and_k_odom (asserted there to stay below this)
FLOOR_PAIRWISE_ODOM = 3.2


def k_odom_apriori():
    """Worst-case distance, in units u[k], of the device's sums from sums64_odom -- read out of the code (odom_sweep_kernel in
    csrc/lslam_kernels.hip, its second writing in odom_gn_kernel, csrc/lslam_solve_dev.hpp reduce_partials; the library is
    built without FMA contraction), counted the way scanmatch_ref.k_apriori counts:

      row entry   12   scanmatch_ref.ROW_UNITS (sin/cos 4 + 8 operations of jacobian_row, which both kernels call)
      b            2   -0.05 * d in float64, rounded once; d itself is the tap's input, so 1, counted as 2 (<= a row entry)
      product     2 * 12 + 1 = 25 (J^T J; J^T r has 12 + 2 + 1)
      wavefront    6   butterfly levels of wave_sum (__shfl_down 32 .. 1)
      block        3   additions over the four wavefronts, in fixed order
      across       0   blocks are added in float64 and the tap returns the float64 totals

    25 + 6 + 3 = 34.  Every rounding at its worst and as if all were aligned: a bound on correct code, not what it typically
    does (the measured values are in the tests' docstrings)."""
    return float((2 * R.ROW_UNITS + 1) + 6 + 3)


K_ODOM = max(10.0 * FLOOR_PAIRWISE_ODOM, k_odom_apriori())  # = 34: the derived value exceeds ten times the floor (32)


# ---------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------
POSE_ZERO = np.zeros(6, F32)
POSE_DRIVE = np.array([0.004, -0.006, 0.03, 0.35, 0.1, 0.02], F32)     # 0.4 m, 0.03 rad: what a sweep of a drive moves
POSE_LARGE = np.array([0.05, -0.04, 0.3, 3.2, -2.3, 0.4], F32)         # 4 m, 0.3 rad: many queries beyond the gate
ITERS = (0, 4, 5, 9, 24)
RAGGED = ((1, 0), (0, 1), (63, 65), (255, 257), (256, 256), (256, 16128), (300, 16200))


def scan_pair(synth, world, rings=16, steps=900, k=0):
    """Two consecutive sweeps of the synthetic scene: (last corner, last surf, corner, surf) of the second, all in scan
    (ring) order, float32 (n, 4)."""
    gt0 = (0.0, 0.0, 0.30 + 0.05 * k, 3.0, -2.0, synth.SENSOR_HEIGHT)
    gt1 = (0.002, -0.003, 0.33 + 0.05 * k, 3.35, -1.9, synth.SENSOR_HEIGHT)
    lc, ls, _ = synth.make_scan(world, rings, steps, gt_pose=gt0, seed=40 + k)
    c1, s1, _ = synth.make_scan(world, rings, steps, gt_pose=gt1, seed=41 + k)
    return lc, ls, c1, s1


def take(cloud, n, seed):
    """n points of the cloud in its order (a sorted random subset); more than it has: the cloud repeated with a jitter of
    a centimetre on the copies, sorted by ring so that it stays in scan order."""
    rng = np.random.default_rng(seed)
    if n <= len(cloud):
        return cloud[np.sort(rng.choice(len(cloud), n, replace=False))].copy()
    reps = [cloud]
    while sum(len(r) for r in reps) < n:
        c = cloud.copy()
        c[:, :3] += rng.normal(0, 0.01, (len(c), 3)).astype(F32)
        reps.append(c)
    out = np.concatenate(reps)[:n]
    return out[np.argsort(out[:, 3].astype(np.int64), kind="stable")].copy()


def with_reltime(cloud, frac):
    """The cloud with every point's relative time set to `frac` of a ring id step (intensity = ring + frac)."""
    out = cloud.copy()
    out[:, 3] = (np.floor(cloud[:, 3]) + F32(frac)).astype(F32)
    return out


def thin_voxels(cloud, leaf):
    """One point per cube of side `leaf` (the first in scan order), order kept."""
    key = np.floor(cloud[:, :3].astype(np.float64) / leaf).astype(np.int64)
    _, first = np.unique(key, axis=0, return_index=True)
    return cloud[np.sort(first)].copy()


def nn_dist(cloud, q):
    """float64 distance of every query from its nearest cloud point (family construction only)."""
    out = np.zeros(len(q))
    c = cloud[:, :3].astype(np.float64)
    for i in range(len(q)):
        out[i] = np.sqrt(((c - q[i, :3].astype(np.float64)) ** 2).sum(1).min())
    return out


def shifted(cloud, off):
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3] + np.asarray(off, F32)[None, :]).astype(F32)
    return out


def family(name, lc, ls, sharp, flat, pose, iters=(0,)):
    return dict(name=name, lc=np.ascontiguousarray(lc, F32), ls=np.ascontiguousarray(ls, F32),
                sharp=np.ascontiguousarray(sharp, F32), flat=np.ascontiguousarray(flat, F32), pose=np.asarray(pose, F32),
                iters=tuple(iters))


FAR_SHIFTS = (("far_3km", (3000.0, -2500.0, 0.0)),       # both grid levels usable, coarse float spacing
              ("far_10km", (10000.0, 9000.0, 0.0)),      # |coordinate| >= 8192 m: the fine level is refused
              ("far_50km", (50000.0, 0.0, 0.0)))         # >= 8192 * 5.02 m on one axis: both levels refused
# voxel leaf the last clouds of a far family are thinned with so that at most TIE_SHARE of its queries tie (0: as they are --
# tests/test_odom_ref.py counts the ties: none at these spacings, 2**-8 m at 50 km against 2 cm of range noise)
FAR_THIN = {"far_3km": 0.0, "far_10km": 0.0, "far_50km": 0.0}
TIE_SHARE = 0.02


def families(synth, world):
    """The input families of the issue's shapes, smallest that reach each path.  -> list of family()."""
    lc, ls, c1, s1 = scan_pair(synth, world, 16, 900)
    ls2 = ls[::2].copy()
    sharp, flat = take(c1, 160, 1), take(s1, 400, 2)
    out = []
    # ragged query counts, at the drive-sized step
    for ns, nf in RAGGED:
        small_ls = ls2 if nf < 1000 else take(ls, 1500, 7)  # (a small last cloud keeps the 16 000-query cases quick)
        out.append(family("ragged_%d_%d" % (ns, nf), lc, small_ls, take(c1, ns, 3), take(s1, nf, 4), POSE_DRIVE))
    # quirk Q5: a sharp count below most closest indices (the forward walk is empty), and one above the last cloud's size
    out.append(family("q5_few_sharp", lc, ls2, take(c1, 3, 5), take(s1, 40, 6), POSE_DRIVE))
    out.append(family("q5_more_sharp_than_cloud", lc[:120], ls2, take(c1, 200, 8), take(s1, 40, 9), POSE_DRIVE))
    # the guard's edge (:337): 11 corner and 101 surface points
    out.append(family("guard_edge", take(lc, 11, 10), take(ls, 101, 11), sharp[:60], flat[:120], POSE_DRIVE))
    # poses, iterations (weights off at 0 and 4, on from 5) and relative times
    out.append(family("pose_zero", lc, ls2, sharp, flat, POSE_ZERO, ITERS))
    out.append(family("pose_drive", lc, ls2, sharp, flat, POSE_DRIVE, ITERS))
    out.append(family("pose_large", lc, ls2, sharp, flat, POSE_LARGE, (0, 9)))
    out.append(family("reltime_0", lc, ls2, with_reltime(sharp, 0.0), with_reltime(flat, 0.0), POSE_LARGE))
    out.append(family("reltime_0999", lc, ls2, with_reltime(sharp, 0.0999), with_reltime(flat, 0.0999), POSE_DRIVE))
    # 64 rings
    lc6, ls6, c6, s6 = scan_pair(synth, world, 64, 450)
    out.append(family("rings_64", lc6, ls6[::4], take(c6, 160, 12), take(s6, 400, 13), POSE_DRIVE, (0, 5)))
    # the ring table: empty rings, ring 0 and ring 255, a cloud not in ring order, ring ids above 255
    def drop(c):
        return c[~np.isin(c[:, 3].astype(np.int64), (3, 4, 9))]
    out.append(family("empty_rings", drop(lc), drop(ls2), sharp, flat, POSE_DRIVE))
    def spread(c):  # rings 0 .. 13 as they are, 14 -> 254, 15 -> 255
        o = c.copy()
        r = np.floor(c[:, 3])
        o[:, 3] = (np.where(r >= 14, r + 240, r) + (c[:, 3] - r)).astype(F32)
        return o
    out.append(family("rings_0_to_255", spread(lc), spread(ls2), spread(sharp), spread(flat), POSE_DRIVE))
    rng = np.random.default_rng(5)
    out.append(family("not_ring_order", lc[rng.permutation(len(lc))], ls2[rng.permutation(len(ls2))], sharp, flat, POSE_DRIVE))
    up = np.array([0.0, 0.0, 0.0, 300.0], F32)
    out.append(family("rings_above_255", lc + up, ls2 + up, sharp + up, flat + up, POSE_DRIVE))
    # sparse last clouds: the nearest point 2 - 4.9 m away, so the fine level cannot prove and the ring table is scanned
    slc, sls = thin_voxels(lc, 3.0), thin_voxels(ls, 5.0)
    qs, qf = take(c1, min(len(c1), 400), 14), take(s1, 1500, 15)
    ds, df = nn_dist(slc, qs), nn_dist(sls, qf)
    out.append(family("sparse_2_to_4.9m", slc, sls, qs[(ds > 2.0) & (ds < 4.9)][:150], qf[(df > 2.0) & (df < 4.9)][:400],
                      POSE_ZERO))
    # equal distances inside the ring windows (never at the nearest point): last clouds on a 1/4 m lattice, every query 3 cm
    # off one of their points along x, zero pose -- the lattice neighbours mirrored in y or z lie at exactly the same distance,
    # and the walks' "first strictly smaller" decides
    def lattice(c):
        o = c.copy()
        o[:, :3] = (np.round(c[:, :3] * F32(4.0)) / F32(4.0)).astype(F32)
        _, first = np.unique(o[:, :3], axis=0, return_index=True)
        return o[np.sort(first)]
    tlc, tls = lattice(lc), lattice(ls2)
    off = np.array([0.03, 0.0, 0.0, 0.0], F32)
    out.append(family("walk_ties", tlc, tls, take(tlc, 120, 16) + off, take(tls, 300, 17) + off, POSE_ZERO))
    # far coordinates, zero pose
    for name, off in FAR_SHIFTS:
        leaf = FAR_THIN[name]
        a, b = (thin_voxels(lc, leaf), thin_voxels(ls2, leaf)) if leaf else (lc, ls2)
        out.append(family(name, shifted(a, off), shifted(b, off), shifted(sharp, off), shifted(flat, off), POSE_ZERO))
    return out
