"""An independent float64 / numpy statement of ScanRegistration::extractFeatures
(L_SLAM/src/odometry/ScanRegistration.cpp:190-666, helpers of util/math_utils.h:46-52,76-92).

It shares nothing with oracle/features_oracle.c or the kernels: it was written from the source alone, keeps the source's
structure (three marking loops, per-region picking loops, sequential Python where the source is sequential), computes every
compared quantity in float64 and carries, next to it, an ERROR BAND: how far the fp32 value the real code computes may lie
from the float64 one.  A ring is `ambiguous` when any quantity on a path that was actually taken lies inside its band --
picking is sequential, one flipped predicate may move every later pick of the ring, so the unit is the ring.

Bands.  u = 2^-24 (fp32 unit roundoff).  The arithmetic bands are 4 x a forward error bound derived in the docstring of the
function that computes the quantity:
    cos-angle (calcCosAngleDiff)           bound 10 u absolute            band 40 u = 2.4e-6
    squared difference (calcSquaredDiff)   bound  5 u relative            band 20 u relative
    diffPrev / diffNext                    bound 11 u relative            band 44 u relative
    depth (calcPointDistance)              bound 2.5 u relative           band 10 u (d1 + d2) on d1 - d2
    curvature                              bound E + 3 u (c + E), E = sum_c 2 |d_c| e_c + e_c^2,
                                           e_c = (2 cr + 1) u (2 cr |p_c| + sum_j |p_c(i+j)| + |p_c(i-j)|); band 4 x
    line distance                          bound |a| theta + (cr + 12) u max|p|; band 4 x
    voxel coordinate v * (1 / leaf)        bound u |v / leaf| (the product) band 4 u |v / leaf|
A quantity whose every fp32 intermediate is representable (dyadic rings) has bound 0: there fp32 and float64 agree exactly,
ties are ties in both.

The eigenvalues and the principal direction of pointClassify cannot be derived; they are MEASURED on the CPU, over the
fixture bank of features_cases.py, between oracle/lslam_oracle.c's solver fed with the fp32 covariance and
numpy.linalg.eigh of the float64 covariance (tests/test_features_ref.py::test_measured_eigen_bands re-measures and holds
the figures below; the kernel takes no part in it):
    largest |D_oracle - eigvalsh64| / lambda_max    = 6.43e-7     (MEASURED_EIG_REL; 8986 line fits)
    largest angle(principal direction, eigh's)      = 5.78e-8 rad (MEASURED_DIR_RAD; fits with lambda_2 > 100 lambda_1)
and 4 x each is the band (EIG_BAND = 2.57e-6 lambda_max, x 101 and x 10001 on the two gates; DIR_BAND = 2.31e-7 rad).  Nothing here imports the oracle, the package or reads the reference tree.
"""
import numpy as np

U = 2.0 ** -24

# measured over the bank (see the module docstring); bands are 4 x
MEASURED_EIG_REL = 6.43e-7
MEASURED_DIR_RAD = 5.78e-8
EIG_BAND = 4 * MEASURED_EIG_REL
DIR_BAND = 4 * MEASURED_DIR_RAD

# PointLabel, ScanRegistration.h:22-42
UNKNOW, SURF_PICKED_NEAR, CORNER_SHARP, SURFACE_LESS_FLAT, SURFACE_FLAT = 6, 3, 1, 0, -1
ONESIDE_FLAT, EDGE_BROKEN, NEAR_BLOCK, BLIND_BLOCK, MESSY = 5, -2, -3, -4, 9

COS175, COS5 = np.cos(np.deg2rad(175.0)), np.cos(np.deg2rad(5.0))      # :653, evaluated in double
COS135, COS45 = np.cos(np.deg2rad(135.0)), np.cos(np.deg2rad(45.0))    # :655


class Params:
    """RegistrationParams defaults, ScanRegistration.h:49-57; blindThreshold = cos(deg2rad(float 0.5)) stored in a float
    (ScanRegistration.cpp:27, math_utils.h:37)."""

    def __init__(self, **kw):
        self.n_feature_regions = 6
        self.curvature_region = 5
        self.max_corner_sharp = 2
        self.max_surface_flat = 4
        self.less_flat_filter_size = 0.2
        self.surface_curvature_threshold = 0.02
        self.blind_threshold = float(np.float32(np.cos(np.float64(np.float32(0.5 * np.pi / 180.0)))))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(k)
            setattr(self, k, v)

    def apply(self, obj):
        """copy the fields onto another parameter object with the same field names (a ctypes struct)"""
        for k, v in vars(self).items():
            setattr(obj, k, v)
        return obj


def f32(x):
    return float(np.float32(x))


def _rep(x):
    """is the float64 value representable in fp32?"""
    return float(np.float32(x)) == float(x)


class Trace:
    """Collects what one ring did: ambiguity (a compared quantity inside its band) and named events for the bank's coverage
    counts."""

    def __init__(self):
        self.ambiguous = False
        self.why = []
        self.events = {}

    def hit(self, name, n=1):
        self.events[name] = self.events.get(name, 0) + n

    def less(self, q, thr, band, what):
        """q < thr, as the source writes it; flags the ring when |q - thr| <= band and band > 0 (band 0: exact)"""
        if band > 0 and abs(q - thr) <= band:
            self.ambiguous = True
            self.why.append((what, q, thr, band))
        return q < thr


# ---- util/math_utils.h -------------------------------------------------------------------------------------------------
def calc_squared_diff(a, b):
    """math_utils.h:46-52.  fp32 sequence: three subtractions (1 rounding each), three squares (the rounded difference
    squared: 2 u + u), two additions of positive terms (+ 2 u): every term carries at most 5 roundings -> relative bound 5 u.
    Returns (value, bound)."""
    d = a - b
    v = float(d @ d)
    exact = all(_rep(x) for x in d) and all(_rep(x * x) for x in d) and _rep(d[0] * d[0] + d[1] * d[1]) and _rep(v)
    return v, (0.0 if exact else 5 * U * v)


def calc_point_distance(p):
    """math_utils.h:76-78.  Sum of three squares of exact inputs (3 roundings per term, all positive: 3 u relative), sqrt
    halves it and rounds once: 1.5 u + u = 2.5 u relative.  Returns (value, bound)."""
    v = float(np.sqrt(p @ p))
    return v, 2.5 * U * v


def calc_cos_angle_diff(a, b):
    """math_utils.h:86-92.  ab: three products and two additions, |error| <= 3 u sum|a_i b_i| <= 3 u |a||b|; the two
    distances 2.5 u each, their product one more rounding: 6 u; the division one: |cos| (6 u + u) <= 7 u.  Together
    <= 10 u ABSOLUTE.  (cos 0.5 deg is 3.8e-5 below 1: the band 40 u = 2.4e-6 is 6 % of that.)  Returns (value, bound)."""
    v = float(a @ b) / (float(np.sqrt(a @ a)) * float(np.sqrt(b @ b)))
    return v, 10 * U


# ---- setScanBuffersFor, :462-522 ----------------------------------------------------------------------------------------
def scan_marks(xyz, cr, blind_thr, tr=None):
    """_scanNeighborPicked of one ring after setScanBuffersFor.  xyz: (n, 3) float64 of the ring (startIdx = 0,
    endIdx = n - 1).  Three loops in source order; fill_n with the source's start indices and lengths."""
    tr = tr if tr is not None else Trace()
    n = len(xyz)
    end = n - 1
    picked = [0] * n                                                     # :466

    def fill_n(first, count, value):
        assert 0 <= first and first + count <= n, (first, count, n)      # the source would write out of the buffer
        for q in range(first, first + count):
            picked[q] = value

    def blind(a, b):
        c, bound = calc_cos_angle_diff(xyz[a], xyz[b])
        return tr.less(c, blind_thr, 4 * bound, "blind")

    for i in range(cr):                                                  # :468-475
        if blind(i, i + 1):
            fill_n(i, cr + 1, BLIND_BLOCK)
            tr.hit("blind_first_loop")
    for i in range(cr):                                                  # :476-484
        if blind(end - i, end - i - 1):
            fill_n(end - i - cr, cr + 1, BLIND_BLOCK)
            tr.hit("blind_last_loop")
    last_blind = last_disc = None
    i = cr                                                               # :487-488, startIdx = 0
    while i < end - cr:
        prev_p, p, next_p = xyz[i - 1], xyz[i], xyz[i + 1]
        diff_next, b_next = calc_squared_diff(next_p, p)                 # :493
        if blind(i, i + 1):                                              # :494-499
            if any(v in (NEAR_BLOCK, EDGE_BROKEN) for v in picked[i - cr + 1:i + cr + 1]):
                tr.hit("blind_over_near_block")
            fill_n(i - cr + 1, cr * 2, BLIND_BLOCK)
            tr.hit("blind_main_loop")
            if last_blind is not None and i - last_blind <= 2 * cr:
                tr.hit("blind_pair_within_2cr")
            if last_disc is not None and i - last_disc == 1:
                tr.hit("blind_after_discontinuity")
            last_blind = i
            i += 1
            continue
        if not tr.less(1.0, diff_next, 4 * b_next, "diffNext"):          # :501  diffNext > 1.0
            i += 1
            continue
        depth1, b1 = calc_point_distance(p)                              # :502-504
        depth2, b2 = calc_point_distance(next_p)
        diff_prev, b_prev = calc_squared_diff(prev_p, p)
        ratio = diff_prev / diff_next
        # two squared differences of 5 u each and the division's rounding: 11 u relative (0 when all three are exact)
        ratio_band = 0.0 if (b_prev == 0 and b_next == 0 and _rep(ratio)) else 44 * U * ratio
        if last_disc is not None:
            tr.hit("disc_spacing_%d" % min(i - last_disc, cr + 2))
        if last_blind is not None and i - last_blind == 1:
            tr.hit("discontinuity_after_blind")
        far_to_near = tr.less(depth2, depth1, 4 * (b1 + b2), "depth")    # :505  depth1 > depth2
        tr.hit("far_to_near" if far_to_near else "near_to_far")
        if last_disc is not None and i - last_disc <= cr + 1:
            # fn: far-to-near jump, nf: near-to-far; fn_nf is a pole in front of a wall, nf_fn a window in a near wall
            tr.hit("pair_%s_%s" % ("fn" if last_far_to_near else "nf", "fn" if far_to_near else "nf"))
        target = i + 1 if far_to_near else i                             # :506-508 / :514-516
        if picked[target] > NEAR_BLOCK:
            if tr.less(ratio, 0.2, ratio_band, "ratio"):
                picked[target] = EDGE_BROKEN
                tr.hit("ratio_taken")
            else:
                tr.hit("ratio_refused")
        else:
            tr.hit("edge_refused_by_guard")
        first = i - cr + 1 if far_to_near else i + 1                     # :509-511 / :517-518
        if EDGE_BROKEN in picked[first:first + cr]:
            tr.hit("edge_overwritten_by_near_block")
        fill_n(first, cr, NEAR_BLOCK)
        last_disc, last_far_to_near = i, far_to_near
        i += 1
    return picked


# ---- setRegionBuffersFor, :420-460 --------------------------------------------------------------------------------------
def curvature(xyz, cr):
    """:430-444 for every point of a ring that has cr neighbours on both sides -> (c, bound), zeros elsewhere"""
    c, b = np.zeros(len(xyz)), np.zeros(len(xyz))
    for i in range(cr, len(xyz) - cr):
        c[i], b[i], _ = curvature_at(xyz, i, cr)
    return c, b


def curvature_at(xyz, i, cr):
    """:430-443 for point i.  Per coordinate: diff = -2cr * p (1 rounding), then cr times diff += (p[i+j] + p[i-j]) (2
    roundings each): 2 cr + 1 roundings over S = 2 cr |p| + sum |p[i+j]| + |p[i-j]| -> e <= (2 cr + 1) u S.  The squares
    and the two additions put at most 3 more roundings on each positive term: bound = E + 3 u (c + E) with
    E = sum_c 2 |d_c| e_c + e_c^2.  Sums whose every intermediate is representable in fp32 are exact (e = 0); when the squares
    and their sum are representable too the bound is 0.  Returns (c, bound, key): two points with exact sums and the same
    key (|d| per coordinate) go through the same fp32 squares and additions -- a tie in fp32 whatever the squares round to."""
    w = -2.0 * cr
    d = w * xyz[i]
    s = np.abs(d)
    sums_exact = all(_rep(x) for x in d)
    for j in range(1, cr + 1):
        t = xyz[i + j] + xyz[i - j]
        d = d + t
        s = s + np.abs(xyz[i + j]) + np.abs(xyz[i - j])
        sums_exact = sums_exact and all(_rep(x) for x in t) and all(_rep(x) for x in d)
    sq = d * d
    c = float((sq[0] + sq[1]) + sq[2])
    key = tuple(np.abs(d)) if sums_exact else None
    if sums_exact and all(_rep(x) for x in sq) and _rep(sq[0] + sq[1]) and _rep(c):
        return c, 0.0, key
    e = np.zeros(3) if sums_exact else (2 * cr + 1) * U * s
    E = float(np.sum(2 * np.abs(d) * e + e * e))
    return c, E + 3 * U * (c + E), key


def region_bounds(start, end, cr, nf, j):
    """:249-257, size_t arithmetic (unsigned 64-bit, the `- 1` may wrap)."""
    M = (1 << 64) - 1
    sp = (((start + cr) * (nf - j) + (end - cr) * j) & M) // nf
    ep = ((((start + cr) * (nf - 1 - j) + (end - cr) * (j + 1)) & M) // nf - 1) & M
    return sp, ep


# ---- pointClassify, :547-666 --------------------------------------------------------------------------------------------
def _one_sided_line(pts, tr, detail):
    """One half of pointClassify (:558-601 / :603-648) over the cr + 1 points `pts` (float64).  -> (is_line, direction)"""
    m = len(pts)
    centroid = pts.sum(0) / m                                            # :559-563
    a = pts - centroid
    A = a.T @ a / m                                                      # :566-577 (lower triangle of the same matrix)
    D, V = np.linalg.eigh(A)                                             # :582-584, ascending
    lam = max(D[2], 0.0)
    band = EIG_BAND * lam
    detail.append(dict(D=D.copy(), v=V[:, 2].copy(), A=A, pts=pts, dist=[]))
    g1 = tr.less(100 * D[1], D[2], band * 101, "eig100")                 # :587
    if not g1:
        return False, None
    g2 = tr.less(10000 * D[0], D[2], band * 10001, "eig10000")           # :588
    if not g2:
        return False, None
    v = V[:, 2]
    pmax = float(np.abs(pts).max())
    for q in range(m):                                                   # :591-600
        # |a x v| / |v|: the direction is off by at most DIR_BAND / 4 = theta, which moves the distance by |a| theta; the
        # centroid (m additions and a division) and the subtraction put (m + 2) u max|p| on a, cross product, norm and
        # division 10 u |a| <= 10 u max|p|: bound |a| theta + (cr + 12) u max|p|
        dist = float(np.linalg.norm(np.cross(a[q], v)) / np.linalg.norm(v))
        bound = float(np.linalg.norm(a[q])) * MEASURED_DIR_RAD + (m + 11) * U * pmax
        detail[-1]["dist"].append(dist)
        if tr.less(0.08, abs(dist), 4 * bound, "dist"):                  # :596
            return False, None
    return True, v


def point_classify(xyz, i, cr, tr=None, detail=None):
    """pointClassify(i): backward window i, i-1 ... i-cr (:557-602), forward window i+cr ... i (:603-649)."""
    tr = tr if tr is not None else Trace()
    detail = detail if detail is not None else []
    line1, v1 = _one_sided_line(xyz[[i - j for j in range(cr + 1)]], tr, detail)
    line2, v2 = _one_sided_line(xyz[[i - j for j in range(-cr, 1)]], tr, detail)
    if line1 and line2:                                                  # :651-658
        diff, b = calc_cos_angle_diff(v1, v2)
        band = 2 * DIR_BAND + 4 * b                                      # each direction off by theta: the angle by 2 theta
        detail.append(dict(diff=diff))
        c1 = tr.less(diff, COS175, band, "cos175")
        c2 = (not c1) and tr.less(COS5, diff, band, "cos5")
        if c1 or c2:
            tr.hit("flat_by_cos175" if c1 else "flat_by_cos5")
            return SURFACE_FLAT
        if tr.less(COS135, diff, band, "cos135") and tr.less(diff, COS45, band, "cos45"):
            return CORNER_SHARP
    return ONESIDE_FLAT if (line1 or line2) else MESSY                   # :659-663


# ---- pcl::VoxelGrid<PointXYZI>::applyFilter -----------------------------------------------------------------------------
def voxel_grid(pts, leaf, tr=None):
    """PCL's VoxelGrid over (n, 4) float64 rows {x, y, z, field}, leaf a float: inverse_leaf = 1 / leaf (a float); min / max
    of the cloud; if the index volume ((max - min) * inverse_leaf truncated, + 1, per axis, multiplied) exceeds INT_MAX the
    cloud is handed back unfiltered; else cell = floor(v * inverse_leaf) - floor(min * inverse_leaf) per axis, linear index
    with x fastest, one centroid of all four fields per occupied cell, in ascending index order.
    -> (centroids (m, 4) float64, point count per centroid, members: list of row-index arrays)"""
    tr = tr if tr is not None else Trace()
    n = len(pts)
    if n == 0:
        return np.zeros((0, 4)), np.zeros(0, int), []
    inv = f32(1.0 / f32(leaf))      # one correctly rounded fp32 division of two floats: the real code holds this very value
    mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
    vol = 1
    for d in range(3):
        vol *= int((mx[d] - mn[d]) * inv) + 1
    if abs(vol - (2 ** 31 - 1)) < 1e-5 * 2 ** 31:
        tr.ambiguous = True
    if vol > 2 ** 31 - 1:
        tr.hit("voxel_guard")
        return pts.copy(), np.ones(n, int), [np.array([k]) for k in range(n)]

    def cell(v, note=False):
        """floor(v * inverse_leaf): the product is the one rounding (bound u |q|, band 4 u |q|; 0 when it is representable)"""
        q = v * inv
        if not _rep(q):
            tr.less(q, float(np.round(q)), 4 * U * abs(q), "voxel")     # a product within its band of an integer
        elif note and q == np.floor(q) and v != 0:
            tr.hit("voxel_point_on_boundary")
        return int(np.floor(q))

    min_b = [cell(mn[d]) for d in range(3)]
    div_b = [cell(mx[d]) - min_b[d] + 1 for d in range(3)]
    idx = np.array([(cell(p[0], True) - min_b[0]) + (cell(p[1], True) - min_b[1]) * div_b[0] + (cell(p[2]) - min_b[2]) * div_b[0] * div_b[1]
                    for p in pts])
    cells = np.unique(idx)                                               # ascending
    members = [np.nonzero(idx == c)[0] for c in cells]
    out = np.array([pts[m].mean(0) for m in members])
    cnt = np.array([len(m) for m in members])
    if len(cells) == 1 and n > 1:
        tr.hit("voxel_single")
    if len(cells) == n and n > 1:
        tr.hit("voxel_all_own")
    if 1 < len(cells) < n:
        tr.hit("voxel_mixed")
    return out, cnt, members


# ---- extractFeatures, :190-418 ------------------------------------------------------------------------------------------
def extract(cloud, ranges, params=None, field=3):
    """cloud: (n, >= 4) float32, ranges: (rings, 2) inclusive.  -> dict
        picked        int8 (n)   marks after setScanBuffersFor (what the device's tap shows)
        label         int8 (n)   _regionLabel, UNKNOW where no region was processed
        curvature, curvature_bound   float64 (n), 0 outside every processed region
        sharp, less_sharp, flat      cloud indices, in output order
        less_flat_pre                cloud indices of every ring's list before its VoxelGrid, in push order
        less_flat                    (m, 4) float64 centroids; less_flat_ring, less_flat_count, less_flat_members per row
        ring_of_*                    ring number per entry of the three index lists
        fits          one dict per one-sided line fit of pointClassify: pts (window, in accumulation order), A, D, v, dist
        ambiguous     bool (rings); why: per ring, the quantities that fell inside their band
        events        per ring, dict name -> count"""
    p = params if params is not None else Params()
    cr, nf = int(p.curvature_region), int(p.n_feature_regions)
    thr = f32(p.surface_curvature_threshold)
    blind_thr = f32(p.blind_threshold)
    cloud = np.asarray(cloud)
    assert cloud.dtype == np.float32
    xyz_all = cloud[:, :3].astype(np.float64)
    n = len(cloud)
    out = dict(picked=np.zeros(n, np.int8), label=np.full(n, UNKNOW, np.int8), curvature=np.zeros(n), curvature_bound=np.zeros(n),
               sharp=[], less_sharp=[], flat=[], less_flat_pre=[], ring_of_sharp=[], ring_of_less_sharp=[], ring_of_flat=[],
               ring_of_less_flat_pre=[], less_flat=[], less_flat_ring=[], less_flat_count=[], less_flat_members=[],
               fits=[], ambiguous=np.zeros(len(ranges), bool), why=[[] for _ in ranges], events=[{} for _ in ranges])

    for ring, (start, end) in enumerate(np.asarray(ranges).tolist()):
        tr = Trace()
        out["events"][ring] = tr.events
        if end <= start + 2 * cr:                                        # :205-207
            tr.hit("ring_skipped")
            if end == start + 2 * cr:
                tr.hit("ring_skipped_at_2cr_plus_1")
            if end < start:
                tr.hit("ring_empty")
            continue
        tr.hit("ring_processed")
        if end == start + 2 * cr + 1:
            tr.hit("ring_smallest_processed")
        if end - start + 1 == 2560:
            tr.hit("ring_2560")
        xyz = xyz_all[start:end + 1]
        picked = scan_marks(xyz, cr, blind_thr, tr)                      # :210
        out["picked"][start:end + 1] = picked
        less_flat_scan = []

        for j in range(nf):                                              # :248
            sp, ep = region_bounds(start, end, cr, nf, j)
            if ep <= sp:                                                 # :260
                tr.hit("region_skipped")
                continue
            size = ep - sp + 1
            tr.hit("region_of_2" if size == 2 else "region")
            # setRegionBuffersFor(sp, ep), :420-460
            cb = [curvature_at(xyz, i - start, cr) for i in range(sp, ep + 1)]
            curv = np.array([c for c, b, key in cb])
            bound = np.array([b for c, b, key in cb])
            out["curvature"][sp:ep + 1] = curv
            out["curvature_bound"][sp:ep + 1] = bound
            c32 = curv.astype(np.float32)
            order = np.argsort(c32, kind="stable") + sp                  # mergeSort with `<=`: ascending, ties by index
            label = [UNKNOW] * size
            below = [tr.less(curv[r], thr, 4 * bound[r], "curvature") for r in range(size)]
            if bound.max() > 0:
                # the order itself is a chain of comparisons: two curvatures closer than their bands may swap
                srt = np.argsort(curv, kind="stable")
                for a, b in zip(srt[:-1], srt[1:]):
                    same = cb[a][2] is not None and cb[a][2] == cb[b][2]
                    if not same and (bound[a] > 0 or bound[b] > 0) and curv[b] - curv[a] <= 4 * (bound[a] + bound[b]):
                        tr.ambiguous = True
                        tr.why.append(("order", curv[a], curv[b], 4 * (bound[a] + bound[b])))
                        break
            vals, counts = np.unique(c32, return_counts=True)
            for v, c in zip(vals, counts):
                if c >= 8:
                    tr.hit("tie_zero" if v == 0 else ("tie_below" if v < thr else "tie_above"))
            if len(vals) == 1 and vals[0] == 0:
                tr.hit("region_all_zero")

            def mark_as_picked(scan_idx):                                # :524-545
                picked[scan_idx] = SURF_PICKED_NEAR
                for q in range(1, cr + 1):
                    picked[scan_idx + q] = SURF_PICKED_NEAR
                for q in range(1, cr + 1):
                    picked[scan_idx - q] = SURF_PICKED_NEAR

            # flat surface features, :268-284
            surf_picked = 0
            k = 0
            while k < size and surf_picked < p.max_surface_flat:
                idx = int(order[k])
                scan_idx, region_idx = idx - start, idx - sp
                if picked[scan_idx] != SURF_PICKED_NEAR and below[region_idx]:
                    surf_picked += 1
                    label[region_idx] = SURFACE_FLAT
                    out["flat"].append(idx)
                    out["ring_of_flat"].append(ring)
                    if k + 1 < size and c32[order[k + 1] - sp] == c32[region_idx]:
                        tr.hit("flat_pick_among_ties")
                    mark_as_picked(scan_idx)
                elif picked[scan_idx] == SURF_PICKED_NEAR and below[region_idx]:
                    tr.hit("flat_excluded_by_mark")
                k += 1
            if surf_picked == p.max_surface_flat:
                tr.hit("flat_cap_reached")

            # less flat surface features and broken edges, :286-303
            for k in range(size):
                idx = sp + k
                scan_idx = idx - start
                if below[k]:
                    less_flat_scan.append(idx)
                    if label[k] != SURFACE_FLAT:
                        label[k] = SURFACE_LESS_FLAT
                if picked[scan_idx] == EDGE_BROKEN:
                    out["sharp"].append(idx)
                    out["less_sharp"].append(idx)
                    out["ring_of_sharp"].append(ring)
                    out["ring_of_less_sharp"].append(ring)
                    label[k] = CORNER_SHARP
                    tr.hit("edge_broken_feature")

            # classified features in descending curvature, :305-387
            corner_picked = 0
            surf_picked = 0
            surf_from_flat = 0
            k = size
            while k > 0:
                k -= 1
                idx = int(order[k])
                scan_idx, region_idx = idx - start, idx - sp
                if below[region_idx]:                                    # :313-314
                    break
                if k > 0 and c32[order[k - 1] - sp] == c32[region_idx]:
                    tr.hit("classified_among_ties")
                det = []
                verdict = point_classify(xyz, scan_idx, cr, tr, det)
                out["fits"] += [d for d in det if "pts" in d]
                tr.hit("verdict_%d" % verdict)
                if verdict == SURFACE_FLAT:                              # :322-331
                    label[region_idx] = SURFACE_FLAT
                    if surf_picked < p.max_surface_flat:
                        surf_picked += 1
                        surf_from_flat += 1
                    less_flat_scan.append(idx)
                elif verdict == CORNER_SHARP:                            # :332-343
                    if picked[scan_idx] > EDGE_BROKEN:
                        label[region_idx] = CORNER_SHARP
                        if corner_picked < p.max_corner_sharp:
                            corner_picked += 1
                            out["sharp"].append(idx)
                            out["ring_of_sharp"].append(ring)
                        else:
                            tr.hit("corner_over_cap")
                        out["less_sharp"].append(idx)
                        out["ring_of_less_sharp"].append(ring)
                    elif picked[scan_idx] == EDGE_BROKEN:
                        tr.hit("corner_on_edge_broken")
                    else:
                        tr.hit("corner_on_block_mark")
                elif verdict == ONESIDE_FLAT:                            # :344-353
                    label[region_idx] = ONESIDE_FLAT
                    if surf_picked < p.max_surface_flat:
                        surf_picked += 1
                        out["flat"].append(idx)
                        out["ring_of_flat"].append(ring)
                    elif surf_from_flat > 0:
                        tr.hit("oneside_refused_by_shared_cap")
                    less_flat_scan.append(idx)
            out["label"][sp:ep + 1] = label

        # :390-399: VoxelGrid of this ring's less-flat points; the copied field is the cloud's `field` column
        out["less_flat_pre"] += less_flat_scan
        out["ring_of_less_flat_pre"] += [ring] * len(less_flat_scan)
        rows = np.concatenate([xyz_all[less_flat_scan], cloud[less_flat_scan, field:field + 1].astype(np.float64)], 1) \
            if less_flat_scan else np.zeros((0, 4))
        cent, cnt, members = voxel_grid(rows, p.less_flat_filter_size, tr)
        out["less_flat"].append(cent)
        out["less_flat_ring"] += [ring] * len(cent)
        out["less_flat_count"] += cnt.tolist()
        out["less_flat_members"] += [np.asarray(less_flat_scan)[m] for m in members]
        out["ambiguous"][ring] = tr.ambiguous
        out["why"][ring] = tr.why

    out["less_flat"] = np.concatenate(out["less_flat"]) if out["less_flat"] else np.zeros((0, 4))
    for k in ("sharp", "less_sharp", "flat", "less_flat_pre", "ring_of_sharp", "ring_of_less_sharp", "ring_of_flat",
              "ring_of_less_flat_pre", "less_flat_ring", "less_flat_count"):
        out[k] = np.asarray(out[k], np.int64)
    return out
