"""The constructed fixture bank of the feature-extraction tests: a 2-D sensor at the origin sweeps one ring in equal azimuth
steps across hand-placed walls, poles and gaps -- no range noise.  Every coordinate is snapped to a multiple of 2^-8 m
(|coordinate| < 64 m), so the curvature sums are exact in fp32 and a tie is a tie in both precisions; the walls that want
whole regions of equal curvature are laid out on the dyadic grid directly (equal Cartesian spacing).

bank() -> list of Call(name, params, cloud, ranges): one Call is one launch (at most 64 rings); REQUIRED names the events
(features_ref.Trace) that the reference must reach on unambiguous rings, with the least count."""
import numpy as np

from features_ref import Params

SNAP = 2.0 ** -8
Z = 0.0      # the sensor's own plane: at any other height the angle between two returns would depend on their ranges


class Call:
    def __init__(self, name, params, rings, limit=64.0):
        self.name, self.params = name, params
        pts, ranges, at = [], [], 0
        for k, r in enumerate(rings):
            n = len(r)
            if n == 0:
                ranges.append([at, at - 1])                             # an empty ring {n, n - 1}
                continue
            c = np.zeros((n, 4), np.float32)
            c[:, :3] = r
            c[:, 3] = np.float32(k) + (np.arange(n) / np.float32(4 * n)).astype(np.float32)  # ring + relative time
            pts.append(c)
            ranges.append([at, at + n - 1])
            at += n
        self.cloud = np.concatenate(pts)
        self.ranges = np.array(ranges, np.int32)
        assert len(rings) <= 64 and np.abs(self.cloud[:, :3]).max() < limit


def snap(p):
    q = np.round(np.asarray(p, np.float64) / SNAP) * SNAP
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
    return q


def ring_from_ranges(az_deg, rng):
    """returns of the beams that have one (range > 0), snapped"""
    az = np.deg2rad(np.asarray(az_deg, np.float64))
    keep = rng > 0
    p = np.stack([rng * np.cos(az), rng * np.sin(az), np.full(len(az), Z)], 1)[keep]
    return snap(p)


def beams(n, step, centre=0.0):
    return centre + (np.arange(n) - (n - 1) / 2.0) * step


def cast(az_deg, segments):
    """range per beam to the nearest of the segments ((x0, y0), (x1, y1)); 0 where nothing is hit"""
    az = np.deg2rad(np.asarray(az_deg, np.float64))
    out = np.zeros(len(az))
    for (x0, y0), (x1, y1) in segments:
        ex, ey = x1 - x0, y1 - y0
        for k, a in enumerate(az):
            dx, dy = np.cos(a), np.sin(a)
            det = dx * (-ey) - dy * (-ex)
            if abs(det) < 1e-12:
                continue
            r = (x0 * (-ey) - y0 * (-ex)) / det
            s = (dx * y0 - dy * x0) / det
            if r > 0 and -1e-9 <= s <= 1 + 1e-9 and (out[k] == 0 or r < out[k]):
                out[k] = r
    return out


def wall_x(az_deg, x):
    return x / np.cos(np.deg2rad(az_deg))


# ---- the rings ----------------------------------------------------------------------------------------------------------
def pole_ring(w, gap=None, w2=3, n=160, step=0.3, window=False):
    """a wall at x = 10 with a pole `w` returns wide at 5 m (window: a wall at 5 m with a hole `w` returns wide); with `gap`,
    a second pole of w2 returns `gap` wall returns after the first"""
    az = beams(n, step)
    far, near = wall_x(az, 10.0), wall_x(az, 5.0)
    rng = near.copy() if window else far.copy()
    a = n // 2 - 10
    spans = [(a, a + w)] + ([(a + w + gap, a + w + gap + w2)] if gap is not None else [])
    for lo, hi in spans:
        rng[lo:hi] = far[lo:hi] if window else 5.0
    return ring_from_ranges(az, rng)


def ratio_ring(n=120, step=0.3):
    """a pole one return wide 4 m in front of the wall (both neighbours of its return are far away: diffPrev / diffNext ~ 1,
    not below 0.2) and a step of 1.5 m back and forth (0.05 m to the previous point: ratio ~ 0.001)"""
    az = beams(n, step)
    rng = wall_x(az, 10.0)
    rng[30] = rng[30] - 4.0            # single return: both neighbours are far away, ratio ~ 1
    rng[60:] = rng[60:] + 1.5          # a step back of 1.5 m: the spacing before it is 0.05 m, ratio ~ 0.001
    rng[90:] = rng[90:] - 1.5
    return ring_from_ranges(az, rng)


def blind_ring(drops, n=160, step=0.3, pole=None):
    """wall at x = 10; the beams listed in `drops` have no return (two missing beams in a row: 0.9 deg to the next point)"""
    az = beams(n, step)
    rng = wall_x(az, 10.0)
    if pole is not None:
        rng[pole[0]:pole[1]] = 5.0
    rng[list(drops)] = 0
    return ring_from_ranges(az, rng)


def tie_wall(n=200, x=10.0, pitch=2.0 ** -4, y0=None, pattern=None, h=2.0 ** -5):
    """equally spaced points on the dyadic grid along y; `pattern` (0 / 1 per point, repeated) sets some back by h"""
    y0 = -(n // 2) * pitch if y0 is None else y0
    p = np.zeros((n, 3))
    p[:, 0] = x
    p[:, 1] = y0 + np.arange(n) * pitch
    p[:, 2] = Z
    if pattern is not None:
        p[:, 0] += h * np.array([pattern[k % len(pattern)] for k in range(n)])
    return snap(p)


def density_wall(n=180, x=10.0):
    """a straight dyadic wall whose point spacing alternates between 2^-5 and 2^-4 m every 15 points: high curvature along
    the wall at every change, both half-lines parallel -- SURFACE_FLAT through pointClassify"""
    dy = np.where((np.arange(n) // 15) % 2 == 0, 2.0 ** -5, 2.0 ** -4)
    p = np.zeros((n, 3))
    p[:, 0] = x
    p[:, 1] = -4.0 + np.cumsum(dy)
    p[:, 2] = Z
    return snap(p)


def sawtooth_ring(n=240, step=0.25, period=2.0, x=9.0, depth=1.0):
    """a wall whose plan is a sawtooth of right angles (faces at +-45 deg to the x = const line): many corners per region"""
    az = beams(n, step)
    segs = []
    y = -8.0
    while y < 8.0:
        segs.append(((x, y), (x + depth, y + period / 2)))
        segs.append(((x + depth, y + period / 2), (x, y + period)))
        y += period
    return ring_from_ranges(az, cast(az, segs))


def room_ring(n=360, step=0.4, half=6.0, centre=0.0):
    """inside a square room, seen over n * step degrees: right-angle corners between long walls"""
    az = beams(n, step, centre)
    h = half
    segs = [((h, -h), (h, h)), ((h, h), (-h, h)), ((-h, h), (-h, -h)), ((-h, -h), (h, -h))]
    return ring_from_ranges(az, cast(az, segs))


def grazing_ring(n=140, step=0.2):
    """a wall x = 5 that ends on the beam of azimuth 0 at P = (5, 0); behind it a grazing wall through P (direction (1, 0.02))
    of which the next beams see points more than 1 m from P and from one another; a back wall at x = 45 behind that.  P
    is the last point before a near-to-far jump (EDGE_BROKEN) and the end of two lines 89 deg apart (CORNER_SHARP)."""
    az = beams(n, step, centre=(0.5 - (n % 2) / 2.0) * step)
    k0 = int(np.argmin(np.abs(az)))
    assert abs(az[k0]) < 1e-9
    rng = np.where(az <= 1e-9, wall_x(az, 5.0), 0.0)
    t = 0.02
    for k in range(k0 + 1, n):
        ta = np.tan(np.deg2rad(az[k]))
        s = 5.0 * ta / (t - ta) if ta < t else -1.0
        if 0 < s < 36.0:
            rng[k] = np.hypot(5.0 + s, s * t)
        else:
            rng[k] = 45.0 / np.cos(np.deg2rad(az[k]))
    return ring_from_ranges(az, rng)


def short_ring(npts, x=10.0, pitch=2.0 ** -4):
    return tie_wall(npts, x=x, pitch=pitch, y0=1.0)


def short_gap_ring(npts, at=2):
    """a short ring with a blind gap (0.25 m at 10 m: 1.4 deg) after point `at`: if the ring is processed at all, an end loop
    marks it"""
    p = short_ring(npts)
    p[at + 1:, 1] += 0.25
    return snap(p)


def big_ring(n=2560):
    az = beams(n, 360.0 / n)
    h = 7.0
    segs = [((h, -h), (h, h)), ((h, h), (-h, h)), ((-h, h), (-h, -h)), ((-h, -h), (h, -h))]
    return ring_from_ranges(az, cast(az, segs))


# ---- the calls ----------------------------------------------------------------------------------------------------------
def _marks_rings(cr):
    rings = []
    for w in range(1, cr + 2):
        rings += [pole_ring(w), pole_ring(w, window=True)]
    for gap in range(1, cr + 2):
        rings += [pole_ring(3, gap=gap), pole_ring(3, gap=gap, window=True)]
    rings.append(ratio_ring())
    rings += [blind_ring([2, 3]), blind_ring([156, 157]), blind_ring([1, 2, 157, 158]),
              blind_ring([66, 67], pole=(69, 75)), blind_ring([76, 77], pole=(69, 75)),
              blind_ring([60, 61, 66, 67]), blind_ring([60, 61, 70, 71]), blind_ring([80, 81])]
    return rings


def _classify_rings():
    return [sawtooth_ring(), sawtooth_ring(period=1.5, depth=0.75), sawtooth_ring(n=300, step=0.2, period=1.0, depth=0.5, x=7.0),
            room_ring(), room_ring(centre=37.0), room_ring(half=5.0, centre=-20.0), density_wall(), density_wall(x=12.0),
            grazing_ring()]


def _tie_rings():
    return [tie_wall(200), tie_wall(200, pattern=[0, 0, 1]), tie_wall(230, x=12.0, pattern=[0, 0, 1]),
            tie_wall(200, pattern=[0, 1, 0, 0, 1, 1]), density_wall()]


def _edge_rings(cr):
    return [short_ring(2 * cr + 1), short_ring(2 * cr + 2), np.zeros((0, 3)), short_ring(2 * cr + 3), tie_wall(100, y0=1.0),
            short_ring(2 * cr + 2, x=11.0), short_gap_ring(2 * cr + 1, at=0), short_gap_ring(2 * cr + 2, at=0),
            short_gap_ring(2 * cr + 2, at=2 * cr)]


def bank():
    calls = [Call("default", Params(), _marks_rings(5) + _classify_rings() + _tie_rings() + _edge_rings(5))]
    calls.append(Call("flat2", Params(max_surface_flat=2, max_corner_sharp=1), _tie_rings() + _classify_rings() + [pole_ring(2), pole_ring(4)]))
    for cr in (1, 16):
        rings = _edge_rings(cr) + [pole_ring(w) for w in (1, 2, cr + 1)] + [tie_wall(200, pattern=[0, 0, 1]), room_ring(),
                                                                              blind_ring([2, 3]), blind_ring([80, 81])]
        calls.append(Call("cr%d" % cr, Params(curvature_region=cr), rings))
    calls.append(Call("ring2560", Params(), [tie_wall(150), big_ring(), tie_wall(150, pattern=[0, 0, 1])]))
    # 70 region points over 40 regions: regions of one point (skipped) beside regions of two
    calls.append(Call("nf40", Params(n_feature_regions=40), [tie_wall(80, pattern=[0, 0, 1]), tie_wall(60), pole_ring(3, n=75),
                                                              room_ring(n=78)]))
    for nf in (1, 6, 40):
        calls.append(Call("ties_nf%d" % nf, Params(n_feature_regions=nf), _tie_rings() + _edge_rings(5)))
    # VoxelGrid: one voxel (every coordinate of the ring inside one 32 m cell), every point its own voxel, points exactly on
    # k * leaf, and a leaf so small that the index volume passes INT_MAX
    vox = [tie_wall(120, y0=1.0), tie_wall(120, y0=1.0, pattern=[0, 0, 1]), tie_wall(200)]
    calls.append(Call("voxel_one", Params(less_flat_filter_size=32.0), vox[:2]))
    calls.append(Call("voxel_own", Params(less_flat_filter_size=2.0 ** -6), vox))
    calls.append(Call("voxel_straddle", Params(less_flat_filter_size=0.25), vox))
    calls.append(Call("voxel_guard", Params(less_flat_filter_size=2.0 ** -14), vox + [room_ring()]))
    return calls


# event -> least count over the bank's UNAMBIGUOUS rings
REQUIRED = {
    # depth discontinuities at every spacing, both orders
    **{"disc_spacing_%d" % k: 1 for k in range(1, 7)},
    "pair_fn_nf": 6, "pair_nf_fn": 6,
    "edge_overwritten_by_near_block": 1, "edge_refused_by_guard": 1, "ratio_taken": 1, "ratio_refused": 1,
    "edge_broken_feature": 1,
    # blind gaps
    "blind_first_loop": 1, "blind_last_loop": 1, "blind_main_loop": 1, "blind_pair_within_2cr": 1,
    "blind_after_discontinuity": 1, "discontinuity_after_blind": 1,
    # ties
    "region_all_zero": 1, "tie_zero": 1, "tie_below": 1, "tie_above": 1, "flat_pick_among_ties": 1, "flat_excluded_by_mark": 1,
    "classified_among_ties": 1, "flat_cap_reached": 1,
    # pointClassify verdicts through loop 3 (which of the two SURFACE_FLAT branches is taken depends on the signs the
    # eigen-solver gives the two directions -- here numpy's; the verdict does not)
    "verdict_9": 10, "verdict_-1": 10, "verdict_1": 10, "verdict_5": 10, "flat_by_cos175": 1, "flat_by_cos5": 1,
    "corner_over_cap": 1, "corner_on_edge_broken": 1, "oneside_refused_by_shared_cap": 1,
    # ring and region edges
    "ring_skipped_at_2cr_plus_1": 3, "ring_smallest_processed": 3, "ring_2560": 1, "region_skipped": 1, "region_of_2": 1,
    "ring_empty": 1,
    # VoxelGrid
    "voxel_single": 1, "voxel_all_own": 1, "voxel_point_on_boundary": 1, "voxel_guard": 1, "voxel_mixed": 1,
}


# ---- one-parameter families for the thresholds --------------------------------------------------------------------------
# Marks and curvature rules: a ring of 40 points, curvatureRegion 5, the rule decided at point 19 / 20.  Classification
# gates: 11 points, pointClassify of point 5 (backward window 5 ... 0, forward window 10 ... 5).
def _arc(radius, az_deg):
    a = np.deg2rad(np.asarray(az_deg, np.float64))
    return np.stack([radius * np.cos(a), radius * np.sin(a), 0 * a], 1)


def fam_blind(t):
    """arc of radius 10 in 0.3 deg steps, an extra gap of t degrees after point 19"""
    az = np.arange(40) * 0.3
    az[20:] += float(t)
    return _arc(10.0, az).astype(np.float32)


def fam_diff_next(t):
    """the points from 20 on stand t metres further out: diffNext of point 19 crosses 1 m^2"""
    r = np.full(40, 10.0)
    r[20:] += float(t)
    return _arc(r, np.arange(40) * 0.3).astype(np.float32)


def fam_ratio(t):
    """a 2 m jump after point 19 and point 18 pulled in by t metres: diffPrev / diffNext of point 19 crosses 0.2"""
    r = np.full(40, 10.0)
    r[20:] += 2.0
    r[18] -= float(t)
    return _arc(r, np.arange(40) * 0.3).astype(np.float32)


def fam_depth(t):
    """200 m out, 0.1 deg steps and 0.4 deg between points 19 and 20 (1.4 m apart, not blind); the points from 20 on stand
    t metres further out: depth1 > depth2 flips, and with it the side that receives NEAR_BLOCK"""
    az = np.arange(40) * 0.1
    az[20:] += 0.3
    r = np.full(40, 200.0)
    r[20:] += float(t)
    return _arc(r, az).astype(np.float32)


def fam_curvature(t):
    """a dyadic wall, point 20 set back by t metres: its curvature (10 t)^2 crosses surfaceCurvatureThreshold"""
    p = tie_wall(40)
    p[20, 0] += float(t)
    return p.astype(np.float32)


def _line11(s):
    p = np.zeros((11, 3))
    p[:, 0] = 10.0
    p[:, 1] = (np.arange(11) - 5) * s
    return p


def fam_eig100(t):
    """backward window zig-zags by +-t across the line: lambda_2 = 100 lambda_1"""
    p = _line11(0.05)
    p[:6, 0] += float(t) * np.array([1, -1, 1, -1, 1, 0.0])
    return p.astype(np.float32)


def fam_eig10000(t):
    """backward window: a fixed zig-zag of 4 mm across (lambda_2 ~ 550 lambda_1) and one of t out of the plane"""
    p = _line11(0.05)
    p[:6, 0] += 0.004 * np.array([1, -1, 1, -1, 1, 0.0])
    p[:6, 2] += float(t) * np.array([1, -1, -1, 1, 1, 0.0])
    return p.astype(np.float32)


def fam_dist(t):
    """0.4 m pitch; the far end of the backward window stands t metres off the line: its distance to the fitted line
    (0.476 t: the end point pulls the fit towards itself) crosses 0.08"""
    p = _line11(0.4)
    p[0, 0] += float(t)
    return p.astype(np.float32)


def fam_angle(alpha_deg):
    """the forward half turns by alpha against the backward half"""
    p = _line11(0.05)
    a = np.deg2rad(float(alpha_deg))
    k = np.arange(1, 6)
    p[6:, 0] = 10.0 + k * 0.05 * np.sin(a)
    p[6:, 1] = k * 0.05 * np.cos(a)
    return p.astype(np.float32)


def as_ring13(p11):
    """an 11-point classification cloud as a ring of 13 points (two more along the forward half): with curvatureRegion 5 and
    one feature region the region is {5, 6}; with surfaceCurvatureThreshold 0 both are classified"""
    p = np.asarray(p11, np.float64)
    d = p[10] - p[9]
    return np.concatenate([p, [p[10] + d, p[10] + 2 * d]]).astype(np.float32)


# name -> (family, lo, hi, decision of an extraction / a verdict at lo)
MARK_FAMILIES = {
    "blind": (fam_blind, 0.0, 0.5), "diff_next": (fam_diff_next, 0.5, 1.5), "ratio": (fam_ratio, 0.5, 0.99),
    "depth": (fam_depth, -0.5, 0.5), "curvature": (fam_curvature, 0.005, 0.03),
}
# the name under which features_ref.Trace reports the rule's quantity when it lies inside its band
RULE_OF = {"blind": ("blind",), "diff_next": ("diffNext",), "ratio": ("ratio",), "depth": ("depth",), "curvature": ("curvature",),
           "eig100": ("eig100",), "eig10000": ("eig10000",), "dist": ("dist",), "angle5": ("cos5", "cos175"),
           "angle45": ("cos45", "cos135"), "angle135": ("cos45", "cos135"), "angle175": ("cos5", "cos175")}
CLASSIFY_FAMILIES = {
    "eig100": (fam_eig100, 0.001, 0.05), "eig10000": (fam_eig10000, 1e-4, 3e-3), "dist": (fam_dist, 0.1, 0.22),
    "angle5": (fam_angle, 1.0, 20.0), "angle45": (fam_angle, 30.0, 60.0), "angle135": (fam_angle, 120.0, 150.0),
    "angle175": (fam_angle, 160.0, 179.0),
}
MARK_DECISION = {
    "blind": lambda out: out["picked"][19] == -4,
    "diff_next": lambda out: out["picked"][22] == -3,
    "ratio": lambda out: out["picked"][19] == -2,
    "depth": lambda out: out["picked"][22] == -3,
    "curvature": lambda out: out["label"][20] == 0,
}
RANGE40 = np.array([[0, 39]], np.int32)
CLASSIFY_PARAMS = dict(n_feature_regions=1, surface_curvature_threshold=0.0)


def cloud4(p):
    c = np.zeros((len(p), 4), np.float32)
    c[:, :3] = p
    c[:, 3] = (np.arange(len(p)) / np.float32(4 * len(p))).astype(np.float32)
    return c


def adjacent_flip(f, lo, hi):
    """f(lo) != f(hi): shrink [lo, hi] to two adjacent float32 values with different f -> (lo, hi, f(lo))"""
    lo, hi = np.float32(lo), np.float32(hi)
    flo = f(lo)
    assert flo != f(hi)
    while True:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if f(mid) == flo:
            lo = mid
        else:
            hi = mid
    assert np.nextafter(lo, hi) == hi
    return lo, hi, flo


def threshold_pairs(oracle):
    """every rule bisected on the oracle -> dict name -> (lo, hi, decision at lo, decision at hi)"""
    pairs = {}
    for name, (fam, lo, hi) in MARK_FAMILIES.items():
        f = lambda t: bool(MARK_DECISION[name](oracle.extract_features(cloud4(fam(t)), RANGE40)))
        lo, hi, at_lo = adjacent_flip(f, lo, hi)
        pairs[name] = (lo, hi, at_lo, f(hi))
    for name, (fam, lo, hi) in CLASSIFY_FAMILIES.items():
        f = lambda t: int(oracle.point_classify(cloud4(fam(t)), 5))
        lo, hi, at_lo = adjacent_flip(f, lo, hi)
        pairs[name] = (lo, hi, at_lo, f(hi))
    return pairs


def threshold_calls(pairs, side):
    """the accepted (side 0: every family at its lo) or the rejected (side 1: at its hi) member of every pair, and a control
    ring per call that is the same on both sides: (marks call, classification call)"""
    marks = [MARK_FAMILIES[n][0](pairs[n][side]) for n in MARK_FAMILIES] + [tie_wall(40).astype(np.float32)]
    cls = [as_ring13(CLASSIFY_FAMILIES[n][0](pairs[n][side])) for n in CLASSIFY_FAMILIES] + [as_ring13(fam_angle(90.0))]
    return (Call("threshold_marks_%d" % side, Params(), [r.astype(np.float64) for r in marks], limit=1000.0),
            Call("threshold_classify_%d" % side, Params(**CLASSIFY_PARAMS), [r.astype(np.float64) for r in cls], limit=1000.0))
