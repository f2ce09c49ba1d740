"""numpy / Python-integer restatement of the occupancy-grid semantics of include/lslam_c.h (lslam_occ_*, csrc/lslam_occ.hip).

The crossed set is taken from its DEFINITION -- the open segment meets the open square -- by testing every cell of the ray's
bounding box: `crossed_exact` with Fractions, `crossed_mask` the same test cross-multiplied in int64 over the cells of the box
that lie in the grid.  Neither walks the ray; the kernel's per-column closed form is restated separately (`crossed_columns`)
and tests/test_occupancy_ref.py holds the three to each other."""
from fractions import Fraction

import numpy as np

F32 = np.float32
FIX = 1 << 30
DEFAULTS = dict(resolution=0.1, origin=(0.0, 0.0), width=0, height=0, up_axis=1, min_range=1.0, max_range=40.0, obstacle_min=0.3,
                obstacle_max=2.0, ground_band=0.15, sensor_height=1.8, ground_clears=1, hit_weight=3, min_observations=1)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(k)
        p[k] = v
    return p


def scale(p):
    return 256.0 / float(F32(p["resolution"]))


def rows(p):
    """The pose rows (graph axes) that are a and b."""
    return (2, 0) if int(p["up_axis"]) == 1 else (0, 1)


def fallback_plane(p):
    u = [0.0, 0.0, 0.0, float(F32(p["sensor_height"]))]
    u[1 if int(p["up_axis"]) == 1 else 2] = 1.0
    return np.array(u, np.float64)


def quantise(v, r, s):
    """Q of the header -> float64 (whole numbers, or not finite)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((np.asarray(v, np.float64) - float(r)) * s)


# ---- the crossed set ---------------------------------------------------------------------------------------------------------
def _t_interval(a, d, c):
    """The open t interval in which 256 c < a + t d < 256 (c + 1), as Fractions, or None when it is empty."""
    lo, hi = 256 * c, 256 * (c + 1)
    if d == 0:
        return (Fraction(-1), Fraction(2)) if lo < a < hi else None
    t0, t1 = Fraction(lo - a, d), Fraction(hi - a, d)
    return (min(t0, t1), max(t0, t1))


def cell_crossed_exact(A, B, i, j):
    """The definition, with Fractions: the open segment A + t (B - A), 0 < t < 1, meets the open square of cell (i, j)."""
    tx = _t_interval(A[0], B[0] - A[0], i)
    ty = _t_interval(A[1], B[1] - A[1], j)
    if tx is None or ty is None:
        return False
    return max(tx[0], ty[0], Fraction(0)) < min(tx[1], ty[1], Fraction(1))


def bbox_cells(A, B):
    i0, i1 = min(A[0], B[0]) >> 8, max(A[0], B[0]) >> 8
    j0, j1 = min(A[1], B[1]) >> 8, max(A[1], B[1]) >> 8
    return i0, i1, j0, j1


def crossed_exact(A, B):
    """-> the set of cells (i, j) the ray crosses: every cell of the bounding box against the definition."""
    i0, i1, j0, j1 = bbox_cells(A, B)
    return {(i, j) for i in range(i0, i1 + 1) for j in range(j0, j1 + 1) if cell_crossed_exact(A, B, i, j)}


def _bounds(a, d, c):
    """int64 arrays over the cells c: lower and upper t bound as num / den with den > 0, and whether the axis admits any t."""
    lo, hi = 256 * c - a, 256 * (c + 1) - a
    if d > 0:
        return lo, hi, np.int64(d), np.ones(c.shape, bool)
    if d < 0:
        return -hi, -lo, np.int64(-d), np.ones(c.shape, bool)
    ok = (lo < 0) & (hi > 0)
    return np.full(c.shape, -1, np.int64), np.full(c.shape, 2, np.int64), np.int64(1), ok


def crossed_mask(A, B, width, height):
    """-> bool (height, width): the crossed cells inside the grid.  The same test as cell_crossed_exact, cross-multiplied in
    int64 (|numerators| <= 2^30 + 2^21, denominators < 2^31), over the bounding box's cells that lie in the grid."""
    out = np.zeros((height, width), bool)
    i0, i1, j0, j1 = bbox_cells(A, B)
    i0, i1, j0, j1 = max(i0, 0), min(i1, width - 1), max(j0, 0), min(j1, height - 1)
    if i0 > i1 or j0 > j1:
        return out
    ci = np.arange(i0, i1 + 1, dtype=np.int64)[None, :]
    cj = np.arange(j0, j1 + 1, dtype=np.int64)[:, None]
    xl, xh, xd, xok = _bounds(int(A[0]), int(B[0]) - int(A[0]), ci)
    yl, yh, yd, yok = _bounds(int(A[1]), int(B[1]) - int(A[1]), cj)
    # max(xl/xd, yl/yd, 0) < min(xh/xd, yh/yd, 1): every lower bound below every upper bound
    ok = xok & yok & (xl < xh) & (yl < yh)
    ok = ok & (xl * yd < yh * xd) & (yl * xd < xh * yd)
    ok = ok & (xl < xd) & (yl < yd) & (xh > 0) & (yh > 0)
    out[j0:j1 + 1, i0:i1 + 1] = ok
    return out


def crossed_columns(A, B):
    """The per-column closed form the kernel uses (restated here to be held to the definition, not used by the reference):
    along the major axis u, the cells of column c are floor(vlo / 256) .. ceil(vhi / 256) - 1 for the v range over the column's
    part of the ray; the zero-length ray has its own line."""
    ax, ay, bx, by = int(A[0]), int(A[1]), int(B[0]), int(B[1])
    dx, dy = bx - ax, by - ay
    if dx == 0 and dy == 0:
        return {(ax >> 8, ay >> 8)} if (ax & 255) and (ay & 255) else set()
    major_a = abs(dx) >= abs(dy)
    au, av, bu, bv = (ax, ay, bx, by) if major_a else (ay, ax, by, bx)
    du, dv = bu - au, bv - av
    if du < 0:
        du, dv = -du, -dv
    umin, umax = min(au, bu), max(au, bu)
    out = set()
    for c in range(umin >> 8, ((umax + 255) >> 8)):
        ul, ur = max(256 * c, umin), min(256 * (c + 1), umax)
        nl, nr = dv * (ul - au), dv * (ur - au)
        vlo = av + (nl if dv >= 0 else nr) // du
        vhi = av - ((-(nr if dv >= 0 else nl)) // du)
        for j in range(vlo >> 8, ((vhi + 255) >> 8)):
            out.add((c, j) if major_a else (j, c))
    return out


# ---- a keyframe's vote -------------------------------------------------------------------------------------------------------
def classify(points, plane, p):
    """-> (obstacle, ground) masks over the points (fp32, every operation rounded on its own)."""
    pts = np.asarray(points, F32).reshape(-1, 4) if np.asarray(points).size else np.zeros((0, 4), F32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    pl = np.asarray(plane, np.float64).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d2 = (x * x + y * y) + z * z
        lo, hi = F32(p["min_range"]) * F32(p["min_range"]), F32(p["max_range"]) * F32(p["max_range"])
        gate = finite & (d2 >= lo) & (d2 <= hi)
        h = ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3]
        obstacle = gate & (h >= F32(p["obstacle_min"])) & (h <= F32(p["obstacle_max"]))
        ground = gate & (np.abs(h) <= F32(p["ground_band"])) & bool(p["ground_clears"])
    return obstacle, ground


def ray_ends(points, T, p):
    """-> (A, B float64 (n, 2) fixed-point values before the range check, E float32 (n, 2))."""
    pts = np.asarray(points, F32).reshape(-1, 4)
    T = np.asarray(T, np.float64).astype(F32).reshape(4, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    s = scale(p)
    E = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in rows(p):
            E.append(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3])
    E = np.stack(E, axis=1).astype(F32)
    B = np.stack([quantise(E[:, 0], p["origin"][0], s), quantise(E[:, 1], p["origin"][1], s)], axis=1)
    ra, rb = rows(p)
    A = np.array([quantise(T[ra, 3], p["origin"][0], s), quantise(T[rb, 3], p["origin"][1], s)], np.float64)
    return A, B, E


def in_range(v):
    with np.errstate(invalid="ignore"):
        return (v >= -FIX) & (v < FIX)  # (NaN: False)


def keyframe_vote(corner, surf, T, plane, p):
    """-> (hit, free: bool (height, width), stats dict cast / dropped / obstacle / ground).  plane None: the fallback."""
    W, H = int(p["width"]), int(p["height"])
    clouds = [np.asarray(c, F32).reshape(-1, 4) for c in (corner, surf)]
    pts = np.concatenate(clouds, axis=0)
    pl = fallback_plane(p) if plane is None else np.asarray(plane, np.float64)
    obstacle, ground = classify(pts, pl, p)
    assert not (obstacle & ground).any()
    A, B, _ = ray_ends(pts, T, p)
    ok = in_range(B[:, 0]) & in_range(B[:, 1]) & bool(in_range(A[0]) and in_range(A[1]))
    hit, free = np.zeros((H, W), bool), np.zeros((H, W), bool)
    st = dict(dropped=int(((obstacle | ground) & ~ok).sum()), obstacle=int((obstacle & ok).sum()), ground=int((ground & ok).sum()))
    st["cast"] = st["obstacle"] + st["ground"]
    if ok.any():
        a = (int(A[0]), int(A[1]))
        for k in np.nonzero((obstacle | ground) & ok)[0]:
            b = (int(B[k, 0]), int(B[k, 1]))
            m = crossed_mask(a, b, W, H)
            if obstacle[k]:
                ei, ej = b[0] >> 8, b[1] >> 8
                if 0 <= ei < W and 0 <= ej < H:
                    hit[ej, ei] = True
                    m[ej, ei] = False
            free |= m
    free &= ~hit
    return hit, free, st


class Grid:
    """The counts of one grid and the ray counters, as the store keeps them."""

    def __init__(self, p):
        self.p = p
        self.clear()

    def clear(self):
        self.n_free = np.zeros((int(self.p["height"]), int(self.p["width"])), np.int64)
        self.n_hit = np.zeros_like(self.n_free)
        self.stats = dict(cast=0, dropped=0, obstacle=0, ground=0)
        self.n_integrated = 0

    def integrate(self, keyframes, ids, poses, planes=None, plane_valid=None):
        """keyframes: list of (corner, surf); planes: (n, 4) or None; plane_valid: flags or None."""
        for k, kid in enumerate(ids):
            use = planes is not None and (plane_valid is None or plane_valid[k])
            hit, free, st = keyframe_vote(keyframes[kid][0], keyframes[kid][1], poses[k], planes[k] if use else None, self.p)
            self.n_hit += hit
            self.n_free += free
            for key in self.stats:
                self.stats[key] += st[key]
            self.n_integrated += 1

    def counts(self):
        return (self.n_free | (self.n_hit << 16)).astype(np.uint32)

    def values(self):
        return values(self.n_hit, self.n_free, self.p["hit_weight"], self.p["min_observations"])


def value(n_hit, n_free, hit_weight, min_observations):
    """One cell, Python integers."""
    if n_hit + n_free < min_observations:
        return -1
    H = hit_weight * n_hit
    D = H + n_free
    return (200 * H + D) // (2 * D)


def values(n_hit, n_free, hit_weight, min_observations):
    nh, nf = np.asarray(n_hit, np.int64), np.asarray(n_free, np.int64)
    H = int(hit_weight) * nh
    D = H + nf
    v = (200 * H + D) // np.maximum(2 * D, 1)
    return np.where(nh + nf < int(min_observations), -1, v).astype(np.int8)


# ---- fit_bounds --------------------------------------------------------------------------------------------------------------
def fit_bounds(poses, p):
    """The header's formula in fp64 -> (origin (a, b), width, height) and the (lo, hi) per axis it was fitted to."""
    T = np.asarray(poses, np.float64).astype(F32).reshape(-1, 4, 4)
    r, m = float(F32(p["resolution"])), float(F32(p["max_range"]))
    origin, cells, spans = [], [], []
    for row in rows(p):
        o = T[:, row, 3].astype(np.float64)
        lo, hi = float((o - m).min()), float((o + m).max())
        i0 = float(np.floor(lo / r))
        while i0 * r > lo:
            i0 -= 1.0
        while (i0 + 1.0) * r <= lo:
            i0 += 1.0
        org = i0 * r
        w = max(1.0, float(np.ceil((hi - org) / r)))
        while org + w * r < hi:
            w += 1.0
        while w > 1.0 and org + (w - 1.0) * r >= hi:
            w -= 1.0
        origin.append(org)
        cells.append(int(w))
        spans.append((lo, hi))
    return tuple(origin), cells[0], cells[1], spans


# ---- helpers of the device tests ---------------------------------------------------------------------------------------------
def pose_matrix(p6):
    """(rx, ry, rz, x, y, z) -> 4x4 float64, R = Rz Ry Rx."""
    rx, ry, rz, x, y, z = (float(v) for v in p6)
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (x, y, z)
    return T


def trinary(vals):
    v = np.asarray(vals, np.int64)
    img = np.full(v.shape, 205, np.uint8)
    img[v >= 65] = 0
    img[(v >= 0) & (v <= 19)] = 254
    return img[::-1]
