"""The bank the mapping fit (find_line, find_plane, corner_coeff, surf_coeff) is held to tests/fit_ref.py on: seeded, numpy only,
shared by tests/test_fit_ref.py (the oracle, CPU) and tests/test_gpu_fit_general.py (the device).

TEST INFRASTRUCTURE.  Nothing is recorded: every array comes from the seeds below.  A bank is a dict
  nb    (N, 5, 4) float32   the five neighbours of every fit (w = 0)
  x     (N, 4)    float32   the query point of every fit
  cell  (N,)      int       index into `cells`
  cells list of (distance of the patch from the origin, aspect or None, noise sigma)
  on_line (lines only) indices whose query point the tests move onto the fitted line (X = A, the fit's own float32 end
          point: the d = 0 row, direction 0/0)
"""
import numpy as np

A_OFF = np.array([-0.5, -0.25, 0.0, 0.25, 0.5])
B_OFF = np.array([0.3, -0.5, 0.5, -0.3, 0.1])
JITTER = 0.1

PLANE_PER_CELL, LINE_PER_CELL = 300, 400
PLANE_CELLS = ([(d, a, s) for d in (0.5, 5.0, 50.0) for a in (1.0, 0.1, 0.01) for s in (0.0, 0.01, 0.05)]
               + [(d, a, s) for d in (300.0, 420.0) for a in (1.0, 0.1) for s in (0.0, 0.01, 0.05)])
LINE_CELLS = [(d, None, s) for d in (0.5, 5.0, 50.0, 300.0, 420.0) for s in (0.0, 0.005, 0.03, 0.08, 0.15)]
X_NEAR, X_FAR = 0.02, 1.5  # the query point's distance from the feature, log-uniform between the two


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _frames(rng, n):
    """n orthonormal frames (u, v, w), uniformly distributed."""
    w = _unit(rng, n)
    t = _unit(rng, n)
    u = np.cross(w, t)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(w, u), w


def _xyz0(p):
    out = np.zeros(p.shape[:-1] + (4,), np.float32)
    out[..., :3] = p.astype(np.float32)
    return out


def _height(rng, n):
    return np.exp(rng.uniform(np.log(X_NEAR), np.log(X_FAR), n)) * rng.choice([-1.0, 1.0], n)


def plane_bank(seed=20261):
    rng = np.random.default_rng(seed)
    nb, x, cell = [], [], []
    for k, (d, aspect, sigma) in enumerate(PLANE_CELLS):
        n = PLANE_PER_CELL
        u, v, w = _frames(rng, n)
        centre = d * _unit(rng, n)
        a = A_OFF[None, :] + rng.uniform(-JITTER, JITTER, (n, 5))
        b = (B_OFF[None, :] + rng.uniform(-JITTER, JITTER, (n, 5))) * aspect
        h = sigma * rng.standard_normal((n, 5))
        p = centre[:, None, :] + a[..., None] * u[:, None, :] + b[..., None] * v[:, None, :] + h[..., None] * w[:, None, :]
        q = centre + rng.uniform(-0.5, 0.5, (n, 1)) * u + rng.uniform(-0.5, 0.5, (n, 1)) * v + _height(rng, n)[:, None] * w
        nb.append(_xyz0(p)); x.append(_xyz0(q)); cell.append(np.full(n, k))
    return dict(nb=np.concatenate(nb), x=np.concatenate(x), cell=np.concatenate(cell), cells=list(PLANE_CELLS))


def line_bank(seed=20262):
    rng = np.random.default_rng(seed)
    nb, x, cell = [], [], []
    for k, (d, _, sigma) in enumerate(LINE_CELLS):
        n = LINE_PER_CELL
        u, v, w = _frames(rng, n)
        centre = d * _unit(rng, n)
        p = centre[:, None, :] + A_OFF[None, :, None] * u[:, None, :] + sigma * rng.standard_normal((n, 5, 3))
        phi = rng.uniform(0, 2 * np.pi, (n, 1))
        q = centre + rng.uniform(-0.3, 0.3, (n, 1)) * u + np.abs(_height(rng, n))[:, None] * (np.cos(phi) * v + np.sin(phi) * w)
        nb.append(_xyz0(p)); x.append(_xyz0(q)); cell.append(np.full(n, k))
    cell = np.concatenate(cell)
    # the first two fits of every noise-free and every 0.005 cell get their point put on the line by the tests
    on_line = np.concatenate([np.flatnonzero(cell == k)[:2] for k, c in enumerate(LINE_CELLS) if c[2] <= 0.005])
    return dict(nb=np.concatenate(nb), x=np.concatenate(x), cell=cell, cells=list(LINE_CELLS), on_line=on_line)


def put_on_line(x, on_line, A):
    """A copy of x with the listed points at the fitted line's end point A (n, 3) float32: X - A = 0 exactly, so the cross product,
    its norm and the direction's denominator are exact zeros."""
    x = np.array(x, np.float32, copy=True)
    x[on_line, :3] = np.asarray(A, np.float32)[on_line, :3]
    return x


def _patch():
    """An ordinary patch: a tilted plane 6 m out with 1 cm noise, and a point 0.3 m off it."""
    rng = np.random.default_rng(77)
    u, v, w = (f[0] for f in _frames(rng, 1))
    c = np.array([3.0, -4.5, 2.5])
    p = c + np.outer(A_OFF, u) + np.outer(B_OFF, v) + np.outer(0.01 * rng.standard_normal(5), w)
    return p.astype(np.float32), (c + 0.1 * u + 0.3 * w).astype(np.float32)


def degenerate_sets():
    """-> (names, nb (n, 5, 4), x (n, 4)): the neighbour sets float64 has no answer for, one per element.  Both fits run on
    every one of them; the rule is device == oracle to the bit, NaNs in the same places."""
    p, q = _patch()
    t = np.arange(-2.0, 3.0)
    sets = []
    sets.append(("collinear", np.stack([1.0 + t, 2.0 + t, np.full(5, 3.0)], 1), q))                    # rank 2
    sets.append(("collinear_through_origin", np.stack([t + 3.0, 2 * (t + 3.0), -(t + 3.0)], 1), q))     # rank 1
    sets.append(("coincident", np.tile([1.5, -2.0, 0.75], (5, 1)), q))
    sets.append(("zeros", np.zeros((5, 3)), q))
    sets.append(("zeros_and_zero_point", np.zeros((5, 3)), np.zeros(3)))
    flat = np.array([[1.0, 2.0, 0.0], [-1.0, 3.0, 0.0], [2.5, -0.5, 0.0], [0.25, 0.75, 0.0], [-2.0, -1.0, 0.0]])
    sets.append(("zero_column", flat, np.array([0.5, 0.5, 0.4])))                                         # z = 0: a zero column
    sets.append(("zero_column_x", flat[:, [2, 0, 1]], np.array([0.4, 0.5, 0.5])))
    for name, bad in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf)):
        for j, k in ((3, 1), (0, 0)):
            c = p.astype(np.float64).copy()
            c[j, k] = bad
            sets.append(("%s_%d%d" % (name, j, k), c, q))
    sets.append(("nan_point", p, np.array([np.nan, 1.0, 2.0])))
    sets.append(("scaled_up_40", p.astype(np.float64) * 2.0 ** 40, q.astype(np.float64) * 2.0 ** 40))
    sets.append(("scaled_down_40", p.astype(np.float64) * 2.0 ** -40, q.astype(np.float64) * 2.0 ** -40))
    dup = p.astype(np.float64).copy()
    dup[4] = dup[1]
    sets.append(("two_duplicates", dup, q))
    line = np.array([3.0, -4.5, 2.5]) + np.outer(A_OFF, [0.6, 0.0, 0.8])
    dupl = line.copy()
    dupl[2] = dupl[3]
    sets.append(("line_two_duplicates", dupl, q))
    names = [s[0] for s in sets]
    return names, _xyz0(np.stack([np.asarray(s[1], np.float64) for s in sets])), _xyz0(np.stack([np.asarray(s[2], np.float64) for s in sets]))


# ---------------------------------------------------------------------------
# mixed wavefronts: 64 consecutive elements of a bank, one lane replaced by a set the in-range fit does not take
# ---------------------------------------------------------------------------
MIXED_LANES = (0, 31, 63)
MIXED_TAILS = (0, 1, 63)  # n = 64 k + tail


def _zero_sum_line():
    """Five collinear points whose x sums to exactly 0 (the centroid's first numerator is +0, outside the in-range fit's
    range), an ordinary line otherwise."""
    p = np.stack([np.array([-1.0, -0.5, 0.0, 0.5, 1.0]), 7.0 + 0.25 * np.arange(5), np.full(5, 2.0)], 1)
    assert p[:, 0].astype(np.float32).sum() == 0.0
    return p


def mixed_wavefronts(bank, kind, n_groups=6):
    """kind 'line_centroid' | 'corner_on_line' | 'plane_floor' | None.  -> dict(nb, x, replaced: indices of the replaced lanes,
    on_line: indices whose point the tests put on the fitted line).  n_groups full groups of 64 from the start of the
    bank's cells (one group per cell, so near and far ones take part) followed by 63 more elements, so that every size in
    MIXED_TAILS is a prefix: the caller runs [: 64 n_groups + tail]."""
    take = []
    cells = np.unique(bank["cell"])
    step = max(1, len(cells) // n_groups)
    for g in range(n_groups):
        take.append(np.flatnonzero(bank["cell"] == cells[(g * step) % len(cells)])[10:74])
    take.append(np.flatnonzero(bank["cell"] == cells[-1])[80:143])
    take = np.concatenate(take)
    assert len(take) == 64 * n_groups + 63
    nb, x = bank["nb"][take].copy(), bank["x"][take].copy()
    replaced = np.array([64 * g + MIXED_LANES[g % 3] for g in range(n_groups)] + [64 * n_groups + 31])
    on_line = np.zeros(0, np.int64)
    if kind == "line_centroid":
        nb[replaced] = _xyz0(_zero_sum_line())[None]
        x[replaced] = _xyz0(np.array([0.1, 7.4, 2.6]))
    elif kind == "corner_on_line":
        on_line = replaced
    elif kind == "plane_floor":
        nb[replaced, :, 2] = 0.0
    elif kind is None:  # the same elements, none replaced
        pass
    else:
        raise ValueError(kind)
    return dict(nb=nb, x=x, replaced=replaced, on_line=on_line, n_groups=n_groups)


# ---------------------------------------------------------------------------
# the oracle through the same door as the device's tap
# ---------------------------------------------------------------------------
MATCHED, KEPT = 8, 2  # the general fit's bits of lslam_debug_fit_stage's flags


def oracle_fit_stage(oracle, nb, x, is_surf, on_line=()):
    """Oracle.find_line / find_plane and corner_coeff / surf_coeff per element, in the layout of lslam_debug_fit_stage's general
    half: (out (n, 12) float32, flags (n,) int32 with bits MATCHED and KEPT, x as used).  A point listed in on_line is moved onto
    the oracle's own A before the coefficient (put_on_line)."""
    nb, x = np.ascontiguousarray(nb, np.float32), np.array(x, np.float32, copy=True)
    n = len(x)
    out, fl = np.zeros((n, 12), np.float32), np.zeros(n, np.int32)
    idx = np.arange(5, dtype=np.int32)
    on_line = set(int(i) for i in on_line)
    for i in range(n):
        if is_surf:
            ok, pl = oracle.find_plane(nb[i], idx)
            out[i, :4] = pl
            if ok:
                kept, out[i, 8:] = oracle.surf_coeff(pl, x[i, :3])
        else:
            A, B = np.zeros(3, np.float32), np.zeros(3, np.float32)
            ok, a, b = oracle.find_line(nb[i], idx)
            if ok:
                A, B = a, b
                if i in on_line:
                    x[i, :3] = A
                kept, out[i, 8:] = oracle.corner_coeff(A, B, x[i, :3])
            out[i, :3], out[i, 3:6] = A, B
        fl[i] = (MATCHED if ok else 0) | (KEPT if ok and kept else 0)
    return out, fl, x
