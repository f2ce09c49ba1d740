"""float64 reference of the mapping fit -- findLine, findPlane and the two feature coefficients (util/feature_utils.h:17-204;
find_line, find_plane, corner_coeff, surf_coeff of csrc/lslam_device.hpp and their twins in oracle/lslam_oracle.c).  numpy only:
nothing here imports the library under test or its oracle.

TEST INFRASTRUCTURE: imported by tests/test_fit_ref.py (the oracle, CPU) and tests/test_gpu_fit_general.py (the device).

The reference takes what a fit takes -- five float32 neighbours, a float32 point -- and works in float64 with algorithms other
than the fit's own: an SVD least-squares solve (numpy.linalg.lstsq) where the fit has a column-pivoted Householder QR, LAPACK's
eigh where it has Eigen's tridiagonal QR iteration.  Every quantity carries the UNIT its tolerance is counted in, and a
criterion is `distance from the reference <= K units`.  Checks of a later stage start from the fit's OWN float32 results of the
stage before (the plane for D, the verdict and the surf coefficient; A, B for the corner coefficient), so each stage is held
on its own and an inaccurate normal does not excuse a wrong D.

EPS = 2^-24.  Units, and in brackets the roundings of the chain each covers (the DERIVED count, worst case, all aligned):

 plane
  normal     sin angle(n^, n*)             u = EPS (kappa + kappa^2 rho* / (sigma_1 |x*|)), kappa = sigma_1 / sigma_3, rho* = |P x* + 1|:
                                           the first-order perturbation bound of a least-squares solution for a relative
                                           backward error EPS of the 5 x 3 matrix.  Householder QR's backward error is gamma_mn
                                           c with m n = 15 and a small c (Higham, Accuracy and Stability, thm 19.3/20.3); the
                                           normalisation adds 4: [DERIVED_PLANE_NORMAL = 15 * 2 + 4 = 34]
             where K u > 0.1 rad the data do not determine the direction: the case is left out of THIS criterion only
  norm       | |n^| - 1 |                  u = EPS   [3 products and 2 sums under a root: 1.5; the root 1; the division 1: 4]
  d          | D^ + n^ . c |               u = EPS (sum |n^_i| |c_i| + sum_i |n^_i| sum_j |p_ji| / 5), c the float64 centroid
                                           [c: 4 sums and the division by 5 -- 5 of the second term; 3 products, 2 sums: 10]
  matched    all five |n^ . p_j + D^| <= 0.2f, in float64 from n^, D^, against the fit's verdict; the margin of a case is the
             distance of the deciding |.| from 0.2f in units u_j = EPS (sum |n^_i| |p_ji| + |D^|)   [3 products, 3 sums: 6]
 line
  centre     | (A^ + B^) / 2 - c |_inf     u = EPS 3 max |p|   [c: 5 of max |p|; A, B: one each of |c| + 0.1; their mean is
                                           taken in float64: (5 + 2) / 3, counted as 3]
  direction  sin angle(B^ - A^, v_2)       u = EPS (sqrt(3) |c|_inf / 0.1 + l_2 / (l_2 - l_1)): the quantisation of A and B at the
                                           coordinate's ulp (one rounding each, 0.2 m apart: 1 of the first term) and
                                           Davis-Kahan for the covariance's error E, |E| <= c EPS l_2: 5 products, 4 sums, the
                                           division, the entry's majorant at most trace <= 1.4 l_2 for an accepted line (14), the
                                           eigen-solver's backward error (tridiagonalisation and at most a few QR sweeps of 3 x 3
                                           rotations: 12)   [DERIVED_LINE_DIRECTION = 26]
  length     | |B^ - A^| / 0.2 - 1 |       u = EPS (sqrt(3) |c|_inf / 0.1 + 1): the same quantisation; the 1 carries the unit
                                           vector's norm (4), 0.1f for 0.1 (0.25) and the product (1)   [6]
  matched    l_2 > 5 l_1 against the fit's verdict; margin |l_2 - 5 l_1| in units EPS l_2
                                           [6 eigenvalue errors of 26 EPS l_2 at worst: DERIVED_LINE_MATCHED = 156]
 corner coefficient, from A^, B^, X (feature_utils.h:17-26, :63-75): n = (X - B) x (X - A), d = |n| / |A - B|,
   dir = (-n) x (B - A) / (|n| |A - B|), w = 1 - 0.9f d, coeff = (dir w, d w).  With nh, crh the cross products of absolute values:
  distance   coeff[3] / w is not returned; d is held through coeff[3]:
  c3         | c3^ - d w |                 u = EPS (dh |w| + d wh), dh = |nh| / |A - B|, wh = 1 + 0.9 dh
                                           [d: the two differences through the product 2, product 1, difference 1, norm 2.5,
                                           |A - B| 3.5, division 1: 11; w: 0.9 x 11 of dh and its own rounding; the product: 13]
  dir        | c_i^ - dir_i w |            u = EPS (dirh_i |w| + |dir_i| wh), dirh_i = crh_i / (|n| |A - B|) + |nh| / |n|
                                           [cr 7, the denominator 6.5 + 3.5 + 1, the division 1, w 11, the product 1: 31]
  kept       w > 0.1 against the fit's bit; margin |w - 0.1| in units EPS wh   [11 + 1: 12]
  the d = 0 row (X on the line: n = 0, dir = 0/0) is part of the specification: NaN, NaN, NaN, 0, kept.
 surf coefficient, from the plane^ and X (:97-106): d = n^ . X + D^, w = 1 - 0.9 |d| / sqrt(|X|), coeff = (n^ w, d w)
  c3         | c3^ - d w |                 u = EPS (dh |w| + |d| wh), dh = sum |n^_i| |X_i| + |D^|, wh = 1 + 0.9 dh / sqrt(|X|)
                                           [d 6; w: 6 of dh, |X| 2.5 / 2, its rounding 1: 9; the product 1: 10]
  normal     | c_i^ - n^_i w |             u = EPS |n^_i| wh   [w 9, the product 1: 10]
  kept       w > 0.1; margin |w - 0.1| in units EPS wh   [9]

K of a criterion is 10 x the worst the ORACLE shows on the bank of tests/fit_cases.py, rounded up (the margin K_S of
tests/scanmatch_ref.py has over its measured floor); the derived count must not be below that worst
(tests/test_fit_ref.py asserts both, and that the oracle stays within K / 4).  For a verdict the oracle's worst is the largest
margin at which its verdict differs from float64's; where it never differs K is the derived count.

  criterion        oracle's worst (CPU)   device's worst (MI355X)   derived   K
  plane_normal            2.39                  2.39                  34      24
  plane_norm              2.18                  2.18                   4      22
  plane_d                 1.68                  1.68                  10      17
  plane_matched           never differs         never differs          6       6
  line_centre             0.917                 0.917                  3      10
  line_direction          0.696                 0.696                 26       7
  line_length             0.864                 0.864                  6       9
  line_matched            never differs         never differs        156     156
  corner_dir              1.17                  1.17                  31      12
  corner_c3               1.62                  1.62                  13      17
  corner_kept             never differs         never differs         12      12
  surf_normal             1.10                  1.10                  10      12
  surf_c3                 1.12                  1.12                  10      12
  surf_kept               never differs         never differs          9       9
(the device's general fit equals the oracle bit for bit on the whole bank -- tests/test_gpu_fit_general.py -- so its worst values are
the oracle's; per cell: DESIGN.md 4, "How accurate the fit is".)  With K = 24 the normal's tolerance is 1.4e-6 kappa rad: about 1e-5 rad for a
1 m patch 2 m from the origin, and undetermined (above 0.1 rad) from kappa = 7e4 on.

`variant` applies one mutation to a COPY of the reference, never to a kernel; tests/test_fit_ref.py shows that every one of
VARIANTS is seen, and in which cells.
"""
import numpy as np

EPS32 = 2.0 ** -24
F02 = float(np.float32(0.2))   # the inlier bound as the fit has it (max_distance = 0.2f)
F09 = float(np.float32(0.9))   # corner weight: 0.9f; the surf weight's 0.9 is a double literal
UNDETERMINED = 0.1             # rad: K_n u_n above this and the data do not determine the normal

VARIANTS = ("ratio_3", "middle_eigenvector", "offset_009", "d_first_neighbour", "tls_normal", "inlier_025", "weight_08",
            "abs_for_sqrt", "corner_negated", "distance_unweighted")

# criterion -> (oracle's worst on the bank, derived count).  Measured by tests/test_fit_ref.py::test_oracle_within_a_quarter_of_k.
MEASURED = {
    "plane_normal": (2.4, 34.0),
    "plane_norm": (2.2, 4.0),
    "plane_d": (1.7, 10.0),
    "plane_matched": (0.0, 6.0),
    "line_centre": (0.92, 3.0),
    "line_direction": (0.7, 26.0),
    "line_length": (0.87, 6.0),
    "line_matched": (0.0, 156.0),
    "corner_c3": (1.7, 13.0),
    "corner_dir": (1.2, 31.0),
    "corner_kept": (0.0, 12.0),
    "surf_c3": (1.2, 10.0),
    "surf_normal": (1.2, 10.0),
    "surf_kept": (0.0, 9.0),
}
VERDICTS = ("plane_matched", "line_matched", "corner_kept", "surf_kept")


def k_of(name):
    worst, derived = MEASURED[name]
    if name in VERDICTS and worst == 0.0:
        return derived
    return float(np.ceil(10.0 * worst))


K = {name: k_of(name) for name in MEASURED}


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _ratio(d, u):
    """d / u per element; 0 where both are 0, inf where only the unit is."""
    with np.errstate(all="ignore"):
        out = np.where(u > 0, d / np.where(u > 0, u, 1.0), np.where(d > 0, np.inf, 0.0))
    return out


# ---------------------------------------------------------------------------
# plane
# ---------------------------------------------------------------------------
def plane_reference(nb, variant=None):
    """nb (N, 5, >=3) float32 -> dict(n (N, 3), D (N,), c (N, 3), u_n (N,), kappa (N,)): the least-squares plane of
    [x y z] x = -1, by SVD."""
    P = _f64(nb)[:, :, :3]
    N = len(P)
    x = np.zeros((N, 3))
    sv = np.zeros((N, 3))
    rhs = -np.ones(5)
    for i in range(N):
        x[i], _, _, sv[i] = np.linalg.lstsq(P[i], rhs, rcond=None)
    c = P.mean(1)
    xn = _norm(x)
    n = x / xn[:, None]
    rho = _norm(np.einsum("nji,ni->nj", P, x) + 1.0)
    kappa = sv[:, 0] / sv[:, 2]
    u_n = EPS32 * (kappa + kappa ** 2 * rho / (sv[:, 0] * xn))
    if variant == "tls_normal":  # mutation: the plane of the centred total least squares (smallest eigenvector of the covariance)
        q = P - c[:, None, :]
        _, V = np.linalg.eigh(np.einsum("nji,njk->nik", q, q))
        n = V[:, :, 0] * np.sign((V[:, :, 0] * n).sum(1))[:, None]
    first = P[:, 0, :] if variant == "d_first_neighbour" else c  # mutation: D from the first neighbour
    return dict(n=n, D=-(n * first).sum(1), c=c, anchor=first, u_n=u_n, kappa=kappa)


def plane_check(nb, plane, matched, variant=None, ref=None):
    """The fit's float32 plane (N, 4) and verdict (N,) bool against the reference -> dict of per-case arrays:
    plane_normal (units; NaN where left out), determined_at(K) via u_n, plane_norm, plane_d (units), plane_matched (the margin
    where the verdict differs from float64's, else 0), margin (every case's distance from the bound, in units)."""
    ref = plane_reference(nb, variant) if ref is None else ref
    P = _f64(nb)[:, :, :3]
    pl = _f64(plane)
    nh, Dh = pl[:, :3], pl[:, 3]
    with np.errstate(all="ignore"):
        sin = _norm(np.cross(nh, ref["n"])) / _norm(nh)
    out = dict(u_n=ref["u_n"], sin=sin, plane_normal=_ratio(sin, ref["u_n"]))
    out["plane_norm"] = np.abs(_norm(nh) - 1.0) / EPS32
    anchor = ref["anchor"]
    u_d = EPS32 * ((np.abs(nh) * np.abs(ref["c"])).sum(1) + (np.abs(nh) * np.abs(P).sum(1) / 5.0).sum(1))
    out["plane_d"] = _ratio(np.abs(Dh + (nh * anchor).sum(1)), u_d)
    bound = 0.25 if variant == "inlier_025" else F02  # mutation: the inlier bound
    dist = np.abs(np.einsum("nji,ni->nj", P, nh) + Dh[:, None])
    u_j = EPS32 * (np.einsum("nji,ni->nj", np.abs(P), np.abs(nh)) + np.abs(Dh)[:, None])
    ref_matched = (dist <= bound).all(1)
    over = _ratio(dist - bound, u_j)   # > 0: neighbour j is outside by so many units
    margin = np.where(ref_matched, (-over).min(1), over.max(1))
    out["ref_matched"] = ref_matched
    out["margin_matched"] = margin
    out["plane_matched"] = np.where(ref_matched != np.asarray(matched, bool), margin, 0.0)
    return out


# ---------------------------------------------------------------------------
# line
# ---------------------------------------------------------------------------
def line_reference(nb, variant=None):
    """-> dict(c, lam (N, 3) ascending, v (N, 3) the direction, A, B, matched, margin_matched)."""
    P = _f64(nb)[:, :, :3]
    c = P.mean(1)
    q = P - c[:, None, :]
    lam, V = np.linalg.eigh(np.einsum("nji,njk->nik", q, q) / 5.0)
    v = V[:, :, 1] if variant == "middle_eigenvector" else V[:, :, 2]  # mutation: the middle eigenvector
    half = 0.09 if variant == "offset_009" else 0.1                     # mutation: c -+ 0.09 v
    ratio = 3.0 if variant == "ratio_3" else 5.0                        # mutation: the eigenvalue ratio
    return dict(c=c, lam=lam, v=v, half=half, A=c - half * v, B=c + half * v, matched=lam[:, 2] > ratio * lam[:, 1],
                margin_matched=_ratio(np.abs(lam[:, 2] - ratio * lam[:, 1]), EPS32 * lam[:, 2]), maxp=np.abs(P).max((1, 2)))


def line_check(nb, A, B, matched, variant=None, ref=None):
    """The fit's float32 A, B (N, 3) and verdict against the reference.  The geometry criteria are NaN where the fit did not
    match (it returns no line there)."""
    ref = line_reference(nb, variant) if ref is None else ref
    A, B, m = _f64(A)[:, :3], _f64(B)[:, :3], np.asarray(matched, bool)
    nan = np.where(m, 0.0, np.nan)
    c, lam = ref["c"], ref["lam"]
    out = dict(ref_matched=ref["matched"], margin_matched=ref["margin_matched"])
    out["line_matched"] = np.where(ref["matched"] != m, ref["margin_matched"], 0.0)
    out["line_centre"] = np.abs((A + B) / 2.0 - c).max(1) / (EPS32 * 3.0 * ref["maxp"]) + nan
    quant = np.sqrt(3.0) * np.abs(c).max(1) / 0.1
    d = B - A
    with np.errstate(all="ignore"):
        sin = _norm(np.cross(d, ref["v"])) / _norm(d)
        gap = lam[:, 2] / (lam[:, 2] - lam[:, 1])
        out["sin"] = sin + nan
        out["line_direction"] = _ratio(sin, EPS32 * (quant + gap)) + nan
        out["line_length"] = np.abs(_norm(d) / (2.0 * ref["half"]) - 1.0) / (EPS32 * (quant + 1.0)) + nan
    return out


# ---------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------
def _cross_abs(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


def _coeff_units(got, want, unit):
    """|got - want| / unit per entry; a NaN the reference has and the fit has too is 0, one that only one of them has is inf."""
    got = np.asarray(got, np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    with np.errstate(all="ignore"):
        u = _ratio(np.abs(got - want), unit)
    u = np.where(gn & wn, 0.0, u)
    return np.where(gn != wn, np.inf, u)


def corner_check(A, B, X, coeff, kept, variant=None):
    """The fit's float32 coefficient (N, 4) and kept bit, from ITS A, B (N, 3) float32 and the point X."""
    A, B, X = _f64(A)[:, :3], _f64(B)[:, :3], _f64(X)[:, :3]
    c = _f64(coeff)
    XB, XA, BA = X - B, X - A, B - A
    n = np.cross(XB, XA)
    nh = _cross_abs(XB, XA)
    cr = np.cross(-n, BA)
    crh = _cross_abs(nh, BA)
    nn, lab = _norm(n), _norm(BA)
    wc = 0.8 if variant == "weight_08" else F09  # mutation: the weight's constant
    with np.errstate(all="ignore"):
        d = nn / lab
        dirv = cr / (nn * lab)[:, None]
        if variant == "corner_negated":  # mutation: the direction's sign
            dirv = -dirv
        dh = _norm(nh) / lab
        dirh = crh / (nn * lab)[:, None] + (_norm(nh) / nn)[:, None]
    w = 1.0 - wc * np.abs(d)
    wh = 1.0 + wc * dh
    c3 = d if variant == "distance_unweighted" else d * w  # mutation: the distance without its weight
    out = dict(w=w, d=d)
    with np.errstate(all="ignore"):
        out["corner_dir"] = _coeff_units(c[:, :3], dirv * w[:, None], EPS32 * (dirh * np.abs(w)[:, None] + np.abs(dirv) * wh[:, None])).max(1)
    out["corner_c3"] = _coeff_units(c[:, 3], c3, EPS32 * (dh * np.abs(w) + d * wh))
    out["ref_kept"] = w > 0.1
    out["margin_kept"] = _ratio(np.abs(w - 0.1), EPS32 * wh)
    out["corner_kept"] = np.where(out["ref_kept"] != np.asarray(kept, bool), out["margin_kept"], 0.0)
    return out


def surf_check(plane, X, coeff, kept, variant=None):
    """The fit's float32 coefficient and kept bit, from ITS float32 plane (N, 4) and the point X."""
    pl, X, c = _f64(plane), _f64(X)[:, :3], _f64(coeff)
    nh, Dh = pl[:, :3], pl[:, 3]
    d = (nh * X).sum(1) + Dh
    dh = (np.abs(nh) * np.abs(X)).sum(1) + np.abs(Dh)
    xn = _norm(X)
    wc = 0.8 if variant == "weight_08" else 0.9
    with np.errstate(all="ignore"):
        root = xn if variant == "abs_for_sqrt" else np.sqrt(xn)  # mutation: |X| for sqrt(|X|)
        w = 1.0 - wc * np.abs(d) / root
        wh = 1.0 + wc * dh / root
    c3 = d if variant == "distance_unweighted" else d * w
    out = dict(w=w, d=d)
    out["surf_normal"] = _coeff_units(c[:, :3], nh * w[:, None], EPS32 * np.abs(nh) * wh[:, None]).max(1)
    out["surf_c3"] = _coeff_units(c[:, 3], c3, EPS32 * (dh * np.abs(w) + np.abs(d) * wh))
    out["ref_kept"] = w > 0.1
    out["margin_kept"] = _ratio(np.abs(w - 0.1), EPS32 * wh)
    out["surf_kept"] = np.where(out["ref_kept"] != np.asarray(kept, bool), out["margin_kept"], 0.0)
    return out


# ---------------------------------------------------------------------------
# whole stages: what both test files run on a fit's outputs
# ---------------------------------------------------------------------------
def check_planes(nb, x, plane, coeff, matched, kept, variant=None):
    """-> {criterion: units (N,), NaN where the criterion does not apply} plus 'undetermined' (bool) and the margins.
    The coefficient criteria apply where the fit matched (it computes no coefficient elsewhere)."""
    m = np.asarray(matched, bool)
    r = plane_check(nb, plane, m, variant)
    out = {k: r[k] for k in ("plane_norm", "plane_d", "plane_matched")}
    und = ~(K["plane_normal"] * r["u_n"] <= UNDETERMINED)
    out["plane_normal"] = np.where(und, np.nan, r["plane_normal"])
    s = surf_check(plane, x, coeff, kept, variant)
    nan = np.where(m, 0.0, np.nan)
    for k in ("surf_normal", "surf_c3", "surf_kept"):
        out[k] = s[k] + nan
    out.update(undetermined=und, sin=r["sin"], margin_matched=r["margin_matched"], margin_kept=s["margin_kept"] + nan,
               ref_matched=r["ref_matched"], ref_kept=s["ref_kept"])
    return out


def check_lines(nb, x, A, B, coeff, matched, kept, variant=None):
    m = np.asarray(matched, bool)
    r = line_check(nb, A, B, m, variant)
    out = {k: r[k] for k in ("line_centre", "line_direction", "line_length", "line_matched")}
    c = corner_check(A, B, x, coeff, kept, variant)
    nan = np.where(m, 0.0, np.nan)
    for k in ("corner_dir", "corner_c3", "corner_kept"):
        out[k] = c[k] + nan
    out.update(sin=r["sin"], margin_matched=r["margin_matched"], margin_kept=c["margin_kept"] + nan, ref_matched=r["ref_matched"],
               ref_kept=c["ref_kept"], d=c["d"])
    return out


PLANE_CRITERIA = ("plane_normal", "plane_norm", "plane_d", "plane_matched", "surf_normal", "surf_c3", "surf_kept")
LINE_CRITERIA = ("line_centre", "line_direction", "line_length", "line_matched", "corner_dir", "corner_c3", "corner_kept")


def worst(units):
    """The largest value of a units array, NaNs (not applicable) aside; 0 for an empty one."""
    u = np.asarray(units, np.float64)
    u = u[~np.isnan(u)]
    return float(u.max()) if len(u) else 0.0


def worst_per_cell(res, cell, n_cells, criteria):
    """-> {criterion: [worst of cell 0, ...]}"""
    return {k: [worst(res[k][cell == i]) for i in range(n_cells)] for k in criteria}


def table(res, bank, criteria, title):
    """The printed table: one row per cell, one column per criterion, the worst units."""
    per = worst_per_cell(res, bank["cell"], len(bank["cells"]), criteria)
    lines = [title, "  %-22s" % "cell (d, aspect, sigma)" + "".join("%16s" % k for k in criteria)]
    for i, cdef in enumerate(bank["cells"]):
        lines.append("  %-22s" % (cdef,) + "".join("%16.3g" % per[k][i] for k in criteria))
    lines.append("  %-22s" % "all" + "".join("%16.3g" % worst(res[k]) for k in criteria))
    return "\n".join(lines)
