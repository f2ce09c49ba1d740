"""tests/occupancy_ref.py held to itself, on the CPU: the crossed set's definition against its properties, the int64 form and
the kernel's per-column closed form against the definition, the value formula, fit_bounds."""
from fractions import Fraction

import numpy as np
import pytest

import occupancy_ref as R

LATTICES = (1, 64, 128, 256)


def _segments(lattice, n, seed, span=5):
    """n segments with ends on multiples of `lattice` fixed-point units within +-span cells: walls and corners are hit often."""
    rng = np.random.default_rng(seed)
    m = (span * 256) // lattice
    pts = rng.integers(-m, m + 1, (n, 4)) * lattice
    out = [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in pts]
    # the special shapes, on every lattice: zero length (interior, wall, corner), along a grid line, diagonals through corners
    L = lattice
    out += [((L, L), (L, L)), ((256, L), (256, L)), ((256, 512), (256, 512)), ((0, 256), (1024, 256)), ((256, -512), (256, 768)),
            ((0, 0), (768, 768)), ((0, 768), (768, 0)), ((L, 0), (L + 512, 512)), ((-256 - L, L), (512 + L, L)),
            ((L, L), (L + 256, L)), ((256, L), (512, L + 256)), ((3, 5), (3, 900)), ((900, 7), (-900, 7))]
    return out


@pytest.mark.parametrize("lattice", LATTICES)
def test_crossed_set_is_symmetric_and_matches_its_int64_and_column_forms(lattice):
    for A, B in _segments(lattice, 300, 10 + lattice):
        want = R.crossed_exact(A, B)
        assert R.crossed_exact(B, A) == want, (A, B)
        assert R.crossed_columns(A, B) == want, (A, B)
        assert R.crossed_columns(B, A) == want, (A, B)
        # the int64 form over a grid shifted so that the box lies inside it, and over one that cuts the box
        for (oi, oj, W, H) in ((-6, -6, 13, 13), (-2, 0, 5, 4)):
            a, b = (A[0] - 256 * oi, A[1] - 256 * oj), (B[0] - 256 * oi, B[1] - 256 * oj)
            m = R.crossed_mask(a, b, W, H)
            got = {(int(i) + oi, int(j) + oj) for j, i in zip(*np.nonzero(m))}
            assert got == {c for c in want if oi <= c[0] < oi + W and oj <= c[1] < oj + H}, (A, B)


@pytest.mark.parametrize("lattice", LATTICES)
def test_crossed_set_against_samples_and_witnesses(lattice):
    """Every point of a 1/8-cell sampling of the segment that lies in an open cell interior lies in a crossed cell, and every
    crossed cell has a rational witness: a t in (0, 1) whose point lies in the cell's open interior."""
    for A, B in _segments(lattice, 120, 50 + lattice):
        want = R.crossed_exact(A, B)
        dx, dy = B[0] - A[0], B[1] - A[1]
        n = max(1, (max(abs(dx), abs(dy)) + 31) // 32)
        for k in range(1, n):
            x, y = A[0] + Fraction(k * dx, n), A[1] + Fraction(k * dy, n)
            if x % 256 != 0 and y % 256 != 0:
                assert (int(x // 256), int(y // 256)) in want, (A, B, k)
        for (i, j) in want:
            tx, ty = R._t_interval(A[0], dx, i), R._t_interval(A[1], dy, j)
            lo, hi = max(tx[0], ty[0], Fraction(0)), min(tx[1], ty[1], Fraction(1))
            assert lo < hi
            t = (lo + hi) / 2
            x, y = A[0] + t * dx, A[1] + t * dy
            assert 0 < t < 1 and 256 * i < x < 256 * (i + 1) and 256 * j < y < 256 * (j + 1), (A, B, i, j)


def test_the_stated_special_cases():
    assert R.crossed_exact((10, 10), (10, 10)) == {(0, 0)}            # zero length inside a cell
    assert R.crossed_exact((256, 10), (256, 10)) == set()              # ... on a wall
    assert R.crossed_exact((0, 256), (2048, 256)) == set()             # along a grid line
    assert R.crossed_exact((0, 0), (512, 512)) == {(0, 0), (1, 1)}     # through a lattice corner: not the two it touches
    assert R.crossed_exact((100, 100), (256, 100)) == {(0, 0)}         # B on a wall reached from the left: end cell 1 not crossed
    assert (256 >> 8, 100 >> 8) == (1, 0)
    assert R.crossed_exact((400, 100), (256, 100)) == {(1, 0)}         # ... from the right: end cell crossed


def test_long_rays_at_the_fixed_point_bound():
    """The cross-multiplied products fit int64 at the far corners of the admitted range: 32 x 32 cell windows at the ray's
    start, middle and end, every cell against the Fraction form."""
    lim = R.FIX
    for A, B in (((-lim, -lim), (lim - 1, lim - 1)), ((lim - 1, -lim), (-lim, lim - 7)), ((-lim, 5), (lim - 1, 6)),
                 ((-lim, lim - 1), (lim - 1, lim - 300))):
        n_crossed = 0
        for t in (Fraction(0), Fraction(1, 2), Fraction(1)):
            oi = int((A[0] + t * (B[0] - A[0])) // 256) - 16
            oj = int((A[1] + t * (B[1] - A[1])) // 256) - 16
            m = R.crossed_mask((A[0] - 256 * oi, A[1] - 256 * oj), (B[0] - 256 * oi, B[1] - 256 * oj), 32, 32)
            for j in range(32):
                for i in range(32):
                    assert bool(m[j, i]) == R.cell_crossed_exact(A, B, i + oi, j + oj), (A, B, i + oi, j + oj)
            n_crossed += int(m.sum())
        assert n_crossed >= 48


@pytest.mark.parametrize("hit_weight", range(1, 17))
def test_value_formula(hit_weight):
    nh, nf = np.meshgrid(np.arange(65), np.arange(65), indexing="ij")
    for min_obs in (1, 3):
        v = R.values(nh, nf, hit_weight, min_obs)
        for h in range(65):
            for f in range(65):
                want = R.value(h, f, hit_weight, min_obs)
                assert v[h, f] == want
                if h + f < min_obs:
                    assert want == -1
                else:
                    H, D = hit_weight * h, hit_weight * h + f
                    assert 0 <= want <= 100 and abs(Fraction(100 * H, D) - want) <= Fraction(1, 2)  # round(100 H / D)


@pytest.mark.parametrize("up_axis", [1, 2])
def test_fit_bounds_holds_every_pose_and_is_minimal(up_axis):
    rng = np.random.default_rng(3)
    for res, max_range, span in ((0.1, 40.0, 100.0), (0.25, 10.0, 3.0), (0.05, 30.0, 50.0), (0.3, 7.0, 1000.0)):
        for n in (1, 2, 17):
            poses = np.tile(np.eye(4), (n, 1, 1))
            poses[:, :3, 3] = rng.uniform(-span, span, (n, 3))
            p = R.params(resolution=res, max_range=max_range, up_axis=up_axis)
            origin, w, h, spans = R.fit_bounds(poses, p)
            r = float(np.float32(res))
            for org, cells, (lo, hi), row in zip(origin, (w, h), spans, R.rows(p)):
                o = poses.astype(np.float32)[:, row, 3].astype(np.float64)
                assert lo == (o - float(np.float32(max_range))).min() and hi == (o + float(np.float32(max_range))).max()
                assert org <= lo and org + cells * r >= hi                 # holds every pose +- max_range
                assert (round(org / r) + 1) * r > lo and (cells == 1 or org + (cells - 1) * r < hi)  # one cell less on either side would not
                assert abs(org / r - round(org / r)) < 1e-6               # the origin is a multiple of the resolution
