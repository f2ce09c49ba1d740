"""The oracle's mapping fit (Oracle.find_line, find_plane, corner_coeff, surf_coeff) through every criterion of tests/fit_ref.py
on the bank of tests/fit_cases.py -- CPU only.  This is where the constants K come from and where the reference shows what it
can see:

  * the bank's caps hold for the reference alone (planes whose direction the data do not determine; lines inside the verdict's
    band), before any fit is looked at;
  * the oracle stays within K / 4 of float64 in every criterion and cell (the printed tables are DESIGN.md's), the recorded worst
    values of fit_ref.MEASURED are this run's, and no derived count lies below them;
  * every mutation of fit_ref.VARIANTS is seen: at least one case further than K from the mutated reference, or a verdict that
    differs outside its band.  Which cells see which (this run; `-s` prints the counts):
      ratio_3              line verdict: the sigma = 0.15 cells at every distance (about 70 of 400 each) and a handful at 0.08; no
                           cell with sigma <= 0.03 has a line between the two ratios
      middle_eigenvector   line direction, every cell
      offset_009           line length, every cell; the corner coefficient does not see it (the line is the same line)
      d_first_neighbour    plane D, every cell with noise (nearly every fit); not the noise-free cells, whose first neighbour
                           lies in the plane
      tls_normal           plane normal, the cells with noise: nearly every fit out to 5 m, 122 .. 296 of 300 at 50 m; at 300 m
                           and 420 m the unit u_n has grown to the tilt between the two planes -- with sigma = 0.01 and aspect 1
                           2 of 300 fits see it at 300 m and none at 420 m (73 .. 97 at aspect 0.1), with sigma = 0.05 200 ..
                           270.  Not the noise-free cells, where the two planes are one
      inlier_025           plane verdict: the sigma = 0.05, aspect 1 cells only, one to three fits each (nothing else has a
                           residual between 0.2 and 0.25)
      weight_08            both coefficients, every cell
      abs_for_sqrt         surf coefficient, every cell
      corner_negated       corner direction, every cell
      distance_unweighted  both coefficients' fourth entry, every cell
"""
import numpy as np
import pytest

import fit_cases as cases
import fit_ref as ref


@pytest.fixture(scope="module")
def fitted(oracle):
    """The two banks and the oracle's fits of them, computed once: dict(planes=(bank, out12, flags, x), lines=...)."""
    pb, lb = cases.plane_bank(), cases.line_bank()
    po, pf, px = cases.oracle_fit_stage(oracle, pb["nb"], pb["x"], 1)
    lo, lf, lx = cases.oracle_fit_stage(oracle, lb["nb"], lb["x"], 0, lb["on_line"])
    return dict(planes=(pb, po, pf, px), lines=(lb, lo, lf, lx))


def check(fitted, variant=None):
    pb, po, pf, px = fitted["planes"]
    lb, lo, lf, lx = fitted["lines"]
    pr = ref.check_planes(pb["nb"], px, po[:, :4], po[:, 8:], pf & cases.MATCHED, pf & cases.KEPT, variant)
    lr = ref.check_lines(lb["nb"], lx, lo[:, :3], lo[:, 3:6], lo[:, 8:], lf & cases.MATCHED, lf & cases.KEPT, variant)
    return pr, lr


def test_caps_hold_for_the_reference_alone():
    """At most 5 % of the planes, and at most 25 % of any cell, have a direction the data do not determine (K_n u_n > 0.1 rad);
    at most 1 % of the lines lie inside the verdict's band.  Nothing but the float64 reference takes part."""
    pb, lb = cases.plane_bank(), cases.line_bank()
    assert len(pb["nb"]) == 39 * cases.PLANE_PER_CELL and len(lb["nb"]) == 25 * cases.LINE_PER_CELL
    und = ref.K["plane_normal"] * ref.plane_reference(pb["nb"])["u_n"] > ref.UNDETERMINED
    per_cell = [und[pb["cell"] == i].mean() for i in range(len(pb["cells"]))]
    print("planes left out of the direction check: %.2f %% overall; worst cell %s: %.1f %%"
          % (100 * und.mean(), pb["cells"][int(np.argmax(per_cell))], 100 * max(per_cell)))
    assert und.mean() <= 0.05 and max(per_cell) <= 0.25
    lr = ref.line_reference(lb["nb"])
    band = lr["margin_matched"] <= ref.K["line_matched"]
    print("lines inside the verdict's band: %d of %d; accepted: %.1f %%" % (band.sum(), len(band), 100 * lr["matched"].mean()))
    assert band.mean() <= 0.01
    assert lr["matched"].any() and not lr["matched"].all()  # both verdicts occur


def test_oracle_within_a_quarter_of_k(fitted):
    pr, lr = check(fitted)
    pb, lb = fitted["planes"][0], fitted["lines"][0]
    print(ref.table(pr, pb, ref.PLANE_CRITERIA, "planes: the oracle's worst units per cell"))
    print(ref.table(lr, lb, ref.LINE_CRITERIA, "lines: the oracle's worst units per cell"))
    for d in (300.0, 420.0):
        far = np.array([c[0] == d for c in pb["cells"]])[pb["cell"]]
        thin = np.array([c[0] == d and c[1] == 0.1 for c in pb["cells"]])[pb["cell"]]
        print("normal's worst error at %g m: %.2e rad (aspect 0.1: %.2e rad); line direction's: %.2e rad"
              % (d, np.nanmax(pr["sin"][far & ~thin]), np.nanmax(pr["sin"][thin]),
                 np.nanmax(lr["sin"][np.array([c[0] == d for c in lb["cells"]])[lb["cell"]]])))
    for res, criteria in ((pr, ref.PLANE_CRITERIA), (lr, ref.LINE_CRITERIA)):
        for name in criteria:
            got, (recorded, derived), k = ref.worst(res[name]), ref.MEASURED[name], ref.K[name]
            assert got <= k / 4.0, (name, got, k)
            assert got <= derived, (name, got, "the derivation is wrong")
            # the recorded worst (what K is ten times of) is this bank's, rounded up in its second or third digit
            assert got <= recorded <= 1.15 * got + 1e-9, (name, got, recorded)


def test_both_sides_of_every_verdict_occur(fitted):
    pb, po, pf, px = fitted["planes"]
    lb, lo, lf, lx = fitted["lines"]
    for name, fl in (("planes", pf), ("lines", lf)):
        m, k = (fl & cases.MATCHED) != 0, (fl & cases.KEPT) != 0
        print(name, "matched %.1f %%, of those kept %.1f %%" % (100 * m.mean(), 100 * k[m].mean()))
        assert m.any() and (~m).any() and k[m].any() and (~k[m]).any()
    # the d = 0 rows: direction 0/0, distance 0, kept
    rows = lb["on_line"]
    assert len(rows) == 20 and np.all((lf[rows] & cases.MATCHED) != 0)
    assert np.isnan(lo[rows, 8:11]).all() and np.all(lo[rows, 11] == 0.0) and np.all((lf[rows] & cases.KEPT) != 0)
    lr = check(fitted)[1]
    assert np.all(lr["d"][rows] == 0.0) and np.all(lr["corner_dir"][rows] == 0.0)


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_every_mutation_is_seen(fitted, variant):
    pr, lr = check(fitted, variant)
    pb, lb = fitted["planes"][0], fitted["lines"][0]
    seen = {}
    for res, bank, criteria in ((pr, pb, ref.PLANE_CRITERIA), (lr, lb, ref.LINE_CRITERIA)):
        for name in criteria:
            with np.errstate(invalid="ignore"):
                over = np.nan_to_num(res[name], nan=0.0) > ref.K[name]
            if over.any():
                seen[name] = [(bank["cells"][i], int(over[bank["cell"] == i].sum())) for i in range(len(bank["cells"])) if over[bank["cell"] == i].any()]
    for name, cells_ in seen.items():
        print(variant, "seen by", name, "in %d cells:" % len(cells_), cells_)
    assert seen, variant


def test_oracle_answers_the_degenerate_sets(oracle):
    """The sets float64 has no answer for: the oracle returns (it is what the device is held to on them), and says what
    tests/test_gpu_fit_general.py expects of some: no line through coincident points, a NaN plane from a NaN coordinate."""
    names, nb, x = cases.degenerate_sets()
    assert len(set(names)) == len(names)
    po, pf, _ = cases.oracle_fit_stage(oracle, nb, x, 1)
    lo, lf, _ = cases.oracle_fit_stage(oracle, nb, x, 0)
    for i, name in enumerate(names):
        print("%-26s plane %s %s | line %s %s" % (name, bool(pf[i] & cases.MATCHED), po[i, :4], bool(lf[i] & cases.MATCHED), lo[i, :6]))
    i = names.index("coincident")
    assert not (lf[i] & cases.MATCHED)
    assert np.isnan(po[names.index("nan_31"), :4]).any()
