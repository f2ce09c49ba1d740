"""The mapping fit on the device -- find_line, find_plane, corner_coeff, surf_coeff of csrc/lslam_device.hpp through the tap
lslam_debug_fit_stage (one fit per lane, the general instantiation and the in-range one) -- held to the float64 reference of
tests/fit_ref.py on the bank of tests/fit_cases.py: patches from 0.5 m to 420 m from the origin, square to nearly collinear,
noise-free to 5 cm (planes) and 15 cm (lines).  Every tolerance is a K of fit_ref (its docstring has unit, derived count and
the oracle's measured worst for each).  Beside float64: the oracle, bit for bit, on the whole bank and on the degenerate sets
float64 has no answer for; and the in-range instantiation's per-wavefront fallbacks with ONE lane of 64 outside the range.

Measured on an MI355X (this file, `-s`): see DESIGN.md 4, "How accurate the fit is".
"""
import numpy as np
import pytest

import fit_cases as cases
import fit_ref as ref

pytestmark = pytest.mark.gpu

INR_KEPT, GEN_KEPT, INR_MATCHED, GEN_MATCHED, REFUSED = 1, 2, 4, 8, 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Equal to the bit, NaNs in the same places (a NaN's payload and sign are the producer's: x86's 0/0 is not the GPU's)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def first_difference(a, b, names=None):
    bad = np.flatnonzero(~same(a, b).reshape(len(a), -1).all(1))
    if not len(bad):
        return None
    i = int(bad[0])
    return len(bad), (names[i] if names is not None else i), np.asarray(a)[i].tolist(), np.asarray(b)[i].tolist()


_cache = {}


def oracle_side(oracle):
    """The two banks and the oracle's fits of them (CPU), once per session: {0: (bank, out12, flags, x), 1: ...}; x has the
    listed points on the oracle's lines."""
    if "oracle" not in _cache:
        pb, lb = cases.plane_bank(), cases.line_bank()
        _cache["oracle"] = {1: (pb,) + cases.oracle_fit_stage(oracle, pb["nb"], pb["x"], 1),
                            0: (lb,) + cases.oracle_fit_stage(oracle, lb["nb"], lb["x"], 0, lb["on_line"])}
    return _cache["oracle"]


def check(which, bank, x, out, matched, kept):
    if which:
        return ref.check_planes(bank["nb"], x, out[:, :4], out[:, 8:], matched, kept), ref.PLANE_CRITERIA
    return ref.check_lines(bank["nb"], x, out[:, :3], out[:, 3:6], out[:, 8:], matched, kept), ref.LINE_CRITERIA


@pytest.mark.parametrize("which", [0, 1], ids=["lines", "planes"])
def test_bank_general_against_float64(ctx, oracle, which):
    """The general instantiation: every criterion of fit_ref within K units, the verdicts and kept bits float64's outside
    their bands (a verdict that differs counts its margin as its units)."""
    bank, _, _, x = oracle_side(oracle)[which]
    _, og, fl = ctx.fit_stage(bank["nb"], x, which)
    res, criteria = check(which, bank, x, og, fl & GEN_MATCHED, fl & GEN_KEPT)
    print(ref.table(res, bank, criteria, "%s: the device's worst units per cell" % ("planes" if which else "lines")))
    for d in (300.0, 420.0):
        far = np.array([c[0] == d for c in bank["cells"]])[bank["cell"]]
        print("worst direction error at %g m: %.2e rad" % (d, np.nanmax(res["sin"][far])))
    if which:
        print("left out of the direction check: %.2f %%" % (100 * res["undetermined"].mean()))
    for name in criteria:
        assert ref.worst(res[name]) <= ref.K[name], (name, ref.worst(res[name]), ref.K[name], int(np.nanargmax(res[name])))


@pytest.mark.parametrize("which", [0, 1], ids=["lines", "planes"])
def test_bank_inrange_equals_general(ctx, oracle, which):
    """The in-range instantiation: the general one's bits wherever the guard let the fit through (bit 4 clear; a line fit's
    groups fall back by themselves and never set it), the same verdicts everywhere."""
    bank, _, _, x = oracle_side(oracle)[which]
    oi, og, fl = ctx.fit_stage(bank["nb"], x, which)
    refused = (fl & REFUSED) != 0
    per_cell = [(c, int(refused[bank["cell"] == i].sum())) for i, c in enumerate(bank["cells"])]
    print("refused by the guard: %d of %d (%.2f %%); per cell:" % (refused.sum(), len(fl), 100 * refused.mean()), per_cell)
    if not which:
        assert not refused.any()
    assert np.array_equal((fl & INR_MATCHED) != 0, (fl & GEN_MATCHED) != 0)
    assert np.array_equal((fl & INR_KEPT) != 0, (fl & GEN_KEPT) != 0)
    assert first_difference(oi[~refused], og[~refused]) is None


@pytest.mark.parametrize("which", [0, 1], ids=["lines", "planes"])
def test_bank_against_the_oracle(ctx, oracle, which):
    """A, B, plane, coefficients and flags of the general instantiation: the oracle's, bit for bit, out to 420 m and on nearly
    collinear neighbourhoods -- the inputs that take the QR's rare branches."""
    bank, want, want_fl, x = oracle_side(oracle)[which]
    _, og, fl = ctx.fit_stage(bank["nb"], x, which)
    assert np.array_equal((fl & GEN_MATCHED) != 0, (want_fl & cases.MATCHED) != 0)
    assert np.array_equal((fl & GEN_KEPT) != 0, (want_fl & cases.KEPT) != 0)
    assert first_difference(og, want) is None


@pytest.mark.parametrize("which", [0, 1], ids=["lines", "planes"])
def test_degenerate_sets_against_the_oracle(ctx, oracle, which):
    """Collinear, coincident, all zero, a zero column, NaN, +-inf, 2^+-40, duplicates: float64 does not define these fits, so the
    device is held to the oracle to the bit, NaNs in the same places."""
    names, nb, x = cases.degenerate_sets()
    want, want_fl, _ = cases.oracle_fit_stage(oracle, nb, x, which)
    _, og, fl = ctx.fit_stage(nb, x, which)
    got_m, got_k = (fl & GEN_MATCHED) != 0, (fl & GEN_KEPT) != 0
    want_m, want_k = (want_fl & cases.MATCHED) != 0, (want_fl & cases.KEPT) != 0
    assert np.array_equal(got_m, want_m), [n for n, a, b in zip(names, got_m, want_m) if a != b]
    assert np.array_equal(got_k, want_k), [n for n, a, b in zip(names, got_k, want_k) if a != b]
    assert first_difference(og, want, names) is None


def mixed(oracle, kind):
    which = 1 if kind == "plane_floor" else 0
    m = cases.mixed_wavefronts(oracle_side(oracle)[which][0], kind)
    if len(m["on_line"]):  # the points that go onto their lines: the oracle's A of those few
        idx = np.arange(5, dtype=np.int32)
        for i in m["on_line"]:
            ok, A, _ = oracle.find_line(m["nb"][i], idx)
            assert ok
            m["x"][i, :3] = A
    return which, m


@pytest.mark.parametrize("kind", ["line_centroid", "corner_on_line"])
def test_one_lane_of_a_wavefront_outside_the_range(ctx, oracle, kind):
    """Groups of 64 bank elements with exactly one lane (0, 31 or 63) outside the in-range fit's range -- a centroid component
    summing to exactly 0 (find_line's first ballot), a point on its line (corner_coeff's) -- at n = 64 k, 64 k + 1 and 64 k + 63:
    the whole wavefront falls back, and every lane of it equals the general fit to the bit; the tail sizes, whose last wavefront
    ballots with inactive lanes, give what the full groups give."""
    which, m = mixed(oracle, kind)
    full = None
    for tail in reversed(cases.MIXED_TAILS):
        n = 64 * m["n_groups"] + tail
        oi, og, fl = ctx.fit_stage(m["nb"][:n], m["x"][:n], which)
        assert first_difference(oi, og) is None, (kind, tail)
        assert np.array_equal((fl & INR_MATCHED) != 0, (fl & GEN_MATCHED) != 0) and np.array_equal((fl & INR_KEPT) != 0, (fl & GEN_KEPT) != 0)
        rep = m["replaced"][m["replaced"] < n]
        assert np.all((fl[rep] & GEN_MATCHED) != 0)  # the replaced lanes are lines, so their coefficients are computed
        if kind == "corner_on_line":
            assert np.isnan(og[rep, 8:11]).all() and np.all(og[rep, 11] == 0.0) and np.all((fl[rep] & GEN_KEPT) != 0)
        if full is None:
            full = (oi, og, fl)
        else:
            assert first_difference(oi, full[0][:n]) is None and first_difference(og, full[1][:n]) is None
            assert np.array_equal(fl, full[2][:n])


def test_one_floor_lane_of_a_wavefront_is_refused(ctx, oracle):
    """... and a floor at z = 0 exactly (find_plane's guard, which does not fall back itself: the sweep kernels fit again):
    bit 4 is set in the replaced lane and in no lane that does not set it without the replacement; the other lanes' fits are
    what they are without it; tail sizes as above."""
    which, m = mixed(oracle, "plane_floor")
    bank = oracle_side(oracle)[which][0]
    plain = cases.mixed_wavefronts(bank, None)  # the same elements, none replaced
    _, pg, pfl = ctx.fit_stage(plain["nb"], plain["x"], which)
    full = None
    for tail in reversed(cases.MIXED_TAILS):
        n = 64 * m["n_groups"] + tail
        oi, og, fl = ctx.fit_stage(m["nb"][:n], m["x"][:n], which)
        rep = np.zeros(n, bool)
        rep[m["replaced"][m["replaced"] < n]] = True
        refused = (fl & REFUSED) != 0
        assert np.all(refused[rep])
        assert np.array_equal(refused[~rep], (pfl[:n][~rep] & REFUSED) != 0)
        print("tail", tail, "refused:", int(refused.sum()), "of them replaced:", int(rep.sum()))
        assert np.array_equal(fl[~rep], pfl[:n][~rep]) and first_difference(og[~rep], pg[:n][~rep]) is None
        ok = ~refused
        assert first_difference(oi[ok], og[ok]) is None
        if full is None:
            full = (oi, og, fl)
        else:
            assert first_difference(oi, full[0][:n]) is None and first_difference(og, full[1][:n]) is None
            assert np.array_equal(fl, full[2][:n])
