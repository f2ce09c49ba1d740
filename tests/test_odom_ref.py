"""The references of tests/odom_ref.py checked on the CPU, on the input families the GPU tests of
tests/test_gpu_odom_general.py use: the brute-force correspondences against the C oracle's kd-tree + walk, the seeded
mutations, and the measured values behind every bar of the GPU tests.

Recorded figures (the families of odom_ref.families on the 16 x 900 scene; each is printed and asserted below):

  correspondences   oracle_odom_corr == corr_ref index for index on all 26 families (33 000 queries); no query ties at its
                    nearest point on any family, the far ones included (fp32 spacing 2**-8 m at 50 km against 2 cm of range
                    noise), so nothing is left out of the index comparison; the `walk_ties` family has equal distances
                    inside the ring windows only
  SEL_UNITS = 29    the oracle's fp32 transformToStart against to_start64: max 3.21 units of
                    2**-24 (sum_j |R_ij| |q_j| + |t_i|) (derivation: odom_ref.SEL_UNITS)
  conditioning      max over points of |oracle fp32 coefficient - coeff64| / max(|d|, 2**-24 |X|), per family:
                    odom_ref.COEFF_COND (between 1.1e-7 for the single flat row and 1.3e-2 on the 16 000-query clouds, where
                    the three points of a plane come from a 1 500-point cloud and nearly lie on a line); the GPU bar of the
                    independent coefficient check is four times the family's value
  fp32 floor        fp32 rows + numpy pairwise fp32 sums against sums64_odom: max 3.15 units u[k] (the single flat row of
                    ragged_0_1: a row's own rounding, no sum); FLOOR_PAIRWISE_ODOM = 3.2
  K_ODOM = 34       max(10 x 3.2 = 32, a-priori 34): the derivation is odom_ref.k_odom_apriori's docstring

Mutations of a COPY of the reference (queries whose correspondence changes / families of the 24 small ones that see it):

  q5_bound_is_cloud_size       up to 384 of 560 queries, 20 families     ring_window_1    up to 115, 17 families
  flat_second_point_any_ring   up to 321, 21 families                    tie_takes_last   25 queries, walk_ties only
  no_weight_from_iter_5        every sum with iter >= 5 moves by > 1e4 units
  b_is_minus_d                 the six J^T r sums move by 19 x their value (> 1e6 units)
"""
import numpy as np
import pytest

import odom_ref as O
import scanmatch_ref as R


def oracle_step(oracle, f, it=0):
    """The oracle's taps of one family: sel, ind, coeff, kept in tap order (sharp then flat)."""
    ns, nf = len(f["sharp"]), len(f["flat"])
    q = np.concatenate([f["sharp"], f["flat"]])
    sel = oracle.odom_to_start(f["pose"], q)
    ind = np.concatenate([oracle.odom_corr(f["lc"], sel[:ns], ns, False), oracle.odom_corr(f["ls"], sel[ns:], nf, True)], axis=1)
    return q, sel, ind


def oracle_coeff(oracle, f, sel, ind, it):
    ns = len(f["sharp"])
    cs, ks = oracle.odom_coeff(f["lc"], sel[:ns], ind[:, :ns], False, it)
    cf, kf = oracle.odom_coeff(f["ls"], sel[ns:], ind[:, ns:], True, it)
    return np.concatenate([cs, cf]), np.concatenate([ks, kf])


def conditioning(oracle, f, sel, ind):
    """Largest coeff_distance of the oracle's coefficients from coeff64 at the oracle's sel, over the family's iterations."""
    ns = len(f["sharp"])
    worst = 0.0
    for it in f["iters"]:
        co, ko = oracle_coeff(oracle, f, sel, ind, it)
        c64, k64, d, have = O.coeff64_step(f["lc"], f["ls"], sel, ind, ns, it)
        ok = have & (d > 0)
        if ok.any():
            worst = max(worst, O.coeff_distance(co[ok], c64[ok], d[ok], sel[ok]).max())
    return worst


@pytest.fixture(scope="module")
def prepared(synth, small_problem, oracle):
    """Every family with the oracle's sel and correspondences and the reference's, computed once."""
    out = []
    for f in O.families(synth, small_problem["world"]):
        q, sel, ind = oracle_step(oracle, f)
        ns, nf = len(f["sharp"]), len(f["flat"])
        ref, tie = O.corr_ref(f["lc"], f["ls"], sel[:ns], sel[ns:], ns, nf)
        out.append(dict(f, q=q, sel=sel, ind=ind, ref=ref, tie=tie))
    return out


def test_oracle_correspondences_equal_the_brute_force_reference(prepared):
    """oracle_odom_corr (kd-tree + the walks of :366-403 / :430-477, the code oracle_odometry_match runs) against corr_ref
    (brute force, no tree, no shared code), index for index on every family.  A query that ties at its nearest point is
    compared through the tie flag only; at most 2 % of a family may (measured: none on any family)."""
    names = [f["name"] for f in prepared]
    assert len(set(names)) == len(names) and {"far_3km", "far_10km", "far_50km", "sparse_2_to_4.9m", "walk_ties"} <= set(names)
    total = 0
    for f in prepared:
        tie = f["tie"]
        assert tie.mean() <= O.TIE_SHARE if len(tie) else True, (f["name"], tie.mean())
        if not f["name"].startswith("far_"):
            assert not tie.any(), f["name"]
        bad = (f["ind"] != f["ref"]).any(axis=0) & ~tie
        assert not bad.any(), (f["name"], np.flatnonzero(bad)[:5], f["ind"][:, bad][:, :5], f["ref"][:, bad][:, :5])
        total += len(tie)
        print("%-26s %5d queries, %d ties, closest %d second %d third %d" % (f["name"], len(tie), tie.sum(), (f["ref"][0] >= 0).sum(),
                                                                             (f["ref"][1] >= 0).sum(), (f["ref"][2] >= 0).sum()))
    # every family but the one-query ones finds second and third points: the walks are exercised, not skipped
    for f in prepared:
        if len(f["flat"]) > 30:
            assert (f["ref"][2] >= 0).sum() > 0 and (f["ref"][1] >= 0).sum() > 0, f["name"]
    assert total > 30000
    # the families do what they are named for
    by = {f["name"]: f for f in prepared}
    f = by["q5_few_sharp"]
    assert (f["ref"][0, :3] + 1 >= 3).all()        # closest + 1 >= n_sharp: the forward walk of every sharp query is empty
    assert len(by["q5_more_sharp_than_cloud"]["sharp"]) > len(by["q5_more_sharp_than_cloud"]["lc"])
    assert len(by["guard_edge"]["lc"]) == 11 and len(by["guard_edge"]["ls"]) == 101
    r = np.floor(by["rings_0_to_255"]["ls"][:, 3])
    assert r.min() == 0 and r.max() == 255
    assert np.floor(by["rings_above_255"]["ls"][:, 3]).min() >= 300
    assert (np.diff(np.floor(by["not_ring_order"]["ls"][:, 3])) < 0).any()
    assert not np.isin((3, 4, 9), np.floor(by["empty_rings"]["ls"][:, 3])).any()
    assert np.abs(by["far_10km"]["ls"][:, :2]).min() >= 8192.0 and np.abs(by["far_50km"]["ls"][:, 0]).min() >= 8192.0 * 5.02


@pytest.mark.parametrize("variant", O.CORR_VARIANTS)
def test_every_seeded_correspondence_variant_is_seen(prepared, variant):
    """A mutated copy of corr_ref differs from corr_ref (hence from the oracle, which equals it) in at least one index on at
    least one family: a test built on the index comparison sees the mutation."""
    seen = {}
    for f in prepared:
        if len(f["flat"]) > 1000:
            continue
        ns, nf = len(f["sharp"]), len(f["flat"])
        mut, _ = O.corr_ref(f["lc"], f["ls"], f["sel"][:ns], f["sel"][ns:], ns, nf, variant=variant)
        n = int((mut != f["ref"]).any(axis=0).sum())
        if n:
            seen[f["name"]] = n
    print(variant, seen)
    assert seen, variant
    if variant == "q5_bound_is_cloud_size":
        assert "q5_few_sharp" in seen and "q5_more_sharp_than_cloud" in seen
    if variant == "tie_takes_last":
        assert "walk_ties" in seen


def test_seeded_coefficient_and_sum_variants_are_seen(prepared, oracle):
    """no_weight_from_iter_5 moves coeff64 (and with it the sums) away from the oracle's coefficients by far more than the
    conditioning bar at iter 5, and not at all at iter 4; b_is_minus_d moves the six J^T r sums by more than K_ODOM units."""
    f = next(f for f in prepared if f["name"] == "pose_drive")
    ns = len(f["sharp"])
    for it, moved in ((4, False), (5, True)):
        co, ko = oracle_coeff(oracle, f, f["sel"], f["ind"], it)
        c64, k64, d, have = O.coeff64_step(f["lc"], f["ls"], f["sel"], f["ind"], ns, it)
        cm, km, _, _ = O.coeff64_step(f["lc"], f["ls"], f["sel"], f["ind"], ns, it, variant="no_weight_from_iter_5")
        dist = O.coeff_distance(co[have], cm[have], d[have], f["sel"][have]).max()
        assert (dist > 100 * 4 * O.COEFF_COND["pose_drive"]) == moved, (it, dist)
        S, u = O.sums64_odom(f["pose"], f["q"], co, ko)
        Sm, _ = O.sums64_odom(f["pose"], f["q"], cm.astype(np.float32), km)
        assert (R.units(Sm, S, u).max() > 100 * O.K_ODOM) == moved, it
        Sb, _ = O.sums64_odom(f["pose"], f["q"], co, ko, variant="b_is_minus_d")
        un = R.units(Sb, S, u)
        assert un[21:].min() > 100 * O.K_ODOM and un[:21].max() == 0.0


def test_fp32_sel_lies_inside_the_derived_bound(prepared):
    """The oracle's float32 transformToStart against to_start64, in units 2**-24 (sum_j |R_ij| |q_j| + |t_i|): inside
    SEL_UNITS = 29 (the operation count of the quaternion route, odom_ref.SEL_UNITS) on every family.  Measured maximum: 3.21
    (0 at the zero pose and at relative time 0, where the rotation is the identity and sel = q)."""
    worst = 0.0
    for f in prepared:
        s64, mag = O.to_start64(f["pose"], f["q"])
        un = O.sel_units(f["sel"], s64, mag)
        worst = max(worst, un.max())
        assert un.max() <= O.SEL_UNITS, (f["name"], un.max())
        if f["name"] in ("pose_zero", "reltime_0"):
            assert np.array_equal(f["sel"], f["q"][:, :3])
    print("sel: largest distance %.2f units (bound %.0f)" % (worst, O.SEL_UNITS))
    assert worst > 1.0  # the comparison is not vacuous


def test_coefficient_conditioning_per_family(prepared, oracle):
    """How far the oracle's float32 coefficients lie from coeff64 at the same sel and indices, relative to
    max(|d|, 2**-24 |X|), per family and over the family's iterations (conditioning()) -- the conditioning of the line / plane fit, which the
    GPU test's independent bar (4 x the value recorded in odom_ref.COEFF_COND) rests on.  The kept flags agree everywhere but
    where the three points of a plane lie on one lattice line (walk_ties: the normal is 0 / 0 in float32)."""
    for f in prepared:
        ns = len(f["sharp"])
        for it in f["iters"]:
            co, ko = oracle_coeff(oracle, f, f["sel"], f["ind"], it)
            c64, k64, d, have = O.coeff64_step(f["lc"], f["ls"], f["sel"], f["ind"], ns, it)
            assert not ko[~have].any() and not co[~have].any()
            if f["name"] != "walk_ties":
                assert np.array_equal(ko, k64), (f["name"], it)
        worst = conditioning(oracle, f, f["sel"], f["ind"])
        print("%-26s conditioning %.3g (recorded %.3g)" % (f["name"], worst, O.COEFF_COND[f["name"]]))
        assert worst <= O.COEFF_COND[f["name"]], (f["name"], worst)
        assert worst >= 0.5 * O.COEFF_COND[f["name"]], (f["name"], worst)  # the record is the measurement, not a loose cap


def test_fp32_floor_and_k_odom(prepared, oracle):
    """The fp32 floor behind K_ODOM: float32 rows and numpy's pairwise float32 sums against sums64_odom on the oracle's taps,
    max over entries, families and iterations: 3.15 units measured (FLOOR_PAIRWISE_ODOM = 3.2).  Ten times that is 32; the
    a-priori count of the device's reduction is 34, so K_ODOM = 34."""
    worst = 0.0
    for f in prepared:
        for it in f["iters"]:
            co, ko = oracle_coeff(oracle, f, f["sel"], f["ind"], it)
            if not ko.any():
                continue
            S, u = O.sums64_odom(f["pose"], f["q"], co, ko)
            worst = max(worst, R.units(O.pairwise32_odom(f["pose"], f["q"], co, ko), S, u).max())
    print("fp32 pairwise floor %.2f units; K_ODOM %.0f" % (worst, O.K_ODOM))
    assert 0.5 * O.FLOOR_PAIRWISE_ODOM <= worst <= O.FLOOR_PAIRWISE_ODOM
    assert O.k_odom_apriori() == 34.0 and O.K_ODOM == max(10 * O.FLOOR_PAIRWISE_ODOM, 34.0) == 34.0


def test_oracle_match_still_runs_on_the_factored_functions(oracle, synth, small_problem):
    """oracle_odometry_match calls the functions the taps expose: its first iteration's row counts are the taps' kept counts."""
    f = next(f for f in O.families(synth, small_problem["world"]) if f["name"] == "pose_drive")
    q, sel, ind = oracle_step(oracle, f)
    co, ko = oracle_coeff(oracle, f, sel, ind, 0)
    n, pose, st = oracle.odometry_match(f["lc"], f["ls"], f["sharp"], f["flat"], f["pose"], max_iterations=1)
    ns = len(f["sharp"])
    assert (st.n_rows, st.n_line, st.n_plane) == (ko.sum(), ko[:ns].sum(), ko[ns:].sum())
