"""CPU checks of the feature extractor's CPU oracle (oracle/features_oracle.c) against tests/features_ref.py, an independent
float64 statement of ScanRegistration::extractFeatures, over the constructed bank of tests/features_cases.py:

  * the bank reaches every situation it was built for, on rings that are not ambiguous, and at most 10 % of its rings are;
  * on every unambiguous ring the oracle's marks, labels and three index lists are the reference's, its less-flat list has
    the reference's voxels in the reference's order with centroids inside the fp32 summation bound; its curvature is
    inside the derived bound everywhere and equal where the bound is 0 (dyadic rings);
  * every threshold of the extractor, one at a time: a one-parameter family is bisected on the oracle down to two adjacent
    fp32 values, and the float64 reference must place the rule's quantity at its threshold within the rule's band, with
    the flip in the stated direction;
  * the measured eigenvalue / direction bands of features_ref.py are re-measured and held."""
import numpy as np
import pytest

import features_cases as CS
import features_ref as R

U = 2.0 ** -24


@pytest.fixture(scope="module")
def bank():
    """[(call, reference result)], computed once and left unchanged"""
    return [(c, R.extract(c.cloud, c.ranges, c.params)) for c in CS.bank()]


def oracle_params(oracle, params):
    return params.apply(oracle.reg_params())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare_with_ref(got, ref, call, tag):
    """`got` (the oracle's or the device's dict) against the reference on the unambiguous rings of one call"""
    cloud, ranges = call.cloud, call.ranges
    key = {tuple(v): i for i, v in enumerate(_bits(cloud[:, :4]).tolist())}
    assert len(key) == len(cloud)
    ring_of = np.full(len(cloud), -1)
    for k, (a, b) in enumerate(ranges.tolist()):
        ring_of[a:b + 1] = k
    clear = ~ref["ambiguous"]
    # curvature: inside its derived bound everywhere, equal where the bound is 0
    err = np.abs(got["curvature"].astype(np.float64) - ref["curvature"])
    assert (err <= ref["curvature_bound"]).all(), (tag, "curvature", err.max())
    for k, (a, b) in enumerate(ranges.tolist()):
        if b < a or not clear[k]:
            continue
        s = slice(a, b + 1)
        assert np.array_equal(got["picked"][s], ref["picked"][s]), (tag, k, "picked")
        assert np.array_equal(got["label"][s], ref["label"][s]), (tag, k, "label")
    for name in ("sharp", "less_sharp", "flat"):
        idx = np.array([key[tuple(v)] for v in _bits(got[name]).tolist()], np.int64)  # KeyError: not a copy of an input point
        for k in np.nonzero(clear)[0]:
            assert np.array_equal(idx[ring_of[idx] == k], ref[name][ref["ring_of_" + name] == k]), (tag, k, name)
    # less flat: the copied field is ring + time / 4, so its centroid names the ring
    g = got["less_flat"].astype(np.float64)
    g_ring = np.floor(g[:, 3]).astype(np.int64)
    for k in np.nonzero(clear)[0]:
        rows = np.nonzero(ref["less_flat_ring"] == k)[0]
        mine = g[g_ring == k]
        assert len(mine) == len(rows), (tag, k, "voxel count", len(mine), len(rows))
        for row, r in zip(mine, rows):
            n = int(ref["less_flat_count"][r])
            if n == 1:
                assert np.array_equal(row, ref["less_flat"][r]), (tag, k, "unfiltered point")
                continue
            terms = np.abs(cloud[ref["less_flat_members"][r]][:, :4].astype(np.float64)).max(0)
            # n additions of terms up to max|term| (n u max|term| on the mean) and the division's rounding
            bound = n * U * terms + U * np.abs(ref["less_flat"][r])
            assert (np.abs(row - ref["less_flat"][r]) <= bound).all(), (tag, k, "centroid", row, ref["less_flat"][r])


def test_bank_reaches_what_it_was_built_for(bank):
    total, rings, ambiguous = {}, 0, 0
    for call, ref in bank:
        assert len(call.ranges) <= 64
        for a, b in call.ranges.tolist():
            assert b < a or b - a + 1 == 2560 or b - a + 1 <= 400
        rings += len(call.ranges)
        ambiguous += int(ref["ambiguous"].sum())
        for k, ev in enumerate(ref["events"]):
            if not ref["ambiguous"][k]:
                for name, n in ev.items():
                    total[name] = total.get(name, 0) + n
    short = {name: (total.get(name, 0), need) for name, need in CS.REQUIRED.items() if total.get(name, 0) < need}
    assert not short, short
    assert 10 * ambiguous <= rings, (ambiguous, rings)           # a condition on the inputs, not a tolerance
    assert ambiguous >= 1                                           # the flag is alive: one pole edge sits 23 um off the 0.08 m bound


def test_ties_are_picked_lowest_index_first(bank):
    """maxSurfaceFlat 4 and 2 on a wall of curvature exactly 0: the picks of a region are its lowest index and then every
    (curvatureRegion + 1)-th, the first that markAsPicked leaves"""
    for name, cap in (("default", 4), ("flat2", 2)):
        call, ref = next((c, r) for c, r in bank if c.name == name)
        k = next(k for k, ev in enumerate(ref["events"]) if ev.get("region_all_zero", 0) == call.params.n_feature_regions)
        a, b = call.ranges[k].tolist()
        flat = ref["flat"][ref["ring_of_flat"] == k]
        want = []
        for j in range(6):
            sp, ep = R.region_bounds(a, b, 5, 6, j)
            want += [sp + 6 * q for q in range(cap)]
        assert flat.tolist() == want


def test_oracle_matches_the_reference_on_the_bank(oracle, bank):
    for call, ref in bank:
        got = oracle.extract_features(call.cloud, call.ranges, oracle_params(oracle, call.params))
        compare_with_ref(got, ref, call, call.name)


# ---- measured bands -----------------------------------------------------------------------------------------------------
def _cov32(pts):
    """the fp32 covariance of pointClassify (:559-577) in the source's order of accumulation"""
    f = np.float32
    p = pts.astype(f)
    m = f(len(p))
    c = np.zeros(3, f)
    for q in p:
        c = (c + q).astype(f)
    c = (c / m).astype(f)
    A = np.zeros((3, 3), f)
    for q in p:
        a = (q - c).astype(f)
        for i in range(3):
            for j in range(i + 1):
                A[i, j] = f(A[i, j] + f(a[i] * a[j]))
    A = (A / m).astype(f)
    return np.tril(A) + np.tril(A, -1).T


def measure_eigen_bands(oracle, bank):
    worst_val = worst_dir = 0.0
    fits = 0
    for call, ref in bank:
        for fit in ref["fits"]:
            D, V = oracle.eig_sym3(_cov32(fit["pts"]))
            lam = fit["D"][2]
            if lam <= 0:
                continue
            fits += 1
            worst_val = max(worst_val, float(np.abs(D.astype(np.float64) - fit["D"]).max() / lam))
            if fit["D"][2] > 100 * fit["D"][1]:                       # the direction is only used behind this gate
                v = V[:, 2].astype(np.float64)
                worst_dir = max(worst_dir, float(np.arcsin(np.linalg.norm(np.cross(v, fit["v"])) / np.linalg.norm(v))))
    return worst_val, worst_dir, fits


def test_measured_eigen_bands(oracle, bank):
    val, ang, fits = measure_eigen_bands(oracle, bank)
    print("eigenvalue error / lambda_max %.3e, direction %.3e rad over %d fits" % (val, ang, fits))
    assert fits > 1000
    assert val <= R.MEASURED_EIG_REL and ang <= R.MEASURED_DIR_RAD
    assert R.EIG_BAND == 4 * R.MEASURED_EIG_REL and R.DIR_BAND == 4 * R.MEASURED_DIR_RAD


# ---- thresholds ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs(oracle):
    return CS.threshold_pairs(oracle)


def _xyz(p):
    return np.asarray(p, np.float32).astype(np.float64)


def test_blind_angle_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["blind"]
    assert not at_lo                                                # a wider gap is blind
    thr = R.f32(R.Params().blind_threshold)
    assert abs(thr - np.cos(np.deg2rad(0.5))) < 2 * U              # cos of half a degree, stored in a float
    for t in (lo, hi):
        p = _xyz(CS.fam_blind(t))
        q, bound = R.calc_cos_angle_diff(p[19], p[20])
        assert abs(q - thr) <= 4 * bound, (q, thr)


def test_diff_next_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["diff_next"]
    assert not at_lo                                                # a larger jump is an occlusion
    for t in (lo, hi):
        p = _xyz(CS.fam_diff_next(t))
        q, bound = R.calc_squared_diff(p[20], p[19])
        assert abs(q - 1.0) <= 4 * 5 * U * q, q


def test_ratio_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["ratio"]
    assert at_lo                                                    # a close previous point makes the edge a broken one
    for t in (lo, hi):
        p = _xyz(CS.fam_ratio(t))
        q = R.calc_squared_diff(p[18], p[19])[0] / R.calc_squared_diff(p[20], p[19])[0]
        assert abs(q - 0.2) <= 44 * U * q, q


def test_depth_order_flips_where_float64_says(oracle, pairs):
    lo, hi, at_lo, at_hi = pairs["depth"]
    assert not at_lo                                                # next point nearer: the points BEFORE the jump are blocked
    for t, after in ((lo, False), (hi, True)):
        p = _xyz(CS.fam_depth(t))
        d1, b1 = R.calc_point_distance(p[19])
        d2, b2 = R.calc_point_distance(p[20])
        assert abs(d1 - d2) <= 4 * (b1 + b2), (d1, d2)
        picked = oracle.extract_features(CS.cloud4(CS.fam_depth(t)), CS.RANGE40)["picked"]
        # the side that receives NEAR_BLOCK flips: :509-511 fills 15 ... 19, :517-518 fills 20 ... 24
        assert (picked[20:25] == -3).all() == after and (picked[15:20] == -3).all() == (not after)
    p = _xyz(CS.fam_depth(hi))
    assert R.calc_point_distance(p[19])[0] <= R.calc_point_distance(p[20])[0] + 4 * 5 * U * 200   # `>`: equal depths take the else branch


def test_curvature_threshold_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["curvature"]
    assert at_lo                                                    # below the threshold: a less-flat point
    thr = R.f32(np.float32(0.02))
    for t in (lo, hi):
        c, bound, _ = R.curvature_at(_xyz(CS.fam_curvature(t)), 20, 5)
        assert bound > 0 and abs(c - thr) <= 4 * bound, (c, thr, bound)


def _fit(p11, backward=True):
    det = []
    R.point_classify(_xyz(p11), 5, 5, detail=det)
    return [d for d in det if "pts" in d][0 if backward else 1]


def test_eigenvalue_gate_100_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["eig100"]
    assert at_lo == R.SURFACE_FLAT and at_hi == R.ONESIDE_FLAT
    for t in (lo, hi):
        D = _fit(CS.fam_eig100(t))["D"]
        assert D[2] > 10000 * D[0]                                  # the other gate is far away
        assert abs(D[2] - 100 * D[1]) <= R.EIG_BAND * D[2] * 101, (D, t)


def test_eigenvalue_gate_10000_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["eig10000"]
    assert at_lo == R.SURFACE_FLAT and at_hi == R.ONESIDE_FLAT
    for t in (lo, hi):
        D = _fit(CS.fam_eig10000(t))["D"]
        assert D[2] > 400 * D[1]                                    # the 100 x gate holds by a factor 4
        assert abs(D[2] - 10000 * D[0]) <= R.EIG_BAND * D[2] * 10001, (D, t)


def test_line_distance_bound_flips_where_float64_says(pairs):
    lo, hi, at_lo, at_hi = pairs["dist"]
    assert at_lo == R.SURFACE_FLAT and at_hi == R.ONESIDE_FLAT
    for t in (lo, hi):
        p = _xyz(CS.fam_dist(t))
        w = p[[5, 4, 3, 2, 1, 0]]
        a = w - w.mean(0)
        lam, V = np.linalg.eigh(a.T @ a / 6)
        assert lam[2] > 150 * lam[1]                                # the 100 x gate holds by a factor 1.5
        dist = np.linalg.norm(np.cross(a, V[:, 2]), axis=1)
        bound = np.linalg.norm(a, axis=1).max() * R.MEASURED_DIR_RAD + 17 * U * np.abs(p).max()
        assert abs(dist.max() - 0.08) <= 4 * bound, (dist.max(), bound)


@pytest.mark.parametrize("name,gate,at_lo,at_hi", [("angle5", 5.0, R.SURFACE_FLAT, R.ONESIDE_FLAT), ("angle45", 45.0, R.ONESIDE_FLAT, R.CORNER_SHARP),
                                                   ("angle135", 135.0, R.CORNER_SHARP, R.ONESIDE_FLAT), ("angle175", 175.0, R.ONESIDE_FLAT, R.SURFACE_FLAT)])
def test_angle_gates_flip_where_float64_say(pairs, name, gate, at_lo, at_hi):
    """the sign of an eigenvector is the solver's choice and the four gates are symmetric under it (cos 175 = -cos 5,
    cos 135 = -cos 45): what can be located is |cos| of the angle between the two lines"""
    lo, hi, verdict_lo, verdict_hi = pairs[name]
    assert verdict_lo == at_lo and verdict_hi == at_hi
    for t in (lo, hi):
        v1, v2 = _fit(CS.fam_angle(t))["v"], _fit(CS.fam_angle(t), backward=False)["v"]
        diff, bound = R.calc_cos_angle_diff(v1, v2)
        assert abs(abs(diff) - abs(np.cos(np.deg2rad(gate)))) <= 2 * R.DIR_BAND + 4 * bound, (diff, gate)
        assert abs(float(t) - gate) < 0.01                          # and the family's own angle agrees


def test_reference_takes_the_oracles_side_of_every_pair(oracle, pairs):
    """the two members of every pair as rings of one extraction each: outside its band the reference decides as the oracle
    does; inside (that is where the pairs sit) it says so"""
    for side in (0, 1):
        for call in CS.threshold_calls(pairs, side):
            ref = R.extract(call.cloud, call.ranges, call.params)
            got = oracle.extract_features(call.cloud, call.ranges, oracle_params(oracle, call.params))
            names = list(CS.MARK_FAMILIES if "marks" in call.name else CS.CLASSIFY_FAMILIES)
            for k, name in enumerate(names):                                        # every rule ring sits inside its rule's band
                assert ref["ambiguous"][k] and any(w[0] in CS.RULE_OF[name] for w in ref["why"][k]), (call.name, name, ref["why"][k])
            assert not ref["ambiguous"][-1]                                         # the control ring does not
            compare_with_ref(got, ref, call, call.name)
