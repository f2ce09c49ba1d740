"""CPU side of the degenerate-solve tests (no GPU): tests/degenerate_ref.py against the C oracle's gn_step, the conditions its
systems and scenes are built to meet, and what a comparison built on it can see.

  conditions   every member of systems() at thresholds 100 and 10, asserted of the float64 side alone: neighbouring
               eigenvalues at least 3 apart, cond(A) <= 2e3 where x is compared, no eigenvalue within 1 % of the threshold, the
               convergence flag at least a thousand units from its threshold, the 32 sign variants of P0 all different and the
               second nearest at least 1e3 units of unit_P farther than the nearest; k = 1, 2, 3, 5 and 6 below 100, smallest
               eigenvalues 5 and 90, largest 3e2 and 1e4, one system whose smallest eigenvalue is 0 to float32
  floors       oracle.gn_step against step64, the largest distance over systems() x thresholds in each unit:
                   matP         1.29 units of unit_P  (k1_small_step; 0.01 .. 0.79 on the others)
                   x            1.75 units of unit_x  (k6_all_below at threshold 10, a plain solve; 1.60 on a projected one)
                   pose         1.52, delta_r 0.33, delta_t 0.37 units
               K_P = 12.91 and K_X = 17.45 are ten times the first two (the project's rule for K, K_S and K_ODOM); both far
               below the 100 units at which the unit itself would be in doubt
  mutations    a matP with the column instead of the row zeroed, the orthogonal projector, a transposed V, one row too many
               and one too few zeroed: each fails the comparison on at least one system (in fact on every system with
               0 < k < 6; the table is printed)
  scenes       on the oracle, one corridor map (892 corner + 1055 surf points) closed at its far end:
                   a  160 + 600 points clear of the end: eigenvalues 0.00, 231, 363, 511, 4954, 7709; degenerate, 7 iterations
                   b  160 + 850 points that reach the end wall: smallest eigenvalue 180; not degenerate, 3 iterations
                   c  a thinned to 80 + 274 points: 0.00, 55, 129, 354, ...: two below 100; degenerate, 4 iterations
                   d  12 + 30 points: 42 rows, fewer than the 50 a solve needs
  sensitivity  every scan coordinate one ulp up: scene a's oracle loop stops after 3 iterations instead of 7 and its pose moves
               by 2.6e-3 m; scene b keeps its 3 iterations and moves by 6.0e-7 m (asserted: a factor of at least 100).  Scene a's
               initial pose is chosen where the third update lands on the convergence threshold -- the sensitivity is that
               test's; from 48 other draws and starts the same corridor moved by 2e-7 .. 7e-7 m, as scene b does
"""
import numpy as np
import pytest

import degenerate_ref as D


@pytest.fixture(scope="module")
def systems():
    return D.systems()


@pytest.fixture(scope="module")
def scenes():
    return D.scenes()


def oracle_step(oracle, sy, eig_thresh, it=0, matP=None, degenerate=False):
    return oracle.gn_step(sy["AtA"], sy["Atb"], it, sy["pose"], np.zeros(36) if matP is None else matP, degenerate,
                          eig_thresh=eig_thresh)


def test_systems_meet_their_conditions(systems):
    ks, lo, hi = set(), set(), set()
    for sy in systems:
        for th in D.THRESHOLDS:
            s = D.assert_conditions(sy, th)
            if th == 100.0:
                ks.add(s["k"])
                lo.add(float(sy["lam"][0]))
                hi.add(float(sy["lam"][-1]))
                assert s["k"] == int((sy["lam"] < th).sum())
    assert {1, 2, 3, 5, 6} <= ks
    assert {5.0, 90.0, 0.0} <= lo and {3.0e2, 1.0e4} <= hi
    assert sum(1 for sy in systems if not sy["check_x"]) == 1


def test_floors(oracle, systems):
    """The oracle inside K_P / K_X of step64 on every system, and the constants ten times what it shows."""
    worst = dict(P=0.0, x=0.0, pose=0.0, delta_r=0.0, delta_t=0.0)
    for sy in systems:
        for th in D.THRESHOLDS:
            g = oracle_step(oracle, sy, th)
            s = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], g["matP"], False, th)
            d = D.compare(g, s, check_x=sy["check_x"])
            print("%-16s thresh %5.0f  k %d  " % (sy["name"], th, s["k"]) + "  ".join("%s %.3f" % (k, d[k]) for k in worst))
            assert d["ok"], (sy["name"], th, d)
            for k in worst:
                if not np.isnan(d[k]):
                    worst[k] = max(worst[k], d[k])
    print("largest: " + "  ".join("%s %.3f" % kv for kv in worst.items()) + "  (K_P %.2f, K_X %.2f)" % (D.K_P, D.K_X))
    assert 10.0 * worst["P"] <= D.K_P * 1.001 and D.K_P <= 10.1 * worst["P"]
    assert 10.0 * worst["x"] <= D.K_X * 1.001 and D.K_X <= 10.1 * worst["x"]
    assert max(worst["pose"], worst["delta_r"], worst["delta_t"]) <= worst["x"]
    assert D.K_P <= 100.0 and D.K_X <= 100.0


def test_singular_system_decision_and_projector(oracle, systems):
    """Smallest eigenvalue 0 to float32 (what an open corridor gives): the decision and matP have a float64 statement; x has
    none -- the pivoted QR's rank decision is the reference's -- and is compared on the device with the oracle alone."""
    sy = [s for s in systems if not s["check_x"]][0]
    for th in D.THRESHOLDS:
        g = oracle_step(oracle, sy, th)
        s = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], g["matP"], False, th)
        d = D.compare(g, s, check_x=False)
        assert s["k"] == 1 and g["degenerate"] and d["ok"], d
        assert np.isfinite(g["x"]).all()


def mutants(s):
    """Wrong matPs for step64's dict s, in its own float64: name -> (6, 6)."""
    V, k = s["V"], s["k"]
    D0 = np.diag([0.0] * k + [1.0] * (6 - k))
    out = {"column_zeroed": V.T @ (V @ D0),                 # matV2's columns instead of its rows
           "orthogonal_projector": V[:, k:] @ V[:, k:].T,
           "transposed_V": V @ D0 @ V.T}                     # eigenvectors taken as the rows of matV
    if k < 6:
        out["one_row_more"] = D.projector(V, k + 1)
    if k > 0:
        out["one_row_fewer"] = D.projector(V, k - 1)
    return out


def test_every_mutation_is_seen(systems):
    """Each mutant, rounded to float32 and put in the implementation's place, fails compare() on at least one system."""
    seen = {}
    for sy in systems:
        s0 = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], None, False, 100.0)
        if not 0 < s0["k"] < 6:
            continue
        for name, P in mutants(s0).items():
            x = P @ s0["x_qr"]
            dR, dT = D.deltas(x)
            got = dict(degenerate=True, matP=P.astype(np.float32), x=x.astype(np.float32),
                       pose=(sy["pose"].astype(np.float64) + x).astype(np.float32), delta_r=dR, delta_t=dT,
                       converged=bool(dR < 0.05 and dT < 0.05))
            s = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], got["matP"], False, 100.0)
            d = D.compare(got, s, check_x=sy["check_x"])
            seen.setdefault(name, []).append((sy["name"], d["ok"], d["P"]))
            print("%-22s %-16s ok %-5s matP %.3g units" % (name, sy["name"], d["ok"], d["P"]))
    assert set(seen) == {"column_zeroed", "orthogonal_projector", "transposed_V", "one_row_more", "one_row_fewer"}
    for name, rows in seen.items():
        assert any(not ok for _, ok, _ in rows), name
    # and the unmutated statement passes the same comparison
    for sy in systems:
        s0 = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], None, False, 100.0)
        got = dict(degenerate=s0["degenerate"], matP=s0["P0"].astype(np.float32), x=s0["x"].astype(np.float32),
                   pose=s0["pose"].astype(np.float32), delta_r=s0["delta_r"], delta_t=s0["delta_t"], converged=s0["converged"])
        s = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], got["matP"], False, 100.0)
        assert D.compare(got, s, check_x=sy["check_x"])["ok"], sy["name"]


def test_carried_state_is_used_as_given(oracle, systems):
    """Iterations above 0: matP and the flag are not recomputed, and the update is matP x of the plain solve."""
    rng = np.random.default_rng(3)
    sy = systems[0]
    dense = rng.uniform(-1.0, 1.0, (6, 6)).astype(np.float32)
    for it in (1, 4, 9):
        plain = oracle_step(oracle, sy, 100.0, it, dense, False)
        assert not plain["degenerate"] and np.array_equal(plain["matP"], dense)
        g = oracle_step(oracle, sy, 100.0, it, dense, True)
        assert g["degenerate"] and np.array_equal(g["matP"], dense)
        want, bound = D.dot6_bound(dense, plain["x"])
        assert (np.abs(g["x"] - want) <= bound).all()
        assert np.array_equal(g["pose"], sy["pose"] + g["x"])
        s = D.step64(sy["AtA"], sy["Atb"], it, sy["pose"], dense, True)
        ux = D.unit_x(s["A"], s["x_qr"]) * np.abs(dense).sum(axis=1).max()
        assert np.abs(g["x"] - s["x"]).max() <= D.K_X * ux


def scene_system(oracle, scenes, k):
    mc, ms = scenes["map"]
    s = scenes["scans"][k]
    sw = oracle.sweep(oracle.kdtree(mc), oracle.kdtree(ms), s["corner"], s["surf"], s["init_pose"])
    AtA, Atb = D.tap_system(sw["sums"])
    return np.linalg.eigvalsh(AtA.astype(np.float64)), int(sw["sums"][27])


def test_scenes_are_what_they_claim(oracle, scenes):
    mc, ms = scenes["map"]
    assert max(len(mc), len(ms)) <= 2100
    got = []
    for k, s in enumerate(scenes["scans"]):
        assert np.abs(s["init_pose"][3:] - s["gt_pose"][3:]).max() <= 0.05 and np.abs(s["init_pose"][:3] - s["gt_pose"][:3]).max() <= 0.006
        E, rows = scene_system(oracle, scenes, k)
        ok, pose, st = oracle.scanmatch_scan(mc, ms, s["corner"], s["surf"], s["init_pose"])
        print("%-12s %4d + %4d points, rows %4d, eigenvalues %s, iterations %d, degenerate %d, converged %d" % (
            s["name"], len(s["corner"]), len(s["surf"]), rows, np.round(E, 2).tolist(), st.iterations, st.degenerate, st.converged))
        got.append(st.degenerate)
        if k == 0:
            assert st.degenerate == 1 and int((E < 100.0).sum()) == 1 and E[0] < 1e-3 * E[1] and st.iterations >= 1
        elif k == 1:
            assert st.degenerate == 0 and E[0] >= 110.0 and st.converged == 1
        elif k == 2:
            assert st.degenerate == 1 and int((E < 100.0).sum()) == 2 and E[1] <= 90.0 and E[2] >= 110.0
            assert np.diff(E).min() >= D.MIN_GAP
        else:
            assert rows < 50 and st.n_rows == rows and st.iterations == 0 and not ok and st.degenerate == 0
            assert np.array_equal(pose, s["init_pose"])
        if k < 3:
            assert rows >= 300
    assert got == D.EXPECT_DEGENERATE


def one_ulp_up(cloud):
    out = cloud.copy()
    out[:, :3] = np.nextafter(cloud[:, :3], np.float32(np.inf))
    return out


def test_one_ulp_moves_the_degenerate_loop_not_the_constrained_one(oracle, scenes):
    """Why the device's degenerate loops are held to the device's own taps and not to the oracle's pose: every scan
    coordinate one ulp up changes the oracle's iteration count on scene a (7 against 3) and its pose by 2.6e-3 m; on scene b
    the count stays and the pose moves by 6.0e-7 m.  The device's sums differ from the oracle's by more than an ulp of the
    input (MFMA order against sequential order), so which of the two loops it runs on scene a is not the oracle's to say.
    (The sensitivity is the convergence test's: scene a starts where the third update lands on the threshold.  From 48 other
    draws and starts of the same corridor the perturbation moved the pose by 2e-7 .. 7e-7 m, like scene b.)"""
    mc, ms = scenes["map"]
    moved, its = [], []
    for s in scenes["scans"][:2]:
        _, p0, st0 = oracle.scanmatch_scan(mc, ms, s["corner"], s["surf"], s["init_pose"])
        _, p1, st1 = oracle.scanmatch_scan(mc, ms, one_ulp_up(s["corner"]), one_ulp_up(s["surf"]), s["init_pose"])
        moved.append(float(np.abs(p1.astype(np.float64) - p0).max()))
        its.append((st0.iterations, st1.iterations))
    print("one ulp: scene a iterations %s, pose moved %.3g; scene b iterations %s, pose moved %.3g" % (its[0], moved[0], its[1], moved[1]))
    assert its[1][0] == its[1][1]
    assert moved[0] >= 100.0 * moved[1] and moved[0] > 1e-4
