"""The degenerate branch of the shared solve step on the device (-m gpu): gn_step_block of csrc/lslam_solve_dev.hpp -- the
projector of quirk Q2 at iteration 0, its storage in GNState::matP, its reload at every later iteration -- through the tap
lslam_gn_step, the production loops and batches, and variant C.  The float64 statement, its units, K_P and K_X are
tests/degenerate_ref.py's; the CPU side of every bar is tests/test_degenerate_ref.py.

  tap, iteration 0   every member of degenerate_ref.systems(), as it is and scaled by ten (the tap's threshold is 100: the scaled
                     system is the threshold-10 case): the decision equals step64's and the oracle's; matP within K_P units of
                     the nearest of the 32 sign variants, the one the oracle's matP is nearest to as well; x, pose, delta_r and
                     delta_t within K_X units of step64; converged equal; pose = pose_in + x in float32 exactly.  The singular
                     system: decision and matP as above; the plain solve's bits are the oracle's and x is matP times them
  tap, iterations    1, 4 and 9 with a matP handed in (iteration 0's, and a random dense one): matP and the flag come back bit
                     for bit; x within 6 * 2^-24 * sum |P[r, k] x_qr[k]| per component of the float64 product with the plain
                     solve's bits (a six-term float32 dot product, fused or not: derived); pose = pose_in + x exactly; with the
                     flag handed in clear a system that would be degenerate is not projected
  loops              scenes a, b, c of degenerate_ref.scenes(), LANE search, both jtj_modes, the convergence thresholds as they
                     are and at zero (all ten iterations run): lslam_scanmatch_scan with max_iterations = n, n = 1 .. 10, against
                     ONE iteration done by hand -- sweep tap -> lslam_gn_step at iteration n - 1 -- from the pose the loop
                     returned for n - 1, with iteration 0's matP and flag handed in.
                     FORM: per iteration, bit for bit -- pose, converged, n_rows, delta_r, delta_t; iterations and degenerate
                     always.  Why bits: the production launch under a forced LANE mode with knn_cert = 0 takes the tap's
                     instantiation (launch_sweep: the same sweep_kernel<256, ., false, depth> by stack mode, no certificate
                     pass) over the same block layout; its bounded search rejects beyond the gate exactly what the gate
                     rejects; both reduce with reduce_partials and hand the solve the same (float) rounding of the float64
                     totals (sweep_ex_impl, solve_finish).  Why per iteration and not one chain from the initial pose: the
                     tap makes a sweep's rotation on the host with std::sin / std::cos(float), the loop on the device as
                     (float)sin((double)a); libm's float functions are not correctly rounded, and at about one pose in twenty one
                     of the twelve values is an ulp off the device's.  The first run of the one-chain form found it (scene b,
                     second iteration: sinf(0.5 * 0.450136) = 0.22317241 on the host, 0.22317240 on the device; the same
                     with LSLAM_UNBOUNDED_KNN, so not the search).  The tap cannot be handed the loop's rotation, so such an
                     iteration is not compared (tap_can_make_the_loops_rotation says which, from the pose alone) and the
                     next one starts from the loop's own pose again; no tolerance anywhere.  At most a third of a loop's
                     iterations may go uncompared
  batches            the four scenes' scans in two orders, scans_in_flight 0, 1 and 2, LANE and GRID: every scan's pose, status,
                     iterations and n_rows equal its single run's bit for bit and stats.degenerate is [1, 0, 1, 0] in scene order;
                     the same with scene a twice at two initial poses (two matPs side by side); knn_cert = 2 once
  variant C          FeatureMap.scan_match_scan over 20 m cubes on scene a: degenerate, and the same pose bits from a second call
                     and from the call after cubemap_invalidate()

Each test prints the largest distances it saw before asserting.  Measured on an MI355X when this file was written:
  tap, iteration 0   matP 1.29 units of unit_P (K_P = 12.91), x 1.60, pose 1.33, delta_r 0.33, delta_t 0.69 units of unit_x
                     (K_X = 17.45) over the 18 systems -- on the committed nine the oracle's own figures to the digit; the
                     member nearest to the device's matP is the oracle's on every system
  tap, iterations    |x - matP x_qr| at most 0.26 of the dot-product bound
  loops              76 iterations over the twelve runs; 72 held bit for bit, 4 not comparable (scene b, iterations 2 and 6);
                     scene a runs 7 iterations, b 3, c 4 with the thresholds as they are.  The scenes' own matP lies 0.07 - 0.08
                     units from the nearest member
  batches, variant C every comparison bit for bit; variant C runs 7 iterations on 760 rows, degenerate
No defect was found in the branch; the one finding is the rotation's sine and cosine above.

Not covered: systems whose sub-threshold eigenvalues coincide (the null-space basis, and with it the quirk's matP, is then not
determined by the matrix); NaN sums; the sharded and joint-stereo loops; an iteration whose rotation the tap cannot make.
"""
import ctypes as C
import math

import numpy as np
import pytest

import degenerate_ref as D

pytestmark = pytest.mark.gpu

LANE, GRID = D.LANE, D.GRID
STACK_DEEP = 0x100


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def systems():
    """systems() and each member scaled by ten; the scaled ones meet the conditions at the tap's threshold as the originals
    do at threshold 10 (asserted)."""
    out = []
    for sy in D.systems():
        D.assert_conditions(sy, 100.0)
        out.append(sy)
        t = dict(sy, name=sy["name"] + "_x10", AtA=(sy["AtA"].astype(np.float64) * 10.0).astype(np.float32),
                 Atb=(sy["Atb"].astype(np.float64) * 10.0).astype(np.float32), lam=sy["lam"] * 10.0)
        D.assert_conditions(t, 100.0)
        out.append(t)
    return out


@pytest.fixture(scope="module")
def scenes():
    return D.scenes()


def test_tap_iteration0_against_step64_and_the_oracle(ctx, oracle, systems):
    worst = dict(P=0.0, x=0.0, pose=0.0, delta_r=0.0, delta_t=0.0)
    n_deg = 0
    for sy in systems:
        zero = np.zeros(36, np.float32)
        g = ctx.gn_step(sy["AtA"], sy["Atb"], 0, sy["pose"], zero, False)
        o = oracle.gn_step(sy["AtA"], sy["Atb"], 0, sy["pose"], zero, False, eig_thresh=100.0)
        s = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], g["matP"], False, 100.0)
        d = D.compare(g, s, check_x=sy["check_x"])
        print("%-22s k %d  " % (sy["name"], s["k"]) + "  ".join("%s %.3f" % (k, d[k]) for k in worst))
        for k in worst:
            if not np.isnan(d[k]):
                worst[k] = max(worst[k], d[k])
        assert bool(g["degenerate"]) == s["degenerate"] == bool(o["degenerate"]), sy["name"]
        assert d["ok"], (sy["name"], d)
        assert np.array_equal(bits(g["pose"]), bits(sy["pose"] + g["x"])), sy["name"]
        if s["degenerate"]:
            n_deg += 1
            so = D.step64(sy["AtA"], sy["Atb"], 0, sy["pose"], o["matP"], False, 100.0)
            assert so["member"] == s["member"] or s["k"] == 6, (sy["name"], so["member"], s["member"])
        else:  # the pinned branch: the oracle's bits
            assert np.array_equal(bits(g["x"]), bits(o["x"])), sy["name"]
        assert g["converged"] == o["converged"], sy["name"]
        if not sy["check_x"]:  # singular: the plain solve is the oracle's, bit for bit, and x is matP times it
            plain = ctx.gn_step(sy["AtA"], sy["Atb"], 1, sy["pose"], zero, False)
            oplain = oracle.gn_step(sy["AtA"], sy["Atb"], 1, sy["pose"], zero, False, eig_thresh=100.0)
            assert np.array_equal(bits(plain["x"]), bits(oplain["x"])), (sy["name"], plain["x"], oplain["x"])
            want, bound = D.dot6_bound(g["matP"], plain["x"])
            assert (np.abs(g["x"] - want) <= bound).all(), (sy["name"], g["x"], want, bound)
            # ... which holds it to the oracle's x through the two matPs' distance
            owant, obound = D.dot6_bound(o["matP"], oplain["x"])
            slack = np.abs(g["matP"].astype(np.float64) - o["matP"]) @ np.abs(plain["x"].astype(np.float64))
            assert (np.abs(g["x"].astype(np.float64) - o["x"]) <= bound + obound + slack).all(), sy["name"]
    print("largest: " + "  ".join("%s %.3f" % kv for kv in worst.items()) + "  (K_P %.2f, K_X %.2f)" % (D.K_P, D.K_X))
    assert n_deg >= 12 and n_deg < len(systems)


@pytest.mark.parametrize("it", [1, 4, 9])
def test_tap_later_iterations_use_the_state_handed_in(ctx, oracle, systems, it):
    rng = np.random.default_rng(17 + it)
    dense = rng.uniform(-1.0, 1.0, (6, 6)).astype(np.float32)
    worst = 0.0
    for sy in systems[::2]:
        first = ctx.gn_step(sy["AtA"], sy["Atb"], 0, sy["pose"], np.zeros(36, np.float32), False)
        assert first["degenerate"]
        for P in (first["matP"], dense):
            plain = ctx.gn_step(sy["AtA"], sy["Atb"], it, sy["pose"], P, False)
            oplain = oracle.gn_step(sy["AtA"], sy["Atb"], it, sy["pose"], P, False, eig_thresh=100.0)
            # handed in clear: not projected, nothing recomputed
            assert not plain["degenerate"] and np.array_equal(bits(plain["matP"]), bits(P)), sy["name"]
            assert np.array_equal(bits(plain["x"]), bits(oplain["x"])), sy["name"]
            assert np.array_equal(bits(plain["pose"]), bits(sy["pose"] + plain["x"]))
            g = ctx.gn_step(sy["AtA"], sy["Atb"], it, sy["pose"], P, True)
            assert g["degenerate"] and np.array_equal(bits(g["matP"]), bits(P)), sy["name"]
            want, bound = D.dot6_bound(P, plain["x"])
            err = np.abs(g["x"].astype(np.float64) - want)
            if (bound > 0).any():
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            assert (err <= bound).all(), (sy["name"], g["x"], want, bound)
            assert np.array_equal(bits(g["pose"]), bits(sy["pose"] + g["x"])), sy["name"]
            dR, dT = D.deltas(g["x"])
            assert abs(g["delta_r"] - dR) <= 4 * D.EPS32 * dR and abs(g["delta_t"] - dT) <= 4 * D.EPS32 * dT
            assert g["converged"] == bool(np.float32(g["delta_r"]) < np.float32(0.05) and np.float32(g["delta_t"]) < np.float32(0.05))
    print("iteration %d: largest |x - P x_qr| / bound %.3f" % (it, worst))


# ---- loops ------------------------------------------------------------------------------------------------------------------
def run_opts(ctx, jtj_mode, search, never_converge=False, **kw):
    opts = ctx.default_opts()
    opts.jtj_mode = jtj_mode
    opts.search_mode = search
    if never_converge:
        opts.delta_r_abort = opts.delta_t_abort = 0.0
    for k, v in kw.items():
        setattr(opts, k, v)
    return opts


def tap_step(ctx, pose, it, P, degenerate, opts):
    """One iteration by hand on the resident scan: sweep tap -> solve tap with the state handed in.  None: too few rows."""
    sw = ctx.sweep(pose, jtj_mode=opts.jtj_mode, taps=False, search_mode=opts.search_mode)["sums"]
    rows = int(sw[27])
    if rows < 50:
        return None
    AtA, Atb = D.tap_system(sw)
    g = ctx.gn_step(AtA, Atb, it, pose, P, degenerate, dr=opts.delta_r_abort, dt=opts.delta_t_abort)
    return dict(g, rows=rows, AtA=AtA, Atb=Atb)


_LIBM = C.CDLL("libm.so.6")
_LIBM.sinf.restype = _LIBM.cosf.restype = C.c_float
_LIBM.sinf.argtypes = _LIBM.cosf.argtypes = [C.c_float]


def tap_can_make_the_loops_rotation(pose):
    """The twelve sines and cosines a sweep's rotation is made of (pose_to_Rt_sc: half and full angles): the tap makes them on
    the host with std::sin / std::cos(float), the loop on the device as (float)sin((double)a) at the end of the previous
    solve.  libm's float functions are good to 0.56 ulp, not correctly rounded: a few values in a thousand are the other
    neighbour of the exact one, and the two sweeps then run with rotations an ulp apart.  -> whether all twelve agree."""
    for a in np.asarray(pose, np.float32)[:3]:
        for v in (np.float32(0.5) * a, a):
            if np.float32(_LIBM.sinf(float(v))) != np.float32(math.sin(float(v))) or np.float32(_LIBM.cosf(float(v))) != np.float32(math.cos(float(v))):
                return False
    return True


@pytest.mark.parametrize("never_converge", [False, True])
@pytest.mark.parametrize("jtj_mode", [0, 1])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_loop_equals_the_chain_done_by_hand(ctx, scenes, k, jtj_mode, never_converge):
    scan = scenes["scans"][k]
    ctx.map_set(*scenes["map"])
    opts = run_opts(ctx, jtj_mode, LANE | STACK_DEEP, never_converge, knn_cert=0)
    ctx.scan_set(scan["corner"], scan["surf"])
    first = tap_step(ctx, scan["init_pose"], 0, np.zeros(36, np.float32), False, opts)
    assert first is not None and bool(first["degenerate"]) == bool(D.EXPECT_DEGENERATE[k])
    P, degenerate = first["matP"].copy(), first["degenerate"]
    if degenerate:  # the loop's matP is the references': the corridor's own system
        s = D.step64(first["AtA"], first["Atb"], 0, scan["init_pose"], P, False, 100.0)
        d = D.compare(first, s, check_x=False)
        print("%s: eigenvalues %s, matP %.3f units from the nearest member" % (scan["name"], np.round(s["E"], 2).tolist(), d["P"]))
        assert s["k"] == (1 if k == 0 else 2) and d["ok"], d
    want, prev, checked, skipped, ran = first, scan["init_pose"], 0, [], 0
    for n in range(1, 11):
        opts.max_iterations = n
        status, pose, st = ctx.scanmatch_scan(scan["corner"], scan["surf"], scan["init_pose"], opts)
        label = (scan["name"], jtj_mode, never_converge, n)
        assert st.iterations == n and bool(st.degenerate) == bool(degenerate), label
        ran = n
        if n == 1 or tap_can_make_the_loops_rotation(prev):
            assert np.array_equal(bits(pose), bits(want["pose"])), (label, pose, want["pose"])
            assert bool(st.converged) == bool(want["converged"]) and st.n_rows == want["rows"], label
            assert np.array_equal(bits([st.delta_r, st.delta_t]), bits([want["delta_r"], want["delta_t"]])), label
            assert np.array_equal(bits(want["matP"]), bits(P)) and bool(want["degenerate"]) == bool(degenerate), label
            checked += 1
        else:
            skipped.append(n)
        if st.converged:  # the loop is over: a larger limit changes nothing
            opts.max_iterations = n + 1
            _, again, st2 = ctx.scanmatch_scan(scan["corner"], scan["surf"], scan["init_pose"], opts)
            assert np.array_equal(bits(again), bits(pose)) and st2.iterations == n and st2.converged == 1, label
            break
        prev = pose
        if n < 10:
            want = tap_step(ctx, prev, n, P, degenerate, opts)
            assert want is not None, label
    print("%s jtj_mode %d: %d iterations%s, %d held bit for bit, %s not (the tap cannot make the rotation the loop ran with)" % (
        scan["name"], jtj_mode, ran, ", converged" if st.converged else "", checked, skipped or "none"))
    if never_converge:
        assert ran == 10 and not st.converged
    assert checked >= 2 and len(skipped) <= max(1, ran // 3), (checked, skipped)


# ---- batches ----------------------------------------------------------------------------------------------------------------
def single_runs(ctx, scans, inits, opts):
    return [ctx.scanmatch_scan(s["corner"], s["surf"], p0, opts) for s, p0 in zip(scans, inits)]


def assert_batch_equals_singles(ctx, scans, inits, opts, single, label):
    ctx.scan_set_batch([(s["corner"], s["surf"]) for s in scans])
    _, poses, stats = ctx.run_batch(np.stack(inits), opts)
    for j, (status, pose, st) in enumerate(single):
        assert np.array_equal(bits(poses[j]), bits(pose)), (label, j, poses[j], pose)
        assert (stats[j].status, stats[j].iterations, stats[j].n_rows, stats[j].degenerate, stats[j].converged) == (
            st.status, st.iterations, st.n_rows, st.degenerate, st.converged), (label, j)
    return stats


@pytest.mark.parametrize("search", [LANE, GRID])
@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0)])
def test_batch_keeps_the_projector_per_scan(ctx, scenes, order, search):
    ctx.map_set(*scenes["map"])
    scans = [scenes["scans"][k] for k in order]
    inits = [s["init_pose"] for s in scans]
    single = single_runs(ctx, scans, inits, run_opts(ctx, 1, search))
    assert [st.degenerate for _, _, st in single] == [D.EXPECT_DEGENERATE[k] for k in order]
    assert single[order.index(3)][2].status == D.TOO_FEW_MATCHES
    assert len({st.iterations for _, _, st in single}) >= 3  # the scans stop at different iterations: finished ones are compacted away
    for in_flight in (0, 1, 2):
        stats = assert_batch_equals_singles(ctx, scans, inits, run_opts(ctx, 1, search, scans_in_flight=in_flight), single,
                                            (order, search, in_flight))
        assert [st.degenerate for st in stats] == [D.EXPECT_DEGENERATE[k] for k in order]
    if search == LANE and order[0] == 0:
        opts = run_opts(ctx, 1, search, knn_cert=2)
        assert_batch_equals_singles(ctx, scans, inits, opts, single_runs(ctx, scans, inits, opts), (order, search, "knn_cert 2"))


@pytest.mark.parametrize("search", [LANE, GRID])
def test_batch_with_two_projectors_side_by_side(ctx, scenes, search):
    """Scene a twice, from two initial poses: two different matPs in one batch, next to a scan that has none."""
    ctx.map_set(*scenes["map"])
    a, b, c, d = scenes["scans"]
    scans = [a, b, a, c, d]
    other = (a["gt_pose"] - (a["init_pose"] - a["gt_pose"])).astype(np.float32)
    inits = [a["init_pose"], b["init_pose"], other, c["init_pose"], d["init_pose"]]
    opts = run_opts(ctx, 1, search)
    # the two starts give two different projectors (the chain's first step says which)
    ctx.scan_set(a["corner"], a["surf"])
    P = [tap_step(ctx, p0, 0, np.zeros(36, np.float32), False, run_opts(ctx, 1, LANE | STACK_DEEP, knn_cert=0))["matP"] for p0 in (inits[0], inits[2])]
    assert not np.array_equal(bits(P[0]), bits(P[1]))
    single = single_runs(ctx, scans, inits, opts)
    assert not np.array_equal(bits(single[0][1]), bits(single[2][1]))
    for in_flight in (0, 1, 2):
        stats = assert_batch_equals_singles(ctx, scans, inits, run_opts(ctx, 1, search, scans_in_flight=in_flight), single, (search, in_flight))
        assert [st.degenerate for st in stats] == [1, 0, 1, 1, 0]


# ---- variant C --------------------------------------------------------------------------------------------------------------
def test_variant_c_on_the_open_corridor(pkg, ctx, scenes):
    a = scenes["scans"][0]
    fm = pkg.FeatureMap(ctx, 21, 11, 21)
    try:
        fm.setup_world_cube_size(20.0)
        fm.setup_lidar_valid_distance(60.0)
        fm.setup_filter_size(0.2, 0.4, 0.05)  # a map leaf below the map's point spacing: the clouds stay as they are
        fm.update(np.zeros(3, np.float32))
        fm.add_feature_cloud(scenes["map"][0], scenes["map"][1], np.eye(4, dtype=np.float32))
        nc, ns = fm.surround_counts()
        assert nc >= 400 and ns >= 600
        status, pose, st = fm.scan_match_scan(a["corner"], a["surf"], a["init_pose"])
        print("variant C: %d + %d map points, iterations %d, rows %d, degenerate %d, converged %d" % (nc, ns, st.iterations, st.n_rows,
                                                                                                  st.degenerate, st.converged))
        assert st.degenerate == 1 and st.iterations >= 2 and st.n_rows >= 300
        assert not np.array_equal(bits(pose), bits(a["init_pose"]))
        _, pose2, st2 = fm.scan_match_scan(a["corner"], a["surf"], a["init_pose"])
        assert np.array_equal(bits(pose2), bits(pose)) and (st2.iterations, st2.n_rows, st2.degenerate) == (st.iterations, st.n_rows, 1)
        fm.cubemap_invalidate()
        _, pose3, st3 = fm.scan_match_scan(a["corner"], a["surf"], a["init_pose"])
        assert fm.cubemap_stats()[1] == 0  # every tree was built again
        assert np.array_equal(bits(pose3), bits(pose)) and (st3.iterations, st3.n_rows, st3.degenerate) == (st.iterations, st.n_rows, 1)
    finally:
        fm.close()
