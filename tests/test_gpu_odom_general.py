"""Scan-to-scan odometry (variant B, csrc/lslam_odom.hip and odom_sweep_kernel of csrc/lslam_kernels.hip) held step by step to
references that share no code with it -- tests/odom_ref.py, and the C oracle's per-point functions -- through the one-step
parity tap lslam_debug_odom_step, on the input families of odom_ref.families (what each is for is said there; the CPU side of
every bar is tests/test_odom_ref.py).  At the end the node the bench times, DeviceLaserOdometry.process, against the oracle sweep
by sweep.

Per step of a family (launch loop, path 0):
  correspondences  ind index for index and the tie flag exactly against corr_ref at the DEVICE's sel; the inputs tie at no
                   query's nearest point (asserted on the reference side), so nothing is left out
  sel              inside SEL_UNITS of to_start64.  The tap's sel is the residual pass's; the search kernel computes its own
                   from the same state -- were the two different, the indices (found from the search's) would not be
                   corr_ref's at the tap's
  coefficients     bit for bit, with the kept flags, against oracle_odom_coeff at the device's sel and indices; and inside
                   4 x the family's conditioning (odom_ref.COEFF_COND) of coeff64
  sums             each of the 27 within K_ODOM = 34 units of sums64_odom built from the device's taps; the three counters exact
  solve            pose and x after the step bit for bit oracle.gn_step's on the device's sums rounded to float32 (the solve
                   consumes the float64 totals through exactly that rounding: solve_finish's (float)tot[k]); on a step the
                   eigenvalue test (threshold 10) calls degenerate -- the first step of seven families, DEGENERATE_AT_0 -- x
                   and the pose within K_X units of the plain solve's error (tests/degenerate_ref.py) and converged equal
and, where the persistent kernel can be held to one generation (iter 4, 9, 24; at most 64 blocks), path 1's indices, sums and
state bit for bit path 0's.

Measured on an MI355X, largest over the 26 families and their iterations (each test prints its own): no index and no tie flag
differs; sel 3.21 units (bound 29); coefficients and kept flags equal the oracle's bits everywhere, and lie within the
family's recorded conditioning of coeff64 (bar: 4 x that); sums 3.15 units (the single flat row of ragged_0_1; 0.2 - 1.8
on the families with sums of many rows; K_ODOM = 34); pose and x equal oracle.gn_step's bits on every non-degenerate step,
and differ from them by 0 on the seven degenerate first steps as well (bar: K_X = 17.45 units).
The ring-table fallback ran on 100 % of the sparse family's queries, the coarse level on 51 % of the large pose's and on all
of the 10 km family's; at 50 km no query saw a grid candidate.  Loop level, 16 and 64 rings x 1800: two sweeps converge (1 and
6 iterations) and four run to 25 iterations per ring count; counts equal, |dt| <= 4.8e-7 m and |dr| <= 1.4e-8 rad on every
sweep, whole loops included; the first five iterations of the eight loops that run to the limit: counts equal,
|dt| <= 4.9e-7 m, |dr| <= 1.4e-8 rad; no tree fallback.
"""
import os

import numpy as np
import pytest

import degenerate_ref as D
import odom_ref as O
import scanmatch_ref as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fams(synth, small_problem):
    return {f["name"]: f for f in O.families(synth, small_problem["world"])}


FAMILY_NAMES = ["ragged_%d_%d" % c for c in O.RAGGED] + [
    "q5_few_sharp", "q5_more_sharp_than_cloud", "guard_edge", "pose_zero", "pose_drive", "pose_large", "reltime_0", "reltime_0999",
    "rings_64", "empty_rings", "rings_0_to_255", "not_ring_order", "rings_above_255", "sparse_2_to_4.9m", "walk_ties", "far_3km",
    "far_10km", "far_50km"]


# families whose first step has an eigenvalue below 10 (tests/odom_ref.py's references say so without a device: few or thin
# clouds, the lattice of walk_ties, and the far families, whose float32 sums are singular) -- where check_step holds the
# projected step
DEGENERATE_AT_0 = {"q5_few_sharp", "guard_edge", "not_ring_order", "walk_ties", "far_3km", "far_10km", "far_50km"}
DEGENERATE_STEPS = {}


class Node:
    """A device node that holds the family's last clouds (its first sweep, taken as they are) and a feature set with the
    family's queries; made with the search profile on."""

    def __init__(self, pkg, ctx, f):
        sr = pkg.scan_registration
        old = os.environ.get("LSLAM_ODOM_SEARCH_TAP")
        os.environ["LSLAM_ODOM_SEARCH_TAP"] = "1"
        try:
            self.dev = pkg.DeviceLaserOdometry(ctx, publish=False)
        finally:
            if old is None:
                del os.environ["LSLAM_ODOM_SEARCH_TAP"]
            else:
                os.environ["LSLAM_ODOM_SEARCH_TAP"] = old
        self.fs = sr.FeatureSet(ctx)
        self.fs.upload(f["sharp"][:0], f["lc"], f["flat"][:0], f["ls"])
        assert self.dev.process(self.fs) is None
        self.fs.upload(f["sharp"], f["lc"], f["flat"], f["ls"])

    def close(self):
        self.dev.close()
        self.fs.close()


def check_step(oracle, f, it, st, label):
    """Everything a path-0 step returns against the references.  -> the largest distances, for the caller to print."""
    ns, nf = len(f["sharp"]), len(f["flat"])
    q = np.concatenate([f["sharp"], f["flat"]])
    sel, ind, coeff, kept = st["sel"], st["ind"], st["coeff"], st["kept"]
    assert st["refreshed"]
    # correspondences
    ref, tie = O.corr_ref(f["lc"], f["ls"], sel[:ns], sel[ns:], ns, nf)
    assert tie.mean() <= O.TIE_SHARE, (label, tie.mean())
    if not f["name"].startswith("far_"):
        assert not tie.any(), label
    assert st["tie"] == bool(tie.any()), (label, st["tie"], int(tie.sum()))
    bad = (ind != ref).any(axis=0) & ~tie
    assert not bad.any(), (label, "queries", np.flatnonzero(bad)[:8].tolist(), "device", ind[:, bad][:, :8].tolist(), "reference",
                           ref[:, bad][:, :8].tolist())
    # sel
    s64, mag = O.to_start64(f["pose"], q)
    su = O.sel_units(sel, s64, mag).max()
    assert su <= O.SEL_UNITS, (label, su)
    # coefficients and kept flags: the oracle's bits, and the geometry's values
    cs, ks = oracle.odom_coeff(f["lc"], sel[:ns], ind[:, :ns], False, it)
    cf, kf = oracle.odom_coeff(f["ls"], sel[ns:], ind[:, ns:], True, it)
    co, ko = np.concatenate([cs, cf]), np.concatenate([ks, kf])
    assert np.array_equal(kept, ko), (label, np.flatnonzero(kept != ko)[:8].tolist())
    neq = (bits(coeff) != bits(co)).any(axis=1)
    assert not neq.any(), (label, "queries", np.flatnonzero(neq)[:8].tolist(), coeff[neq][:4].tolist(), co[neq][:4].tolist())
    c64, k64, d, have = O.coeff64_step(f["lc"], f["ls"], sel, ind, ns, it)
    ok = have & (d > 0)
    cd = O.coeff_distance(coeff[ok], c64[ok], d[ok], sel[ok]).max() if ok.any() else 0.0
    assert cd <= O.COEFF_BAR_FACTOR * O.COEFF_COND[f["name"]], (label, cd, O.COEFF_COND[f["name"]])
    if f["name"] != "walk_ties":
        assert np.array_equal(kept, k64), label
    # sums
    sums = st["sums"]
    n_rows, n_line, n_plane = int(kept.sum()), int(kept[:ns].sum()), int(kept[ns:].sum())
    assert (sums[27], sums[28], sums[29]) == (n_rows, n_line, n_plane), (label, sums[27:30], n_rows, n_line, n_plane)
    assert (st["n_rows"], st["n_line"], st["n_plane"]) == (n_rows, n_line, n_plane)
    S, u = O.sums64_odom(f["pose"], q, coeff, kept)
    un = R.units(sums, S, u)
    assert un.max() <= O.K_ODOM, (label, "entry %d: %.1f units > %.0f" % (un.argmax(), un.max(), O.K_ODOM), un.round(1).tolist())
    # solve
    degenerate, deg_units = False, 0.0
    if n_rows < 10:  # :501-503: the iteration is skipped, the counter moves on
        assert np.array_equal(bits(st["pose"]), bits(f["pose"])) and st["loop_iter"] == it + 1 and st["solves"] == 0
    else:
        s32 = sums.astype(np.float32)
        AtA = np.zeros((6, 6), np.float32)
        for k, (i, j) in enumerate(R.PAIRS):
            AtA[i, j] = AtA[j, i] = s32[k]
        g = oracle.gn_step(AtA, s32[21:27], it, f["pose"], np.zeros(36, np.float32), False, eig_thresh=10.0, dr=0.1, dt=0.1)
        assert bool(st["degenerate"]) == g["degenerate"], label
        assert st["loop_iter"] == it + 1 and st["solves"] == 1
        if not g["degenerate"]:
            assert np.array_equal(bits(st["x"]), bits(g["x"])), (label, st["x"], g["x"])
            assert np.array_equal(bits(st["pose"]), bits(g["pose"])), (label, st["pose"], g["pose"])
            assert bool(st["converged"]) == g["converged"]
        elif it == 0:
            # the projected step (LaserOdometry.cpp:583-614, threshold 10): nothing pins the device's eigenvectors to the
            # oracle's bit for bit, so x and the pose are held within K_X units of the plain solve's error
            # (tests/degenerate_ref.py; measured: no difference at all); the pose is one float32 addition more.  The unit
            # grows with cond(A): on the far families, whose float32 sums are singular, only the decision and converged bind
            degenerate = True
            ux = D.unit_x_of(AtA, s32[21:27])
            dx = float(np.abs(st["x"].astype(np.float64) - g["x"]).max())
            dp = float(np.abs(st["pose"].astype(np.float64) - g["pose"]).max())
            deg_units = dx / ux if ux > 0 else (0.0 if dx == 0 else np.inf)
            print("%s: degenerate step, |x - oracle| %.3g = %.3g units (K_X %.2f, cond %.3g)" % (
                label, dx, deg_units, D.K_X, np.linalg.cond(AtA.astype(np.float64))))
            assert dx <= D.K_X * ux, (label, st["x"], g["x"], ux)
            assert dp <= D.K_X * ux + 2 * D.EPS32 * float(np.abs(g["pose"]).max()), (label, st["pose"], g["pose"], ux)
            assert bool(st["converged"]) == g["converged"], label
    return dict(sel=su, coeff=cd, sums=un.max(), rows=n_rows, degenerate=degenerate, deg_units=deg_units)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_one_step_against_the_references(pkg, ctx, oracle, fams, name):
    """One iteration of the loop per family and iteration counter through the tap, every output held as the module docstring
    says; then what the family is for is shown to have run, by the search profile's flags or the node's counters."""
    f = fams[name]
    ns, nf = len(f["sharp"]), len(f["flat"])
    nb = (ns + 255) // 256 + (nf + 255) // 256
    node = Node(pkg, ctx, f)
    dev = node.dev
    tr0 = dev.transform.copy()
    lc0, ls0 = dev.last_clouds()
    assert np.array_equal(bits(lc0), bits(f["lc"])) and np.array_equal(bits(ls0), bits(f["ls"]))
    for it in f["iters"]:
        label = "%s iter %d" % (name, it)
        st = dev.debug_step(node.fs, f["pose"], it, path=0, refresh=True)
        m = check_step(oracle, f, it, st, label)
        if it == 0:
            DEGENERATE_STEPS[name] = m["degenerate"]
            print("degenerate first steps so far: %d of %d families (%s)" % (sum(DEGENERATE_STEPS.values()), len(DEGENERATE_STEPS),
                                                                          ", ".join(k for k, v in DEGENERATE_STEPS.items() if v)))
            # (reference side: the oracle's decision on the device's sums) the families whose first step is projected
            assert m["degenerate"] == (name in DEGENERATE_AT_0), (name, m["degenerate"])
        prof = dev.search_profile(ns + nf)
        assert len(prof) == ns + nf
        print("%-32s rows %5d  sel %.2f units  coeff %.3g (bar %.3g)  sums %.2f units (K %.0f)  coarse %.0f%%  ring table %.0f%%" % (
            label, m["rows"], m["sel"], m["coeff"], O.COEFF_BAR_FACTOR * O.COEFF_COND[name], m["sums"], O.K_ODOM,
            100.0 * (prof[:, 3] & 1).astype(bool).mean(), 100.0 * (prof[:, 3] & 2).astype(bool).mean()))
        if it == f["iters"][0]:
            found = st["ind"][0] >= 0
            if name == "sparse_2_to_4.9m":   # the fine level cannot prove a category's nearest: the ring table is scanned
                assert ((prof[:, 3] & 2) != 0).mean() > 0.10, ((prof[:, 3] & 2) != 0).mean()
            if name == "pose_large":         # queries beyond the fine level's radius: the coarse level decides
                assert ((prof[:, 3] & 1) != 0).any() and (~found).any()
            if name == "far_3km":            # both levels usable: most queries are decided by the fine level alone
                assert (prof[:, 1] > 0).all() and ((prof[:, 3] & 1) != 0).mean() < 0.5
            if name == "far_10km":           # the fine level refused: every nearest neighbour comes from a coarse pass, and
                assert ((prof[:, 3] & 1) != 0).all() and found.all()          # every category from the ring table (the same
                assert ((prof[:, 3] & 2) != 0).all() and (prof[:, 2] > 0).any()  # clouds 3 km out: 4 % and 50 %)
            if name == "far_50km":           # both refused: no grid candidate at all, yet every query has its points --
                assert (prof[:, 1] == 0).all() and (prof[:, 2] == 0).all() and ((prof[:, 3] & 3) == 0).all()   # the whole
                assert found.all() and (st["ind"][1] >= 0).mean() > 0.9              # cloud was searched, the walk literal
            if name in ("not_ring_order", "rings_above_255"):  # the literal walk: no category pass over grid or ring table
                assert (prof[:, 2] == 0).all() and (st["ind"][1] >= 0).any()
        # without a refresh the step reuses the correspondences and gives the same bits
        if it % 5 != 0:
            again = dev.debug_step(node.fs, f["pose"], it, path=0, refresh=False)
            assert not again["refreshed"] and np.array_equal(again["ind"], st["ind"])
            assert np.array_equal(again["sums"], st["sums"]) and np.array_equal(bits(again["pose"]), bits(st["pose"]))
        # the persistent kernel, one generation
        if it in (4, 9, 24) and nb <= 64:
            p1 = dev.debug_step(node.fs, f["pose"], it, path=1)
            assert np.array_equal(p1["ind"], st["ind"]) and p1["tie"] == st["tie"]
            assert np.array_equal(p1["sums"].view(np.uint64), st["sums"].view(np.uint64)), label
            for k in ("pose", "x"):
                assert np.array_equal(bits(p1[k]), bits(st[k])), (label, k)
            for k in ("n_rows", "n_line", "n_plane", "degenerate", "converged", "done", "loop_iter", "solves"):
                assert p1[k] == st[k], (label, k)
    # the tap moved nothing
    assert np.array_equal(bits(dev.transform), bits(tr0))
    lc1, ls1 = dev.last_clouds()
    assert np.array_equal(bits(lc1), bits(f["lc"])) and np.array_equal(bits(ls1), bits(f["ls"]))
    if name.startswith("ragged_") and ns and nf:
        # path 1 at the block counts themselves (one generation at the last allowed iteration), and which loop the node takes
        if nb <= 64:
            p0 = dev.debug_step(node.fs, f["pose"], 24, path=0, refresh=True)
            p1 = dev.debug_step(node.fs, f["pose"], 24, path=1)
            assert np.array_equal(p1["sums"].view(np.uint64), p0["sums"].view(np.uint64)) and np.array_equal(p1["ind"], p0["ind"])
            assert np.array_equal(bits(p1["pose"]), bits(p0["pose"])) and p1["done"] == p0["done"] == 1
        else:
            with pytest.raises(pkg.LslamError):
                dev.debug_step(node.fs, f["pose"], 24, path=1)
        before = dev.run_counts()
        dev.process(node.fs)
        assert dev.last_ostats.matched == 1
        after = dev.run_counts()
        if nb > 64:   # 66 blocks: above OGN_MAX_BLOCKS, the node takes the launch loop
            assert (after[0] - before[0], after[1] - before[1]) == (0, 1), (nb, before, after)
        else:         # 64 blocks and fewer: the persistent kernel
            assert (after[0] - before[0], after[1] - before[1]) == (1, 0), (nb, before, after)
    node.close()


def test_the_tap_refuses_what_it_cannot_run(pkg, ctx, fams):
    """No last clouds yet, path 1 away from the end of a segment, per-point taps are path 0's, a reuse of correspondences that
    were never made: errors, not launches."""
    f = fams["pose_drive"]
    sr = pkg.scan_registration
    dev = pkg.DeviceLaserOdometry(ctx, publish=False)
    fs = sr.FeatureSet(ctx).upload(f["sharp"], f["lc"], f["flat"], f["ls"])
    with pytest.raises(pkg.LslamError):
        dev.debug_step(fs, f["pose"], 0)           # the node holds no last clouds
    dev.process(fs)
    with pytest.raises(pkg.LslamError):
        dev.debug_step(fs, f["pose"], 3, path=1)   # the kernel would run two generations
    with pytest.raises(pkg.LslamError):
        dev.debug_step(fs, f["pose"], 25)          # beyond max_iterations
    with pytest.raises(pkg.LslamError):
        dev.debug_step(fs, f["pose"], 3, refresh=False)  # nothing to reuse
    st = dev.debug_step(fs, f["pose"], 0)
    assert st["n_rows"] > 100
    dev.close()
    fs.close()


def _raw(synth, world, k, rings, steps):
    gt = (0.0, 0.0, 0.3 + 0.01 * k, 3.0 + 0.4 * k, -2.0 + 0.15 * k, synth.SENSOR_HEIGHT)
    _, _, _, cloud, _ = synth.make_scan(world, rings, steps, gt_pose=gt, seed=300 + k, full=True)
    ring = np.floor(cloud[:, 3]).astype(np.int64)
    return cloud[np.lexsort((ring, -(cloud[:, 3] - ring)))]


POSE_TOL_M, POSE_TOL_RAD = 1e-4, 1e-5   # the project's bar
END_TOL = 2e-5                          # test_gpu_pipeline.py::test_transform_to_end_matches_oracle
LOOP_TOL = 2e-3                         # test_gpu_pipeline.py's bar for loops that run to the iteration limit


def _pose_diff(a, b):
    return float(np.abs(a[3:] - b[3:]).max()), float(np.abs(a[:3] - b[:3]).max())


@pytest.mark.parametrize("rings,lo,hi", [(16, -15.0, 15.0), (64, -24.9, 2.0)])
def test_device_node_sweep_by_sweep_against_the_oracle(pkg, ctx, oracle, synth, small_problem, rings, lo, hi):
    """DeviceLaserOdometry.process over sweeps that go out and come back (0 1 2 3 2 1 0), 1800 azimuth steps.  Per sweep the
    oracle is given the DEVICE's last clouds and previous _transform, so differences do not compound.  Where the oracle's loop
    converges: iteration, row, line and plane counts equal, _transform within 1e-4 m / 1e-5 rad, the last clouds within 2e-5 of
    transformToEnd with the device's pose.  Where it runs to 25 iterations: the same bar on the first five iterations (the node
    behind the host-pointer entry and the oracle, both with max_iterations = 5, from the same clouds and previous _transform),
    the full loop printed and held at 2e-3."""
    sr = pkg.scan_registration
    world = small_problem["world"]
    dev = pkg.DeviceLaserOdometry(ctx, publish=False)
    fs = sr.FeatureSet(ctx)
    n_conv = n_long = 0
    for step, k in enumerate((0, 1, 2, 3, 2, 1, 0)):
        reg, rr = sr.multiscan_register(ctx, _raw(synth, world, k, rings, 1800), lo, hi, rings)
        sr.extract_features_dev(ctx, reg, rr, fs)
        if step == 0:
            assert dev.process(fs) is None
            continue
        lists = {key: fs.download(key) for key in sr.LISTS}
        lc, ls = dev.last_clouds()
        prev = dev.transform.copy()
        n, opose, ost = oracle.odometry_match(lc, ls, lists["sharp"], lists["flat"], prev)
        dev.process(fs)
        st, os_ = dev.last_stats, dev.last_ostats
        dm, dr = _pose_diff(dev.transform, opose)
        print("%d rings sweep %d: iterations %d (oracle %d, converged %d) rows %d |dt| %.3g |dr| %.3g tree_fallbacks %d" % (
            rings, step, st.iterations, ost.iterations, ost.converged, st.n_rows, dm, dr, os_.tree_fallbacks))
        assert os_.matched == 1
        if ost.converged:
            n_conv += 1
            assert (st.iterations, st.n_rows, st.n_line, st.n_plane, st.converged) == \
                   (ost.iterations, ost.n_rows, ost.n_line, ost.n_plane, 1), step
            assert dm <= POSE_TOL_M and dr <= POSE_TOL_RAD, (step, dm, dr)
        else:
            n_long += 1
            assert st.iterations == ost.iterations and st.sweeps == 25 and not st.converged
            assert dm <= LOOP_TOL and dr <= LOOP_TOL, (step, dm, dr)
            # the first segment of the same loop: a node with max_iterations = 5 started from the SAME previous _transform
            # (the host-pointer entry's node: lslam_odom_process always starts from the node's own _transform, which a fresh
            # node does not have) and the oracle with max_iterations = 5, on the same clouds
            _, pose5, st5 = ctx.odometry_match(lc, ls, lists["sharp"], lists["flat"], prev, max_iterations=5)
            n5, opose5, ost5 = oracle.odometry_match(lc, ls, lists["sharp"], lists["flat"], prev, max_iterations=5)
            dm5, dr5 = _pose_diff(pose5, opose5)
            print("    first segment: iterations %d rows %d |dt| %.3g |dr| %.3g (whole loop %.3g / %.3g)" % (
                st5.iterations, st5.n_rows, dm5, dr5, dm, dr))
            assert (st5.iterations, st5.sweeps, st5.n_rows, st5.n_line, st5.n_plane, st5.converged) == \
                   (ost5.iterations, n5, ost5.n_rows, ost5.n_line, ost5.n_plane, 0), step
            assert st5.sweeps == 5
            assert dm5 <= POSE_TOL_M and dr5 <= POSE_TOL_RAD, (step, dm5, dr5)
        nlc, nls = dev.last_clouds()
        for got, less in ((nlc, lists["less_sharp"]), (nls, lists["less_flat"])):
            ref = oracle.transform_to_end(less, dev.transform)
            assert np.array_equal(got[:, 3], less[:, 3]) and np.abs(got[:, :3] - ref[:, :3]).max() <= END_TOL, step
    print("%d rings: %d sweeps converged, %d ran to the limit" % (rings, n_conv, n_long))
    assert n_conv >= 1 and n_long >= 1  # both branches above ran
    dev.close()
    fs.close()
    ctx.map_set(small_problem["map_corner"], small_problem["map_surf"])
