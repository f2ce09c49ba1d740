"""The coarse alignment's kernel and host fit, step by step against tests/icp_ref.py (-m gpu).

lslam_debug_icp_step runs ONE correspondence pass of lslam_icp_align's loop -- the loop's own launch with two tap pointers set
-- and returns, per source point, the paired target index and the float32 squared distance, the 18 reduced sums, and the fit
the host would compose into T.  Every input of icp_ref.cases(): general rotations and a translation of hundreds of metres in
the running transform, block and wavefront tails, targets of fewer than five points, gates (one exactly on a distance), the
overflow-stack instantiation, planar clouds and rank-deficient targets.

  index, d2, n, the instantiation flag, iteration counts: exact
  sums: |device - exact| <= (n - 1) 2^-53 sum |term| per entry (any order of fp64 summation), nothing on top
  fit: test_icp_ref.FIT_BAR per family (measured there on the reference alone); rank-deficient: rigid + minimal objective

Every condition these comparisons rely on (no ties, gates away from distances, loop decisions away from their thresholds, the
mutations they see) is tests/test_icp_ref.py's, on the CPU.
"""
import os
import sys

import numpy as np
import pytest

import icp_ref as I
from test_icp_ref import FIT_BAR, ORACLE_TOL_M, ORACLE_TOL_R, bars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def prepared():
    """Every case with its reference step, computed once and left unchanged."""
    return [dict(c, ref=I.ref_step(c["target"], c["source"], c["T"], c["gate"])) for c in I.cases()]


@pytest.fixture(scope="module")
def taps(ctx_module, prepared):
    return {c["name"]: ctx_module.icp_step(c["target"], c["source"], c["T"], c["gate"] or 0.0) for c in prepared}


@pytest.fixture(scope="module")
def ctx_module(_session_ctx):
    return _session_ctx


def test_every_step_against_the_reference(prepared, taps):
    """Index, distance, count, the 17 sums and the fit of one pass, every case."""
    failures, worst_sum, worst_R = [], 0.0, {}
    for c in prepared:
        tap, r = taps[c["name"]], c["ref"]
        bad = I.compare_step(tap, r, *bars(c), degenerate=c["degenerate"])
        if tap["overflow_stack"] != c["deep"]:
            bad.append("instantiation: overflow stack %r" % tap["overflow_stack"])
        if tap["blocks"] != (r["m"] + 127) // 128:
            bad.append("blocks %d" % tap["blocks"])
        if bad:
            failures.append((c["name"], bad[:4]))
        err, bound = I.sum_errors(tap["sums"], r), I.sums_bound(r["n"], r["maj"])
        if r["n"] > 1:
            worst_sum = max(worst_sum, (err[1:17][bound[1:17] > 0] / bound[1:17][bound[1:17] > 0]).max())
        if r["fit"] is not None and not c["degenerate"] and tap["fitted"]:
            w = worst_R.setdefault(c["family"], [0.0, 0.0])
            w[0] = max(w[0], np.abs(tap["R"] - r["fit"]["R"]).max())
            w[1] = max(w[1], np.abs(tap["t"] - r["fit"]["t"]).max())
    print("largest |sum - exact| / bound: %.3g" % worst_sum)
    for k, (a, b) in sorted(worst_R.items()):
        print("%-14s |R - ref| %.2e (bar %.1e)  |t - ref| %.2e (bar %.1e)" % (k, a, FIT_BAR[k][0], b, FIT_BAR[k][1]))
    assert failures == []


def test_both_instantiations_ran_and_agree(prepared, taps):
    """The deep target takes icp_corr_kernel<true>, the same input without the far clusters icp_corr_kernel<false>: the same
    indices (into the shared prefix), distances and sums, bit for bit."""
    for deep, flat in (("deep", "pose_rand1"), ("deep_gate0.6", "pose_rand1_gate0.6")):
        a, b = taps[deep], taps[flat]
        assert a["overflow_stack"] and not b["overflow_stack"]
        assert np.array_equal(a["idx"], b["idx"]) and a["idx"].max() < 1600
        assert np.array_equal(bits32(a["d2"]), bits32(b["d2"])) and np.array_equal(bits64(a["sums"]), bits64(b["sums"]))
        assert np.array_equal(bits64(a["R"]), bits64(b["R"])) and np.array_equal(bits64(a["t"]), bits64(b["t"]))


def test_strides_give_the_same_bits(ctx, prepared, taps):
    by = {c["name"]: c for c in prepared}
    for name in ("pose_init", "pose_rand0_gate0.6"):
        c, want = by[name], taps[name]
        T16, conv16, its16, fit16 = ctx.icp_align(c["target"], c["source"], c["T"], max_correspondence_distance=c["gate"] or 0.0)
        for stride in (12, 32):
            t, s = I.with_stride(c["target"], stride), I.with_stride(c["source"], stride)
            got = ctx.icp_step(t, s, c["T"], c["gate"] or 0.0)
            assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(bits32(got["d2"]), bits32(want["d2"])), (name, stride)
            assert np.array_equal(bits64(got["sums"]), bits64(want["sums"])), (name, stride)
            T, conv, its, fit = ctx.icp_align(t, s, c["T"], max_correspondence_distance=c["gate"] or 0.0)
            assert np.array_equal(bits32(T), bits32(T16)) and (conv, its, fit) == (conv16, its16, fit16), (name, stride)


def test_one_iteration_composes_the_taps_fit(ctx, prepared, taps):
    """lslam_icp_align with max_iterations = 1 returns the float32 rounding of [R | t] T of the tap's own R, t (the same
    kernels: the same bits), one iteration, converged (the cap counts as convergence), and as fitness the mean squared distance
    of a reference step at the returned transform."""
    ran = 0
    for c in prepared:
        tap, r = taps[c["name"]], c["ref"]
        if not tap["fitted"]:
            continue
        ran += 1
        T, conv, its, fit = ctx.icp_align(c["target"], c["source"], c["T"], max_iterations=1, max_correspondence_distance=c["gate"] or 0.0)
        want = I.compose(tap["R"], tap["t"], c["T"]).astype(np.float32)
        assert np.array_equal(bits32(T), bits32(want)), c["name"]
        assert (conv, its) == (True, 1), c["name"]
        after = I.ref_step(c["target"], c["source"], T, c["gate"])
        if after["n"] == 0:
            assert fit == I.DBL_MAX, c["name"]
            continue
        exact = after["sums"][1] / after["n"]
        # the sum's derived bound, divided by n, + the rounding of the division itself
        bound = I.sums_bound(after["n"], after["maj"])[1] / after["n"] + 2.0 ** -52 * exact
        assert abs(fit - exact) <= bound, (c["name"], fit, exact, bound)
    assert ran >= 40


@pytest.fixture(scope="module")
def loops(prepared):
    return [dict(c, max_iterations=mi, align=I.ref_align(c["target"], c["source"], c["T"], max_iterations=mi, gate=c["gate"]))
            for c in prepared for mi, _ in c["loop"]]


def test_whole_loops_against_ref_align_and_the_oracle(ctx, loops):
    """Iteration count and converged flag exact against ref_align, the transform at the fit bar times the iteration count plus
    float32 rounding; and within tests/test_icp.py's 1e-4 m / 1e-5 of oracle/icp_oracle.py."""
    import icp_oracle
    assert len(loops) == 12
    for c in loops:
        a = c["align"]
        T, conv, its, fit = ctx.icp_align(c["target"], c["source"], c["T"], max_iterations=c["max_iterations"],
                                          max_correspondence_distance=c["gate"] or 0.0)
        d = np.abs(T.astype(np.float64) - a["T"])
        print("%-14s max %2d: %d iterations (reference %d), |T - ref| rotation %.2e translation %.2e, fitness %.3g (%.3g)"
              % (c["name"], c["max_iterations"], its, a["iterations"], d[:3, :3].max(), d[:3, 3].max(), fit, a["fitness"]))
        if c["name"] == "identical":
            # fitness 0, the guess returned within float32 rounding, converged within 2 iterations: whether the first
            # increment has cos(angle) >= 1 and zero translation exactly is decided by rounding
            assert conv and its <= 2 and fit == 0.0
            assert np.abs(T - np.eye(4, dtype=np.float32)).max() <= 2.0 ** -23
        else:
            assert I.compare_align(T, conv, its, a, *bars(c)) == [], c["name"]
        To, _, _, _ = icp_oracle.icp_align(c["target"], c["source"], c["T"], max_iterations=c["max_iterations"], max_corr_dist=c["gate"])
        assert np.abs(T[:3, 3] - To[:3, 3]).max() <= ORACLE_TOL_M and np.abs(T[:3, :3] - To[:3, :3]).max() <= ORACLE_TOL_R, c["name"]
        assert np.array_equal(T[3], [0, 0, 0, 1])


def test_guards(ctx, prepared):
    """Fewer than 3 correspondences: not converged, no iteration, T untouched; the empty source's fitness is DBL_MAX (PCL's
    getFitnessScore() without correspondences).  Every rank-deficient target: a finite, rigid transform."""
    by = {c["name"]: c for c in prepared}
    for name in ("source_0", "source_1", "source_2", "gate_keeps_2"):
        c = by[name]
        T, conv, its, fit = ctx.icp_align(c["target"], c["source"], c["T"], max_correspondence_distance=c["gate"] or 0.0)
        assert (conv, its) == (False, 0) and np.array_equal(bits32(T), bits32(c["T"])), name
        if name == "source_0":
            assert fit == I.DBL_MAX
    ran = 0
    for c in prepared:
        if not c["degenerate"]:
            continue
        ran += 1
        T, conv, its, fit = ctx.icp_align(c["target"], c["source"], c["T"])
        R = T[:3, :3].astype(np.float64)
        assert np.isfinite(T).all() and np.isfinite(fit) and conv and its >= 1, c["name"]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * 2.0 ** -23, (c["name"], np.abs(R @ R.T - np.eye(3)).max())
        assert np.linalg.det(R) > 0.5 and np.array_equal(T[3], [0, 0, 0, 1]), c["name"]
    assert ran == 8


def test_an_icp_call_takes_the_map(pkg, ctx, small_problem, prepared):
    """lslam_icp_align puts the target's tree into the context's map: lslam_map_epoch changes, and a ScanMatch that had its
    reference clouds resident on the same context uploads them again instead of matching against the ICP's target."""
    pr = small_problem
    sm = pkg.ScanMatch(10, ctx=ctx)
    sm.setReferenceEpoch(7)
    lib, h = ctx.lib, ctx.h
    ok0, pose0 = sm.scanMatchScan(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"], pr["init_pose"])
    e0 = lib.lslam_map_epoch(h)
    sm.scanMatchScan(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"], pr["init_pose"])
    assert e0 != 0 and lib.lslam_map_epoch(h) == e0      # resident: no map set
    c = prepared[0]
    ctx.icp_align(c["target"], c["source"], c["T"], max_iterations=1)
    e1 = lib.lslam_map_epoch(h)
    assert e1 != e0                                      # (0: the map is nobody's resident map any more)
    ok2, pose2 = sm.scanMatchScan(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"], pr["init_pose"])
    assert ok2 == ok0 and np.array_equal(bits32(pose0), bits32(pose2))
    e2 = lib.lslam_map_epoch(h)
    assert e2 not in (0, e0)                             # uploaded again
    ctx.icp_step(c["target"], c["source"], c["T"])       # the tap takes the map as the call it mirrors does
    assert lib.lslam_map_epoch(h) != e2
