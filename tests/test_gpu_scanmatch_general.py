"""The scan-match kernels at general poses, entry by entry (-m gpu, through the C ABI).

Every sweep kernel shares jacobian_row (csrc/lslam_device.hpp) and block_accumulate (csrc/lslam_sweep_dev.hpp).  The older
tests run them at roll, pitch ~ +-0.015 rad and hold all 27 normal-equation sums to one scale, the largest rotation entry.
Here: seven poses (tests/scanmatch_ref.general_pose_family: roll, pitch up to +-1.3 rad, yaw over +-pi, yaw = pi - 1e-3,
pitch = pi/2 - 0.02) and ragged scan sizes down to a single row.

  taps      idx, d2, flags, coeff bit for bit against oracle.sweep; counters exact -- as before, now at general poses
  sums      each of the 21 + 6 within K * u[k] of the float64 sums of float64 rows built from the DEVICE's taps
            (scanmatch_ref.reference_sums; u[k] = 2**-24 * sum of the entry's majorant terms, K = 92: derived from the
            reduction's structure in scanmatch_ref.k_apriori, above ten times the measured fp32 floor of 1.7)
  two paths MFMA against VALU within 2 K u[k] per entry
  loops     scanmatch_full against oracle.scanmatch_scan from every family pose: status, iterations, converged, counts equal,
            pose within 1e-4 m / 1e-5 rad; the persistent loop and a batch against the launch loop / the single runs bit for bit

Each test prints the largest distance it saw in units u[k] before asserting.  Measured on an MI355X when this file was
written: 0.5 .. 1.5 units over the family (1.48 at yaw = pi - 1e-3 in all eight combinations of search and contraction:
what the two contractions share -- the float32 rows and sin/cos -- dominates there), 3.5 on the ragged subsets, 1.3 between
MFMA and VALU; the stereo sums 7.1 units (one wavefront's chain of 183 rows).  All of it is inside ten times the fp32
floors as well; no defect was found.  Not covered here: odometry variant B at large initial transforms (its de-skew makes
the oracle comparison chaotic there) and the ICP kernel.
"""
import numpy as np
import pytest

import scanmatch_ref as R

pytestmark = pytest.mark.gpu

POSE_TOL_M = 1e-4    # BASELINE.json north_star
POSE_TOL_RAD = 1e-5
GRID = 3             # LSLAM_SEARCH_GRID
SEARCH_SHAPES = {"lane": 1 | 0x100, "lane_shallow": 1 | 0x200, "packet": 2, "grid": GRID}
SHAPE_VARIANT = {"lane": "deep", "lane_shallow": "shallow", "packet": "packet"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def fam(small_problem, oracle):
    """The family with the oracle's sweep at every member (computed once, never modified)."""
    pr = small_problem
    tc, ts = oracle.kdtree(pr["map_corner"]), oracle.kdtree(pr["map_surf"])
    members = R.general_pose_family(pr)
    for m in members:
        m["oracle"] = oracle.sweep(tc, ts, m["corner"], m["surf"], m["pose"])
    return dict(members=members, tc=tc, ts=ts)


def _assert_sweep(g, o, pose, corner, surf, label):
    """Device sweep g against oracle sweep o (taps, counters) and against the float64 reference built from g's own taps
    (sums).  -> the largest distance in units."""
    assert np.array_equal(g["idx"], o["idx"]), label
    assert np.array_equal(bits(g["d2"]), bits(o["d2"])), label
    assert np.array_equal(g["flags"], o["flags"]), label
    assert np.array_equal(bits(g["coeff"]), bits(o["coeff"])), label
    assert g["sums"][27] == o["sums"][27] and g["sums"][28] == o["sums"][28], label
    q = np.concatenate([corner, surf])
    S, u = R.reference_sums(pose, q, g["coeff"], g["flags"])
    un = R.units(g["sums"], S, u)
    assert int(g["sums"][27]) == int(((g["flags"] & 4) != 0).sum()), label
    assert un.max() <= R.K, (label, "entry %d: %.1f units" % (un.argmax(), un.max()), un.round(1).tolist())
    return float(un.max())


@pytest.mark.parametrize("search", ["lane", "lane_shallow", "packet", "grid"])
@pytest.mark.parametrize("jtj_mode", [0, 1])
def test_sweep_sums_per_entry_at_general_poses(ctx, fam, small_problem, jtj_mode, search):
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    worst = []
    for m in fam["members"]:
        ctx.scan_set(m["corner"], m["surf"])
        before, g0 = ctx.sweep_launches(), ctx.grid_launches()
        g = ctx.sweep(m["pose"], jtj_mode=jtj_mode, search_mode=SEARCH_SHAPES[search])
        after = ctx.sweep_launches()
        if search == "grid":
            assert ctx.grid_launches() == g0 + 1
        else:  # the instantiation asked for is the one that ran
            assert after[SHAPE_VARIANT[search]] - before[SHAPE_VARIANT[search]] == 1
            assert sum(after.values()) - sum(before.values()) == 1 and ctx.grid_launches() == g0
        assert ((m["oracle"]["flags"] & 4) != 0).sum() > 10000
        worst.append(_assert_sweep(g, m["oracle"], m["pose"], m["corner"], m["surf"], (m["name"], jtj_mode, search)))
    print("jtj_mode %d %s: max units per pose %s (K = %.0f)" % (jtj_mode, search, np.round(worst, 2).tolist(), R.K))


@pytest.mark.parametrize("which", [0, R.TILTED])
@pytest.mark.parametrize("jtj_mode", [0, 1])
def test_ragged_sizes_per_entry(ctx, oracle, fam, small_problem, jtj_mode, which):
    """(n_corner, n_surf) from one point to two blocks and a bit, kept rows first: blocks in which a single lane carries a
    non-zero row, partly filled last wavefronts, an empty corner or surf cloud.  Fewer than 50 kept rows are too few for a
    solve, not for the sums: those must match per entry all the same."""
    pr = small_problem
    m = fam["members"][which]
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    worst, few = 0.0, 0
    for n_c, n_s in R.RAGGED:
        corner, surf = R.ragged_subset(m, m["oracle"]["flags"], n_c, n_s)
        o = oracle.sweep(fam["tc"], fam["ts"], corner, surf, m["pose"])
        kept = int(((o["flags"] & 4) != 0).sum())
        assert kept == n_c + n_s  # kept rows first: every row of the subset is a non-zero row
        few += int(kept < 50)
        ctx.scan_set(corner, surf)
        for search in ("lane", "grid"):
            g = ctx.sweep(m["pose"], jtj_mode=jtj_mode, search_mode=SEARCH_SHAPES[search])
            worst = max(worst, _assert_sweep(g, o, m["pose"], corner, surf, (m["name"], jtj_mode, search, n_c, n_s)))
    assert few >= 2
    print("ragged, jtj_mode %d at %s: max %.2f units (K = %.0f)" % (jtj_mode, m["name"], worst, R.K))


def test_mfma_equals_valu_per_entry_at_a_tilted_pose(ctx, fam, small_problem):
    pr = small_problem
    m = fam["members"][R.TILTED]
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set(m["corner"], m["surf"])
    a = ctx.sweep(m["pose"], jtj_mode=0)
    b = ctx.sweep(m["pose"], jtj_mode=1, taps=False)["sums"]
    S, u = R.reference_sums(m["pose"], np.concatenate([m["corner"], m["surf"]]), a["coeff"], a["flags"])
    d = np.abs(a["sums"][:27].astype(np.float64) - b[:27].astype(np.float64)) / u
    print("MFMA against VALU at %s: max %.2f units (bound %.0f)" % (m["name"], d.max(), 2 * R.K))
    assert d.max() <= 2 * R.K, d.round(1).tolist()
    assert np.array_equal(a["sums"][27:29], b[27:29])


@pytest.mark.parametrize("which", range(7))
def test_full_loop_matches_oracle_from_every_family_pose(ctx, oracle, fam, small_problem, which):
    """The family pose is as far from the pose at which the member's scan matches the map as init_pose is from gt_pose (a
    perturb_pose-sized offset by construction).  Whatever the oracle does from there -- yaw next to pi and pitch next to
    pi/2 included -- the device does: same status, iterations, converged flag and counts, pose within the bar."""
    pr = small_problem
    m = fam["members"][which]
    status, pose, st = ctx.scanmatch_full(pr["map_corner"], pr["map_surf"], m["corner"], m["surf"], m["pose"])
    ok, opose, ost = oracle.scanmatch_scan(pr["map_corner"], pr["map_surf"], m["corner"], m["surf"], m["pose"])
    print("%s: status %d iterations %d converged %d rows %d |dt| %.2e |dr| %.2e" %
          (m["name"], st.status, st.iterations, st.converged, st.n_rows, np.abs(pose[3:] - opose[3:]).max(), np.abs(pose[:3] - opose[:3]).max()))
    assert (status == 0) == ok and st.status == ost.status
    assert st.iterations == ost.iterations and st.converged == ost.converged
    assert (st.n_line, st.n_plane, st.n_rows) == (ost.n_line, ost.n_plane, ost.n_rows)
    assert np.abs(pose[3:] - opose[3:]).max() <= POSE_TOL_M
    assert np.abs(pose[:3] - opose[:3]).max() <= POSE_TOL_RAD
    assert abs(st.score - ost.score) <= 1e-5 * ost.score and abs(st.percent - ost.percent) <= 1e-6


def test_batch_equals_single_runs_at_tilted_poses(ctx, fam, small_problem):
    """Two tilted members and the near-identity one matched together give, bit for bit, what each gives alone (the form of
    test_gpu_parity.test_batch_equals_individual_runs)."""
    pr = small_problem
    ms = [fam["members"][i] for i in (R.TILTED, 0, 3)]
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    single = [ctx.scanmatch_scan(m["corner"], m["surf"], m["pose"]) for m in ms]
    ctx.scan_set_batch([(m["corner"], m["surf"]) for m in ms])
    worst, poses, stats = ctx.run_batch(np.stack([m["pose"] for m in ms]))
    for k, (status, pose, st) in enumerate(single):
        assert stats[k].status == st.status and stats[k].iterations == st.iterations, k
        assert (stats[k].n_rows, stats[k].n_line, stats[k].n_plane) == (st.n_rows, st.n_line, st.n_plane), k
        assert np.array_equal(bits(poses[k]), bits(pose)), k
        assert st.converged == 1, k
