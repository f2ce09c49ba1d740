"""The lean instantiation of the grid sweep's SECOND pass (sweep_queue_kernel<256, true, 12, 1, true>): where the production
loop's first pass runs lean (tests/test_gpu_grid_lean.py), the tree search of the points it listed runs a kernel with the
shuffle sums, the taps, the _fineScore gate, the clocks and the counters folded away at compile time, a leaf that fetches
12 bytes per slot and nothing kept in registers from one work item to the next.  Same operations on the same values: the SAME
BITS as the general instantiations, which lslam_opts.ab_switches & LSLAM_AB_GRID_GENERAL (256) brings back for both passes --
poses, stats, and what the sweeps carry per point (where it was, how far its fifth neighbour).  Every launch that needs a
folded path keeps the general kernel (lslam_debug_queue_lean_launches counts the lean ones)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANE, GRID = 1, 3
AB_GRID_GENERAL = 256
TOO_FEW_MATCHES = 5
TIMES = ("gpu_ms_total", "gpu_ms_sweep")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stats_but_times(st):
    return [(name, getattr(st, name)) for name, _ in st._fields_ if name not in TIMES]


def cloud(xyz):
    xyz = np.asarray(xyz, np.float32)
    return np.concatenate([xyz[:, :3], np.zeros((len(xyz), 1), np.float32)], 1)


def carried_state(ctx, n_points):
    """lslam_debug_cert_state with the fourth word kept: per resident point {x, y, z, fifth squared distance} as the last sweep
    that handled it left them, and the per-point array beside it (the grid sweep's hints from pass 1 to pass 2)."""
    q = np.zeros((n_points, 4), np.float32)
    lb = np.zeros(n_points, np.float32)
    fp = C.POINTER(C.c_float)
    n = ctx.lib.lslam_debug_cert_state(ctx.h, q.ctypes.data_as(fp), lb.ctypes.data_as(fp), n_points)
    assert n == n_points, (n, n_points)
    return q, lb


def counters(ctx):
    return ctx.queue_lean_launches(), ctx.grid_lean_launches(), ctx.grid_launches(), ctx.sweep_launches()


def settle(call):
    """A call sizes its first batch of launches from the iterations of the calls before it (one spare launch until three calls
    in a row have run the same number): three calls ahead, and every repetition that follows launches the same."""
    for _ in range(3):
        call()


def lean_and_general(ctx, inits, n_points, **opts):
    """The resident batch through the grid sweep with the lean kernels and with the general ones: equal status, byte-equal
    poses, equal stats but for the two times, byte-equal carried state, equal grid- and sweep-launch counts; the lean second
    pass ran in every sweep of the first run and in none of the second.  -> (poses, stats) of the lean run."""
    o = ctx.default_opts()
    o.search_mode = GRID
    for k, v in opts.items():
        setattr(o, k, v)
    inits = np.asarray(inits, np.float32)
    o.ab_switches = AB_GRID_GENERAL
    settle(lambda: ctx.run_batch(inits, o))
    res = []
    for ab in (0, AB_GRID_GENERAL):
        o.ab_switches = ab
        q0, l0, g0, s0 = counters(ctx)
        rc, p, st = ctx.run_batch(inits, o)
        q1, l1, g1, s1 = counters(ctx)
        grid = g1 - g0
        assert grid > 0
        assert (q1 - q0, l1 - l0) == ((grid, grid) if ab == 0 else (0, 0)), (ab, q1 - q0, l1 - l0, grid)
        res.append((int(rc), p.copy(), st, carried_state(ctx, n_points), grid, {k: s1[k] - s0[k] for k in s1}))
    lean, gen = res
    assert lean[0] == gen[0]
    assert np.array_equal(bits(lean[1]), bits(gen[1]))
    assert len(lean[2]) == len(gen[2])
    for a, b in zip(lean[2], gen[2]):
        assert stats_but_times(a) == stats_but_times(b)
    assert np.array_equal(bits(lean[3][0]), bits(gen[3][0]))  # position and fifth distance per point
    assert np.array_equal(bits(lean[3][1]), bits(gen[3][1]))
    assert lean[4] == gen[4] and lean[5] == gen[5]
    return lean[1], lean[2]


def listed_by_sweep(ctx, inits, **opts):
    """Points the first pass listed for the second, [type][sweep of the loop], of one run with the counters on (which takes
    the general kernels: the lists are the same ones)."""
    o = ctx.default_opts()
    o.search_mode = GRID
    o.debug_stats = 1
    for k, v in opts.items():
        setattr(o, k, v)
    before = ctx.grid_stats().astype(np.int64)
    ctx.run_batch(np.asarray(inits, np.float32), o)
    listed = (ctx.grid_stats().astype(np.int64) - before)[:, :, 0]
    print("points listed for pass 2 [corner, surf][sweep]:", listed.tolist())
    return listed


def n_points_of(scans):
    return sum(len(c) + len(s) for c, s in scans)


def test_seven_scans_three_in_flight(ctx, synth, small_problem):
    """Seven copies of the scan, start poses further and further from the truth: loops of different length, first sweeps
    that list many points and late sweeps that list few, chunks of three scans."""
    pr = small_problem
    scans = [(pr["corner"], pr["surf"])] * 7
    inits = np.stack([synth.perturb_pose(pr["gt_pose"], seed=40 + k, dt=0.05 + 0.05 * k, dr_deg=0.3 + 0.3 * k) for k in range(7)])
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set_batch(scans)
    _, st = lean_and_general(ctx, inits, n_points_of(scans), scans_in_flight=3)
    assert all(s.sweeps >= 2 for s in st) and len({s.sweeps for s in st}) > 1
    listed = listed_by_sweep(ctx, inits, scans_in_flight=3)
    assert listed[:, 0].sum() > listed[:, 1].sum() > 0


def test_a_group_with_more_than_one_item(ctx, synth, small_problem):
    """One 32 x 1800 scan (its surf points are one group of the planner) started far off: the first sweep lists more than a
    workgroup's worth of points in that group, so the group is cut into several items that share a prefix."""
    pr = small_problem
    corner, surf, gt = synth.make_scan(pr["world"], 32, 1800, gt_pose=tuple(float(v) for v in pr["gt_pose"]), seed=77)
    assert 256 < len(surf) <= 256 * 256
    init = np.asarray(gt, np.float32).copy()
    init[:3] += np.deg2rad([1.5, -2.0, 4.0]).astype(np.float32)
    init[3:] += np.array([0.8, -0.6, 0.25], np.float32)
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set_batch([(corner, surf)])
    lean_and_general(ctx, init[None], len(corner) + len(surf))
    listed = listed_by_sweep(ctx, init[None])
    assert listed[1, 0] > 256


def test_a_scan_beyond_the_map(ctx, small_problem):
    """Every point farther than the gate from every map point: empty lists, a plan without items, too few matches."""
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set_batch([(pr["corner"], pr["surf"])])
    far = np.asarray(pr["init_pose"], np.float32).reshape(1, 6).copy()
    far[0, 3] += 400.0
    _, st = lean_and_general(ctx, far, len(pr["corner"]) + len(pr["surf"]))
    assert st[0].status == TOO_FEW_MATCHES and st[0].n_line == 0 and st[0].n_plane == 0
    assert listed_by_sweep(ctx, far).sum() == 0


def test_a_scan_of_fewer_than_64_points(ctx, small_problem):
    """Whatever such a scan lists fits one wavefront of one item; the other three take part in the barriers and the sums."""
    pr = small_problem
    corner, surf = pr["corner"][::40][:20], pr["surf"][::200][:40]
    assert 0 < len(corner) + len(surf) < 64
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set_batch([(corner, surf)])
    init = np.asarray(pr["init_pose"], np.float32).reshape(1, 6)
    lean_and_general(ctx, init, len(corner) + len(surf))
    lean_and_general(ctx, init, len(corner) + len(surf), max_iterations=1)  # a first sweep alone (nothing carried)


@pytest.mark.parametrize("name", ["lattice_ties", "duplicates"])
def test_exact_ties_go_to_the_second_pass(ctx, goldens, name):
    """The tie fixtures as map and scan, started at the identity: the first pass refuses to prove a point whose answer depends
    on nanoflann's visit order, so the second pass's tree search decides those -- the lean one as the general one."""
    g = goldens[name]
    pts, q = cloud(g["pts"]), cloud(g["queries"])
    ctx.map_set(pts, pts)
    scans = [(q[: len(q) // 4], q), (q[: len(q) // 4], q)]
    inits = np.array([[0, 0, 0, 0, 0, 0], [0.002, -0.003, 0.004, 0.03, -0.02, 0.01]], np.float32)
    ctx.scan_set_batch(scans)
    lean_and_general(ctx, inits, n_points_of(scans))
    assert listed_by_sweep(ctx, inits)[:, 0].sum() > 0


def test_launches_that_need_a_folded_path_keep_the_general_kernel(ctx, small_problem):
    """The counters, the shuffle sums, the taps and a fine_score call's re-sweep: the lean second pass runs in none of them
    (in the loop of the fine_score call it does; its re-sweep is one more grid sweep, general)."""
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set(pr["corner"], pr["surf"])
    init = np.asarray(pr["init_pose"], np.float32).reshape(1, 6)

    def deltas(run):
        q0, l0, g0, _ = counters(ctx)
        run()
        q1, l1, g1, _ = counters(ctx)
        return q1 - q0, l1 - l0, g1 - g0

    def batch(**opts):
        o = ctx.default_opts()
        o.search_mode = GRID
        for k, v in opts.items():
            setattr(o, k, v)
        return lambda: ctx.run_batch(init, o)

    settle(batch())
    ql, l, grid = deltas(batch())
    assert grid > 0 and ql == l == grid
    for opts in (dict(debug_stats=1), dict(jtj_mode=0), dict(ab_switches=AB_GRID_GENERAL)):
        assert deltas(batch(**opts)) == (0, 0, grid), opts
    ql, l, g = deltas(lambda: ctx.sweep(pr["init_pose"], jtj_mode=1, search_mode=GRID))  # lslam_sweep_ex with the taps
    assert g == 1 and ql == 0 and l == 0

    def single(**opts):
        o = ctx.default_opts()
        o.search_mode = GRID
        o.fine_score = 1
        for k, v in opts.items():
            setattr(o, k, v)
        return lambda: ctx.run(pr["init_pose"], o)

    settle(single())
    ql, l, g = deltas(single())
    assert g == l + 1 and ql == l and l >= 2
    assert deltas(single(ab_switches=AB_GRID_GENERAL)) == (0, 0, g)
