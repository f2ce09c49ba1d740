"""The paged mode of the localisation node (lslam_pmap_*, csrc/lslam_loc.hip; util/DynamicFeatureMap.h) against its
restatement (tests/paged_map_ref.py, composed from the CPU oracle) and against the static node over the same files: the
window's contents and counters step by step, the search tap against the oracle tree of every query's cube, single sweeps and the trajectory,
staging, refusals, the mirrors and the lifetime of the step's buffers.

The scene: localization_ref's world and sweeps, every sweep cut to 30 m, the map binned into 10 m cubes (133 corner and 297 surf
files, indices -6..6, -6..6, 0..2), a 9 x 9 x 5 window, valid distance 20 m, map leaves 1.0 / 1.0."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import localization_ref as lr
import paged_map_ref as pm

pytestmark = pytest.mark.gpu

TOL_T, TOL_R = 1e-4, 1e-5  # the project's pose tolerances
STEP_S = 0.2
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def scene(synth):
    return pm.make_scene(synth, 4)


@pytest.fixture(scope="module")
def mapdir(scene, tmp_path_factory):
    """index2.txt (global indices) and index.txt (+ the static array's origin) over the same PCDs."""
    d = str(tmp_path_factory.mktemp("paged_map"))
    index = pm.write_paged_map(d, scene["map_corner"], scene["map_surf"], pm.CUBE)
    assert (len(index[0]), len(index[1])) == (133, 297)
    with open(os.path.join(d, "index.txt"), "w") as f:
        for line in open(os.path.join(d, "index2.txt")):
            w = [int(v) for v in line.split()]
            f.write("%d %d %d %d %d %d\n" % (w[0], w[1], w[2] + pm.STATIC_ORIGIN[0], w[3] + pm.STATIC_ORIGIN[1], w[4] + pm.STATIC_ORIGIN[2], w[5]))
    return d


def _ref(oracle, directory):
    return pm.RefPagedMap(oracle, directory, pm.WINDOW, pm.CUBE, pm.VALID, *pm.LEAVES)


def _node(pkg, ctx, directory, dims=pm.WINDOW, valid=pm.VALID, grid=True, capacity=None):
    node = pkg.LaserLocalization(ctx, *dims, map_filter_corner=pm.LEAVES[0], map_filter_surf=pm.LEAVES[1], cube_size=pm.CUBE,
                                 lidar_valid_distance=valid, dynamic_mode=True, files_directory=directory, paged_capacity=capacity)
    node.set_search(grid)
    return node


def _static_node(pkg, ctx, directory, grid=True):
    node = pkg.LaserLocalization(ctx, *pm.STATIC_DIMS, map_filter_corner=pm.LEAVES[0], map_filter_surf=pm.LEAVES[1], cube_size=pm.CUBE,
                                 world_origin=pm.STATIC_ORIGIN, lidar_valid_distance=pm.VALID)
    node.load_map(directory)
    node.set_search(grid)
    return node


def _xyz(scene, k):
    return np.asarray(scene["poses"][k][3:6], F)


def _prior(synth, scene, k):
    """Sweep k's ground truth with the rotation perturbed and the translation kept: the sensor cubes are (0,0,0), (1,0,0),
    (1,0,0), (2,0,0), so sweeps 1 and 3 step the window (22 and 18 files)."""
    p = synth.perturb_pose(scene["poses"][k], seed=99 + k, dt=0.2, dr_deg=1.0)
    p[3:] = _xyz(scene, k)
    return p


def _queries(ref, rng, n=1000):
    """Map-frame queries per type: resident map points near the sensor, jittered; some land in cubes without a tree."""
    out = []
    for t in range(2):
        cloud = ref.window_map()[t]
        pick = cloud[rng.integers(0, len(cloud), n), :3]
        out.append((pick + rng.normal(0, 0.4, pick.shape)).astype(F))
    return out


def _oracle_in_cube(ref, t, q):
    """Five nearest of every query inside its own cube of the window: ``oracle.kdtree(cube).knn`` -- nanoflann's traversal, which
    also decides which of several tied points is returned.  tie: an exact tie among the six nearest (fp32, x -> y -> z)."""
    nq = len(q)
    xyz, d2 = np.zeros((nq, 5, 3), F), np.zeros((nq, 5), F)
    ok, tie = np.zeros(nq, bool), np.zeros(nq, bool)
    g = pm.glo_idx(q, ref.cube_size)
    trees = {}
    for i in range(nq):
        key = tuple(int(v) for v in g[i])
        if not ref.in_window(key):
            continue
        pts = ref.cubes[t].get(key)
        if pts is None or len(pts) < 5:
            continue
        if key not in trees:
            trees[key] = ref.o.kdtree(pts)
        idx, d = trees[key].knn(q[i:i + 1], 5)
        dx, dy, dz = (q[i, 0] - pts[:, 0]).astype(F), (q[i, 1] - pts[:, 1]).astype(F), (q[i, 2] - pts[:, 2]).astype(F)
        b = np.sort(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F))[:6]
        ok[i] = True
        tie[i] = bool(np.any(np.diff(b) == 0))
        xyz[i], d2[i] = pts[idx[0], :3], d[0]
    return xyz, d2, ok, tie


def _check_window(node, ref, rng, label, first):
    """Surround, counters and tap of the device window against the restatement's after the same update."""
    info = node.window_info()
    got, want = node.get_window_surround(), ref.surround()
    for t in range(2):
        assert got[t].shape == want[t].shape and np.array_equal(bits(got[t]), bits(want[t])), (label, t)
    assert tuple(info["centre"]) == ref.centre and info["active_cubes"] == len(ref.active), label
    entered = [len(ref.entered[t]) for t in range(2)]
    trees = sum(1 for t in range(2) for g in ref.entered[t] if len(ref.cubes[t][g]) >= 5)
    stepped = sum(entered) > 0 or first
    if stepped:
        # only the entering cubes were read, one tree per entering cube with at least five points, no surviving tree rebuilt
        assert info["files_read"] == ref.files_read == sum(entered) and info["files_missing"] == 0, (label, info)
        assert tuple(info["entered"]) == tuple(entered) and tuple(info["adopted"]) == (0, 0), (label, info)
        assert info["trees_built"] == trees and (1 <= info["step_forest_builds"] <= 3 if trees else info["step_forest_builds"] == 0), (label, info)
        assert info["step_filter_runs"] == sum(1 for e in entered if e) and info["step_kernels"] <= 4, (label, info)
    assert tuple(info["resident"]) == tuple(len(ref.cubes[t]) for t in range(2)), label
    assert tuple(info["resident_with_tree"]) == tuple(sum(1 for v in ref.cubes[t].values() if len(v) >= 5) for t in range(2)), label
    if sum(info["staged"]) == 0:  # (the arena holds the staged cubes' points too)
        assert info["arena_points_used"] == sum(len(v) for t in range(2) for v in ref.cubes[t].values()), label
    tap = []
    for t, q in enumerate(_queries(ref, rng)):
        xyz, d2, how = node.debug_knn5(t, q)
        bx, bd, ok, tie = _oracle_in_cube(ref, t, q)
        assert np.array_equal(how != 0, ok), (label, t)
        assert (ok & ~tie).sum() > 0.8 * len(q), (label, t, int((ok & ~tie).sum()))
        # every answered query, the tied ones included: the oracle tree's five bit for bit, zeros where there is no tree
        assert np.array_equal(bits(d2), bits(bd)) and np.array_equal(bits(xyz), bits(bx)), (label, t)
        assert np.all(how[ok & tie] == 2), (label, t)
        tap.append((q, xyz, d2, how))
    print("%s: centre %s entered %s files %d trees %d active %d, surround %d / %d points, tap how %s; step: %d kernels %d filter runs "
          "%d forest builds %d waits %d bytes up; arena %d / %d points %d / %d nodes" %
          (label, ref.centre, entered, ref.files_read, trees, len(ref.active), len(want[0]), len(want[1]),
           [np.bincount(x[3], minlength=3).tolist() for x in tap], info["step_kernels"], info["step_filter_runs"], info["step_forest_builds"],
           info["step_host_waits"], info["bytes_uploaded"], info["arena_points_used"], info["arena_points_capacity"],
           info["arena_nodes_used"], info["arena_nodes_capacity"]))
    return tap, trees if stepped else 0


def _walk(scene):
    return [("sweep 0", _xyz(scene, 0)), ("sweep 1", _xyz(scene, 1)), ("sweep 2", _xyz(scene, 2)), ("sweep 3", _xyz(scene, 3)),
            ("y step", np.asarray((15.0, 8.0, 1.8), F)), ("diagonal x+z", np.asarray((26.0, 8.0, 6.0), F)),
            ("origin", np.asarray((0.0, 0.0, 0.0), F)), ("jump", np.asarray((-40.0, 30.0, 0.0), F)),
            ("jump past the window", np.asarray((50.0, -30.0, 0.0), F))]


def test_window_contents_step_by_step(pkg, ctx, scene, mapdir, oracle):
    """update at the four sweep positions, a y step, a diagonal step in x and z, back to the origin, a jump of four cubes and
    one of nine (no cube of the old window survives): surround, counters and tap against the restatement after each; the cubes
    are (0,0,0) (1,0,0) (1,0,0) (2,0,0) (2,1,0) (3,1,1) (0,0,0) (-4,3,0) (5,-3,0).  A fresh node opened at the diagonal step's and at the jump's position agrees with the node that
    walked there in every bit of surround and tap."""
    node, ref = _node(pkg, ctx, mapdir), _ref(oracle, mapdir)
    assert node.window_info()["paged"] == 1 and node.window_info()["files_read_total"] == 0  # nothing is read at open
    centres, trees_total = [], 0
    for n, (label, pos) in enumerate(_walk(scene)):
        node.update(pos)
        ref.update(pos)
        rng = np.random.default_rng(100 + n)
        tap, trees = _check_window(node, ref, rng, label, n == 0)
        trees_total += trees
        centres.append(ref.centre)
        assert node.window_info()["steps"] == ref.steps
        if label == "jump past the window":
            assert tuple(node.window_info()["left"]) == tuple(n_before) and sum(n_before) > 0  # everything left, nothing survived
        n_before = [len(ref.cubes[t]) for t in range(2)]
        if label in ("diagonal x+z", "jump"):
            fresh = _node(pkg, ctx, mapdir)
            fresh.update(pos)
            a, b = node.get_window_surround(), fresh.get_window_surround()
            assert all(np.array_equal(bits(a[t]), bits(b[t])) for t in range(2)), label
            for t in range(2):
                xyz, d2, how = fresh.debug_knn5(t, tap[t][0])
                assert np.array_equal(bits(xyz), bits(tap[t][1])) and np.array_equal(bits(d2), bits(tap[t][2])), (label, t)
                assert np.array_equal(how, tap[t][3]), (label, t)
            assert fresh.window_info()["files_read_total"] >= node.window_info()["files_read"]
            fresh.close()
    assert centres == [(0, 0, 0), (1, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (3, 1, 1), (0, 0, 0), (-4, 3, 0), (5, -3, 0)]
    info = node.window_info()
    assert info["steps"] == 8 and info["refused_steps"] == 0
    assert info["trees_built_total"] == trees_total  # every tree was built once, when its cube entered
    node.close()


def test_steps_bring_in_22_and_18_files(pkg, ctx, scene, mapdir):
    node = _node(pkg, ctx, mapdir)
    read = []
    for k in range(4):
        node.update(_xyz(scene, k))
        info = node.window_info()
        read.append((info["files_read"], info["steps"], tuple(info["centre"])))
    assert [r[1] for r in read] == [1, 2, 2, 3]
    assert [r[2] for r in read] == [(0, 0, 0), (1, 0, 0), (1, 0, 0), (2, 0, 0)]
    assert read[0][0] == 235 and read[1][0] == 22 and read[3][0] == 18
    assert node.window_info()["files_read_total"] == 235 + 22 + 18
    node.close()


def test_single_sweeps_match_the_restatement(pkg, ctx, synth, scene, mapdir, oracle):
    """lslam_loc_match updates the window at the Twist's translation, then prepareFeatureFrame + optimizeTransform: status,
    iterations and the three counters equal the restatement's, the pose within 1e-4 m / 1e-5 rad."""
    node, ref = _node(pkg, ctx, mapdir), _ref(oracle, mapdir)
    frame = lr.RefLocalization(oracle, pm.WINDOW, pm.CUBE, (0, 0, 0))
    for k in range(4):
        c, s = scene["sweeps"][k]
        p0 = _prior(synth, scene, k)
        ok, pr, st_r = ref.match(*frame.prepare_frame(c, s), p0)
        status, p, st = node.match(c, s, p0)
        dt, dr = np.abs(p[3:] - pr[3:]).max(), np.abs(p[:3] - pr[:3]).max()
        print("sweep %d: centre %s status %d iterations %d line %d plane %d rows %d |dt| %.2e |dr| %.2e" %
              (k, ref.centre, status, st.iterations, st.n_line, st.n_plane, st.n_rows, dt, dr))
        assert tuple(node.window_info()["centre"]) == ref.centre
        assert (status == 0) == ok
        assert (st.iterations, st.n_line, st.n_plane, st.n_rows) == (st_r.iterations, st_r.n_line, st_r.n_plane, st_r.n_rows)
        assert dt <= TOL_T and dr <= TOL_R
        assert ok and 876 <= st_r.n_rows <= 1570
    node.close()


def _drive(node, scene, ctx, between=None):
    node.handle_initial_pose(ctx.pose_to_isometry(scene["start"]))
    out = []
    for k, (c, s) in enumerate(scene["sweeps"]):
        if between is not None:
            between(k)
        odom = ctx.pose_to_isometry(np.asarray(scene["poses"][k], F))
        T = node.process(c, s, odom, 1_000_000_000 + k * 200_000_000)
        st = node.last_stats
        out.append((T, None if node.velocity is None else node.velocity.copy(), node.last_flags, node.last_status,
                    (st.iterations, st.n_line, st.n_plane, st.n_rows)))
    return out


def _assert_runs_identical(a, b, label):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(bits(x[0]), bits(y[0])), (label, k, x[0], y[0])
        assert (x[1] is None) == (y[1] is None) and (x[1] is None or np.array_equal(bits(x[1]), bits(y[1]))), (label, k)
        assert x[2:] == y[2:], (label, k, x[2:], y[2:])


@pytest.fixture(scope="module")
def ref_run(scene, mapdir, oracle):
    node = pm.RefPagedLocalization(oracle, _ref(oracle, mapdir))
    return lr.run_trajectory(node, scene, node.pose_to_isometry)


@pytest.mark.parametrize("grid", [True, False])
def test_paged_trajectory_equals_the_static_node(pkg, ctx, scene, mapdir, ref_run, grid):
    """The same files loaded whole by the static node (array 21 x 21 x 11, origin (10, 10, 5), index.txt = index2.txt + origin):
    the four-sweep trajectory through process gives the same poses, velocities, flags and counters in every bit, with the grid
    path on and off; the paged run stays within the project's bar of the restatement's."""
    paged, static = _node(pkg, ctx, mapdir, grid=grid), _static_node(pkg, ctx, mapdir, grid=grid)
    a, b = _drive(paged, scene, ctx), _drive(static, scene, ctx)
    _assert_runs_identical(a, b, "paged against static, grid %s" % grid)
    info = paged.window_info()
    assert info["steps"] == 2 and tuple(info["centre"]) == (1, 0, 0)  # the merged priors sit in cubes 0, 1, 1, 1
    cnt = paged.search_stats()
    assert (cnt["grid_proven"][1] > 0) == grid
    for k, ((T, v, flags, _, _), (Tr, vr, fr)) in enumerate(zip(a, ref_run)):
        assert flags == fr, k
        if k == 0:
            assert np.array_equal(bits(T), bits(Tr))  # the reset pose exactly
        p, pr = ctx.isometry_to_pose(T), ctx.isometry_to_pose(Tr)
        dt, dr = np.abs(T[:3, 3] - Tr[:3, 3]).max(), np.abs(p[:3] - pr[:3]).max()
        print("grid %s sweep %d: |dt| %.2e m |dr| %.2e rad" % (grid, k, dt, dr))
        assert dt <= TOL_T and dr <= TOL_R, (k, dt, dr)
        assert (v is None) == (vr is None)
        if v is not None:
            assert np.abs(v - vr).max() <= TOL_T / STEP_S, k
    paged.close()
    static.close()


def test_first_window_follows_the_merged_prior_not_the_pending_pose(pkg, ctx, scene, mapdir):
    """The quirk is kept: with an initial pose pending, the first sweep's window is centred on the merged prior."""
    node = _node(pkg, ctx, mapdir)
    far = np.eye(4, dtype=F)
    far[:3, 3] = (-40.0, 30.0, 0.0)
    node.handle_initial_pose(far)
    c, s = scene["sweeps"][0]
    T = node.process(c, s, ctx.pose_to_isometry(np.asarray(scene["poses"][0], F)), 1_000_000_000)
    assert np.array_equal(bits(T), bits(far)) and node.last_flags & 4
    assert tuple(node.window_info()["centre"]) == (0, 0, 0)
    node.close()


def test_staged_cubes_are_adopted_and_change_nothing(pkg, ctx, synth, scene, mapdir):
    """lslam_pmap_stage at the next sweep's position before sweeps 1 and 3: those steps read no file and adopt 22 / 18 cubes;
    poses, counters, surround and tap are those of the unstaged node in every bit.  The same for the process trajectory."""
    plain, staged = _node(pkg, ctx, mapdir), _node(pkg, ctx, mapdir)
    rng = np.random.default_rng(7)
    q = rng.uniform((-20, -25, 0), (40, 25, 4), (1000, 3)).astype(F)
    adopted = {}
    for k in range(4):
        c, s = scene["sweeps"][k]
        p0 = _prior(synth, scene, k)
        if k in (1, 3):
            before = staged.window_info()
            staged.stage(_xyz(scene, k))
            mid = staged.window_info()
            assert mid["steps"] == before["steps"] and tuple(mid["centre"]) == tuple(before["centre"])  # no table changed
            assert sum(mid["staged"]) == (22 if k == 1 else 18) and mid["files_read_total"] - before["files_read_total"] == sum(mid["staged"])
        ra, rb = plain.match(c, s, p0), staged.match(c, s, p0)
        assert ra[0] == rb[0] and np.array_equal(bits(ra[1]), bits(rb[1]))
        assert (ra[2].iterations, ra[2].n_line, ra[2].n_plane, ra[2].n_rows) == (rb[2].iterations, rb[2].n_line, rb[2].n_plane, rb[2].n_rows)
        ia, ib = plain.window_info(), staged.window_info()
        if k in (1, 3):
            assert ib["files_read"] == 0 and sum(ib["adopted"]) == sum(ia["entered"]) == ia["files_read"] == (22 if k == 1 else 18)
            assert ib["trees_built"] == 0 and sum(ib["staged"]) == 0
            adopted[k] = sum(ib["adopted"])
        assert tuple(ia["resident"]) == tuple(ib["resident"]) and tuple(ia["centre"]) == tuple(ib["centre"])
        sa, sb = plain.get_window_surround(), staged.get_window_surround()
        assert all(np.array_equal(bits(sa[t]), bits(sb[t])) for t in range(2))
        for t in range(2):
            xa, xb = plain.debug_knn5(t, q), staged.debug_knn5(t, q)
            assert all(np.array_equal(xa[i].view(np.uint8), xb[i].view(np.uint8)) for i in range(3)), (k, t)
    assert adopted == {1: 22, 3: 18}
    plain.close()
    staged.close()
    plain, staged = _node(pkg, ctx, mapdir), _node(pkg, ctx, mapdir)
    a = _drive(plain, scene, ctx)
    b = _drive(staged, scene, ctx, between=lambda k: staged.stage(_xyz(scene, k)))
    _assert_runs_identical(a, b, "staged against unstaged")
    assert sum(staged.window_info()["adopted_total"]) >= 22 and sum(plain.window_info()["adopted_total"]) == 0
    plain.close()
    staged.close()


def test_unreached_staged_cubes_are_dropped_when_room_is_needed(pkg, ctx, scene, mapdir, oracle):
    """A staged set far from the drive is never adopted; under a capacity that holds the window and its step but not the staged
    cubes too, the step drops them and nothing observable changes."""
    node, ref = _node(pkg, ctx, mapdir), _ref(oracle, mapdir)
    node.update(_xyz(scene, 0))
    ref.update(_xyz(scene, 0))
    room = node.window_info()["arena_points_capacity"]
    node.stage(np.asarray((-40.0, 30.0, 0.0), F))
    node.stage(np.asarray((-40.0, -30.0, 0.0), F))
    staged = node.window_info()["staged"]
    assert sum(staged) > 0
    # the stagings outgrew the arena: it moved with the window live, and the window answers as before
    assert node.window_info()["arena_points_capacity"] > room
    _check_window(node, ref, np.random.default_rng(6), "after staging", False)
    held = [sum(len(v) for v in ref.cubes[t].values()) for t in range(2)]
    ref.update(_xyz(scene, 1))
    new = [sum(len(ref.cubes[t][g]) for g in ref.entered[t]) for t in range(2)]
    node.setup_paged_capacity(max(held[t] + new[t] for t in range(2)) + 8)
    node.update(_xyz(scene, 1))
    info = node.window_info()
    assert sum(info["staged"]) == 0 and sum(info["staged_dropped_total"]) == sum(staged) and sum(info["adopted"]) == 0
    assert info["files_read"] == 22 and info["refused_steps"] == 0
    _check_window(node, ref, np.random.default_rng(3), "after the drop", False)
    node.close()


def test_a_refused_step_leaves_the_node_as_it_was(pkg, ctx, synth, scene, mapdir, oracle):
    """A capacity too small for the step of sweep 1: the step is refused (LSLAM_ERR_INVALID), the window, its counters, the
    surround and the tap are as before, and sweep 0 repeats bit for bit; with the capacity lifted the step goes through."""
    node, ref = _node(pkg, ctx, mapdir), _ref(oracle, mapdir)
    c0, s0 = scene["sweeps"][0]
    p0 = _prior(synth, scene, 0)
    first = node.match(c0, s0, p0)
    ref.update(p0[3:])
    held = [sum(len(v) for v in ref.cubes[t].values()) for t in range(2)]
    before = node.window_info()
    sur = node.get_window_surround()
    q = np.random.default_rng(11).uniform((-20, -25, 0), (30, 25, 4), (1000, 3)).astype(F)
    tap = [node.debug_knn5(t, q) for t in range(2)]
    node.setup_paged_capacity(max(held))
    with pytest.raises(pkg.LslamError) as e:
        node.match(*scene["sweeps"][1], _prior(synth, scene, 1))
    assert e.value.code == pkg.Status.ERR_INVALID and "capacity" in str(e.value)
    with pytest.raises(pkg.LslamError):
        node.update(_xyz(scene, 1))
    after = node.window_info()
    assert after["refused_steps"] == 2 and after["steps"] == before["steps"] == 1 and tuple(after["centre"]) == (0, 0, 0)
    for f in ("resident", "resident_with_tree", "arena_points_used", "arena_nodes_used", "files_read_total", "trees_built_total"):
        assert after[f] == before[f], f
    again = node.match(c0, s0, p0)
    assert again[0] == first[0] and np.array_equal(bits(again[1]), bits(first[1])) and again[2].n_rows == first[2].n_rows
    sur2 = node.get_window_surround()
    assert all(np.array_equal(bits(sur[t]), bits(sur2[t])) for t in range(2))
    for t in range(2):
        x = node.debug_knn5(t, q)
        assert all(np.array_equal(x[i].view(np.uint8), tap[t][i].view(np.uint8)) for i in range(3))
    node.setup_paged_capacity(0)
    node.update(_xyz(scene, 1))
    ref.update(_xyz(scene, 1))
    _check_window(node, ref, np.random.default_rng(12), "after the capacity was lifted", False)
    node.close()


def test_refusals_at_open(pkg, ctx, scene, mapdir, oracle, tmp_path):
    """An even window dimension, an active area wider than the half window and a missing index2.txt are refused; a node that
    was open keeps its window through a refused open."""
    for dims in ((8, 9, 5), (9, 9, 4)):
        with pytest.raises(pkg.LslamError) as e:
            _node(pkg, ctx, mapdir, dims=dims)
        assert e.value.code == pkg.Status.ERR_INVALID and "even" in str(e.value)
    with pytest.raises(pkg.LslamError) as e:
        _node(pkg, ctx, mapdir, valid=20.5)  # ws = 3 > 5 / 2
    assert e.value.code == pkg.Status.ERR_INVALID and "window" in str(e.value)
    with pytest.raises(pkg.LslamError) as e:
        _node(pkg, ctx, str(tmp_path))
    assert e.value.code == pkg.Status.ERR_INVALID and "index2.txt" in str(e.value)
    node, ref = _node(pkg, ctx, mapdir), _ref(oracle, mapdir)
    node.update(_xyz(scene, 0))
    ref.update(_xyz(scene, 0))
    with pytest.raises(pkg.LslamError):
        node.setup_files_directory(str(tmp_path))
    with pytest.raises(pkg.LslamError):
        node._check(node.lib.lslam_loc_setup_lidar_valid_distance(node.h, 30.0))
    _check_window(node, ref, np.random.default_rng(2), "after refused opens", False)
    node.close()
    static = _static_node(pkg, ctx, mapdir)
    with pytest.raises(pkg.LslamError) as e:
        static.update(_xyz(scene, 0))
    assert "not in the paged mode" in str(e.value)
    static.close()


def test_a_listed_but_missing_file_leaves_its_cube_empty(pkg, ctx, synth, scene, mapdir, oracle, tmp_path):
    d = str(tmp_path / "holes")
    shutil.copytree(mapdir, d)
    index = pm.parse_index(os.path.join(d, "index2.txt"))
    os.remove(os.path.join(d, "%d.pcd" % index[1][(0, 0, 0)]))
    with open(os.path.join(d, "%d.pcd" % index[0][(1, 0, 0)]), "wb") as f:
        f.write(b"not a point cloud\n")
    node, ref = _node(pkg, ctx, d), _ref(oracle, d)
    frame = lr.RefLocalization(oracle, pm.WINDOW, pm.CUBE, (0, 0, 0))
    c, s = scene["sweeps"][0]
    p0 = _prior(synth, scene, 0)
    status, p, st = node.match(c, s, p0)
    os.remove(os.path.join(d, "%d.pcd" % index[0][(1, 0, 0)]))  # (the restatement knows only "missing", not "unreadable")
    ok, pr, st_r = ref.match(*frame.prepare_frame(c, s), p0)
    info = node.window_info()
    assert info["files_missing"] == 2 and ref.files_missing == 2 and info["files_read"] == ref.files_read
    assert tuple(info["resident"]) == tuple(len(ref.cubes[t]) for t in range(2))  # listed: resident, and empty
    assert (status == 0) == ok and (st.iterations, st.n_rows) == (st_r.iterations, st_r.n_rows)
    assert np.abs(p[3:] - pr[3:]).max() <= TOL_T and np.abs(p[:3] - pr[:3]).max() <= TOL_R
    got, want = node.get_window_surround(), ref.surround()
    assert all(np.array_equal(bits(got[t]), bits(want[t])) for t in range(2))
    node.close()


def test_index_rules_on_the_device(pkg, ctx, oracle, tmp_path):
    """A later line wins, a type other than 0 / 1 is surf, negative indices are cubes like any other."""
    rng = np.random.default_rng(1)
    d = str(tmp_path)

    def cloud(centre, n):
        return np.concatenate([(np.asarray(centre) * pm.CUBE + rng.uniform(-4, 4, (n, 3))), np.zeros((n, 1))], 1).astype(F)
    files = [cloud((0, 0, 0), 50), cloud((0, 0, 0), 80), cloud((-1, -2, 0), 60), cloud((0, 0, 0), 70), cloud((1, 0, 0), 3)]
    for n, pts in enumerate(files):
        pm.write_pcd(os.path.join(d, "%d.pcd" % n), pts)
    with open(os.path.join(d, "index2.txt"), "w") as f:
        f.write("0 0 0 0 0 50\n1 7 0 0 0 80\n2 0 -1 -2 0 60\n3 0 0 0 0 70\n4 1 1 0 0 3\n")
    node, ref = _node(pkg, ctx, d), _ref(oracle, d)
    assert ref.index[0] == {(0, 0, 0): 3, (-1, -2, 0): 2} and ref.index[1] == {(0, 0, 0): 1, (1, 0, 0): 4}
    pos = np.asarray((1.0, -1.0, 0.5), F)
    node.update(pos)
    ref.update(pos)
    info = node.window_info()
    assert info["files_read"] == 4 and tuple(info["resident"]) == (2, 2) and tuple(info["resident_with_tree"]) == (2, 1)
    got, want = node.get_window_surround(), ref.surround()
    assert all(np.array_equal(bits(got[t]), bits(want[t])) for t in range(2)) and len(want[0]) and len(want[1])
    node.close()


def test_python_dynamic_feature_map_mirror(pkg, ctx, synth, scene, mapdir, oracle):
    """dynamic_feature_map.DynamicFeatureMap with the scene's settings: update / get_surround_feature / scan_match_scan give the
    restatement's results; its defaults are the reference's 21 x 11 x 21."""
    m = pkg.DynamicFeatureMap(ctx)
    m.setup_files_directory(mapdir)
    assert tuple(m.window_info()["dims"]) == (21, 11, 21) and m.window_info()["paged"] == 1
    m.close()
    m = pkg.DynamicFeatureMap(ctx, *pm.WINDOW)
    m.setup_filter_size(*pm.LEAVES)
    m.setup_world_cube_size(pm.CUBE)
    m.setup_lidar_valid_distance(pm.VALID)
    m.setup_lidar_fov(20.0, 20.0)
    m.setup_files_directory(mapdir)
    with pytest.raises(ValueError):
        m.setup_world_cube_size(20.0)
    ref = _ref(oracle, mapdir)
    frame = lr.RefLocalization(oracle, pm.WINDOW, pm.CUBE, (0, 0, 0))
    m.update(_xyz(scene, 1), (0.0, 0.0, 1.0))
    ref.update(_xyz(scene, 1))
    got, want = m.get_surround_feature(), ref.surround()
    assert all(np.array_equal(bits(got[t]), bits(want[t])) for t in range(2))
    m.stage(_xyz(scene, 3))
    c, s = scene["sweeps"][3]
    p0 = _prior(synth, scene, 3)
    ok_r, pr, st_r = ref.match(*frame.prepare_frame(c, s), p0)
    ok, p, st = m.scan_match_scan(c, s, p0)
    assert ok == ok_r and (st.iterations, st.n_rows) == (st_r.iterations, st_r.n_rows)
    assert np.abs(p[3:] - pr[3:]).max() <= TOL_T and np.abs(p[:3] - pr[:3]).max() <= TOL_R
    info = m.window_info()
    assert info["files_read"] == 0 and sum(info["adopted"]) == sum(info["entered"]) > 0
    m.close()


def test_destroy_with_a_steps_buffers_live_then_create_again(pkg, ctx, scene, mapdir, oracle):
    """The arena, the staging buffer and the staged cubes belong to the node: destroyed with all of them live, a new node
    starts from nothing and gives the same window; a node switched back to a static map and paged again does too."""
    node = _node(pkg, ctx, mapdir)
    node.update(_xyz(scene, 0))
    node.stage(_xyz(scene, 3))
    assert node.window_info()["arena_points_used"] > 0 and sum(node.window_info()["staged"]) > 0
    node.close()
    node.close()
    node, ref = _node(pkg, ctx, mapdir), _ref(oracle, mapdir)
    info = node.window_info()
    assert info["have_window"] == 0 and info["arena_points_used"] == 0 and info["files_read_total"] == 0
    node.update(_xyz(scene, 3))
    ref.update(_xyz(scene, 3))
    _check_window(node, ref, np.random.default_rng(4), "second node", True)
    node.set_map(scene["map_corner"][:2000], scene["map_surf"][:2000])  # the static mode takes the arenas' memory
    assert node.window_info()["paged"] == 0
    node.setup_files_directory(mapdir)
    ref = _ref(oracle, mapdir)
    node.update(_xyz(scene, 1))
    ref.update(_xyz(scene, 1))
    _check_window(node, ref, np.random.default_rng(5), "paged again", True)
    node.close()


def test_cpp_paged_localization_equals_the_abi_run(pkg, ctx, synth, scene, tmp_path):
    """tests/cpp/paged_localization_end_to_end.cpp -- LaserLocalization::setDynamicMode / setupFilesDirectory and DynamicFeatureMap in
    C++ -- over a map saved by lslam_fmap_save and converted by convertIndexFile: the same ABI calls as the Python mirrors, so the
    same flags, counters, window centres, poses and velocities, bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "paged_localization_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "paged_localization_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    fm = pkg.FeatureMap(ctx, *pm.STATIC_DIMS)
    fm.setup_world_cube_size(pm.CUBE)
    fm.setup_world_origin(*pm.STATIC_ORIGIN)
    fm.add_feature_cloud(scene["map_corner"], scene["map_surf"], np.eye(4, dtype=F))  # no active area: nothing is filtered
    d = tmp_path / "map"
    d.mkdir()
    fm.save_cloud_to_files(str(d))
    fm.close()
    assert not (d / "index2.txt").exists()
    with open(tmp_path / "session.bin", "wb") as fo:
        fo.write(np.ascontiguousarray(ctx.pose_to_isometry(scene["start"]), F).tobytes())
        for k, (c, s) in enumerate(scene["sweeps"]):
            fo.write(struct.pack("<q", 1_000_000_000 + k * 200_000_000))
            fo.write(np.ascontiguousarray(ctx.pose_to_isometry(np.asarray(scene["poses"][k], F)), F).tobytes())
            for cloud in (c, s):
                cloud = np.ascontiguousarray(cloud, F)[:, :4]
                fo.write(struct.pack("<I", len(cloud)))
                fo.write(np.ascontiguousarray(cloud).tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "session.bin"), str(d)] + [str(v) for v in pm.STATIC_ORIGIN + pm.WINDOW] +
                         [str(pm.CUBE), str(pm.VALID)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    index = pm.parse_index(d / "index2.txt")
    assert (len(index[0]), len(index[1])) == (133, 297) and min(k[0] for k in index[1]) == -6
    lines = [l.split() for l in out.stdout.splitlines()]
    sweeps = [l for l in lines if l and l[0] == "SWEEP"]
    assert len(sweeps) == 4 and ["OK", "sweeps", "4"] in lines
    node = _node(pkg, ctx, str(d))
    run = _drive(node, scene, ctx)
    files_total = 0
    for k, (w, (T, v, flags, status, counters)) in enumerate(zip(sweeps, run)):
        got = [int(x) for x in w[1:12]]
        assert got[:2] == [k, flags] and got[2] == status and tuple(got[3:7]) == counters, (k, got)
        vals = np.asarray([float.fromhex(x) for x in w[12:]], F)
        assert np.array_equal(bits(vals[:16]), bits(T.reshape(16))), k
        if v is not None:
            assert np.array_equal(bits(vals[16:19]), bits(v)), k
        files_total = got[10]
    assert files_total == node.window_info()["files_read_total"] == 235 + 22
    node.close()
    m = pkg.DynamicFeatureMap(ctx, *pm.WINDOW)
    m.setup_filter_size(1.0, 1.0, 0.6)
    m.setup_world_cube_size(pm.CUBE)
    m.setup_lidar_valid_distance(pm.VALID)
    m.setup_files_directory(str(d))
    first = _xyz(scene, 0)
    m.update(first)
    sc, ss = m.get_surround_feature()
    ok, p, st = m.scan_match_scan(*scene["sweeps"][0], np.asarray((0.0, 0.0, 0.3) + tuple(first), F))
    w = [l for l in lines if l and l[0] == "MAP"][0]
    assert [int(x) for x in w[1:7]] == [len(sc), len(ss), int(ok), st.n_line, st.n_plane, st.iterations]
    assert np.array_equal(bits(np.asarray([float.fromhex(x) for x in w[7:13]], F)), bits(p))
    assert len(sc) > 0 and len(ss) > 0 and st.n_rows > 500
    m.close()
