"""The localisation node on the device (lslam_loc_*, csrc/lslam_loc.hip) against its restatement (tests/localization_ref.py,
composed from the CPU oracle) on the scene of tests/test_localization_ref.py: the search's neighbours bit for bit against an
in-cube brute force, single sweeps against ``oracle.scanmatch_cubes``, whole trajectories from the three kinds of map input,
independence of the search path, residency of the structures, and the edge cases."""
import os
import struct
import subprocess

import numpy as np
import pytest

import localization_ref as lr

pytestmark = pytest.mark.gpu

TOL_T, TOL_R = 1e-4, 1e-5  # the project's pose tolerances (test_cube_map_variant_matches_oracle)
STEP_S = 0.2
NEXT_CUBE_POSE = (0.01, -0.015, 0.5, 27.0, 4.0, 1.8)  # round(27 / 50) = 1: the sensor has crossed into the next cube


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(synth):
    return lr.make_scene(synth, extra_poses=[NEXT_CUBE_POSE])


@pytest.fixture(scope="module")
def refs(scene, oracle):
    """The restatement's run over the scene for both maps: 'raw' (the map as it is) and 'filtered' (1.0 m per-cube filter)."""
    out = {}
    for name, filt in (("raw", False), ("filtered", True)):
        ref = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
        ref.set_map(scene["map_corner"], scene["map_surf"], filter=filt)
        stats = []
        ref.handle_initial_pose(ref.pose_to_isometry(scene["start"]))
        run = []
        for k, (c, s) in enumerate(scene["sweeps"]):
            odom = ref.pose_to_isometry(np.asarray(scene["poses"][k], np.float32))
            T, flags = ref.process(c, s, odom, 1_000_000_000 + k * 200_000_000)
            run.append((T, None if ref.velocity is None else ref.velocity.copy(), flags))
            stats.append(ref.last)
        out[name] = dict(ref=ref, run=run, stats=stats)
    return out


def _node(pkg, ctx, scene=None, filt=False):
    node = pkg.LaserLocalization(ctx, *lr.DIMS)
    if scene is not None:
        node.set_map(scene["map_corner"], scene["map_surf"], filter=filt)
    return node


def _drive(node, scene, ctx, sweeps=None, between=None):
    node.handle_initial_pose(ctx.pose_to_isometry(scene["start"]))
    out = []
    for k, (c, s) in enumerate(scene["sweeps"] if sweeps is None else sweeps):
        if between is not None:
            between(k)
        odom = ctx.pose_to_isometry(np.asarray(scene["poses"][k], np.float32))
        T = node.process(c, s, odom, 1_000_000_000 + k * 200_000_000)
        out.append((T, None if node.velocity is None else node.velocity.copy(), node.last_flags, node.last_stats))
    return out


def _assert_run_close(ctx, got, want, label):
    for k, ((T, v, flags, _), (Tr, vr, fr)) in enumerate(zip(got, want)):
        assert flags == fr, (label, k, flags, fr)
        if k == 0:
            assert np.array_equal(bits(T), bits(Tr)), label  # the reset pose exactly
        p, pr = ctx.isometry_to_pose(T), ctx.isometry_to_pose(Tr)
        dt, dr = np.abs(T[:3, 3] - Tr[:3, 3]).max(), np.abs(p[:3] - pr[:3]).max()
        print("%s sweep %d: |dt| %.2e m |dr| %.2e rad" % (label, k, dt, dr))
        assert dt <= TOL_T and dr <= TOL_R, (label, k, dt, dr)
        assert (v is None) == (vr is None)
        if v is not None:
            assert np.abs(v - vr).max() <= TOL_T / STEP_S, (label, k)


def _brute_in_cube(ref, t, q):
    """Five nearest of every query inside its own cube: fp32, accumulated x -> y -> z as L2_Simple.  -> xyz, d2, ok, tie"""
    F = np.float32
    nq = len(q)
    xyz, d2 = np.zeros((nq, 5, 3), F), np.zeros((nq, 5), F)
    ok, tie = np.zeros(nq, bool), np.zeros(nq, bool)
    ijk = lr.cube_index(q, ref.cube_size, ref.origin)
    for i in range(nq):
        if not all(0 <= v < d for v, d in zip(ijk[i], ref.dims)):
            continue
        pts = ref.cubes[t].get(ref._to_index(ijk[i]))
        if pts is None or len(pts) < 5:
            continue
        dx, dy, dz = (q[i, 0] - pts[:, 0]).astype(F), (q[i, 1] - pts[:, 1]).astype(F), (q[i, 2] - pts[:, 2]).astype(F)
        d = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)
        order = np.argsort(d, kind="stable")[:6]
        ok[i] = True
        tie[i] = bool(np.any(np.diff(d[order]) == 0))
        xyz[i], d2[i] = pts[order[:5], :3], d[order[:5]]
    return xyz, d2, ok, tie


def _brute_global_d2(cloud, q):
    F = np.float32
    out = np.zeros((len(q), 5), F)
    for i in range(len(q)):
        dx, dy, dz = (q[i, 0] - cloud[:, 0]).astype(F), (q[i, 1] - cloud[:, 1]).astype(F), (q[i, 2] - cloud[:, 2]).astype(F)
        d = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)
        out[i] = np.sort(d[np.argpartition(d, 5)[:6]])[:5]
    return out


@pytest.mark.parametrize("name", ["raw", "filtered"])
def test_neighbours_equal_the_in_cube_brute_force(pkg, ctx, scene, refs, name):
    """The tap (the kernels the loop runs) at the restatement's final pose of sweep 3: coordinates and d2 of the five, bit for
    bit, for EVERY downsampled point; no tie among six; both paths used; every border point decided by its cube's tree."""
    ref = refs[name]["ref"]
    node = _node(pkg, ctx, scene, filt=(name == "filtered"))
    T = refs[name]["run"][3][0]
    c, s = ref.prepare_frame(*scene["sweeps"][3])
    used = set()
    for t, cloud in ((0, c), (1, s)):
        q = (cloud[:, :3] @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        xyz, d2, how = node.debug_knn5(t, q)
        bx, bd, ok, tie = _brute_in_cube(ref, t, q)
        assert not tie.any()
        assert np.array_equal(how != 0, ok)
        assert np.array_equal(bits(d2[ok]), bits(bd[ok])) and np.array_equal(bits(xyz[ok]), bits(bx[ok]))
        gd = _brute_global_d2(ref.map[t], q)
        border = ok & np.any(bits(gd) != bits(bd), axis=1)
        print("%s type %d: %d queries, %d by the grid, %d by cube trees, %d border points" %
              (name, t, len(q), int((how == 1).sum()), int((how == 2).sum()), int(border.sum())))
        assert np.all(how[border] == 2)
        assert int((how == 2).sum()) >= int(border.sum())
        if t == 1:
            assert border.sum() > 0  # the scene exercises the border case
        used |= set(how.tolist())
    assert {1, 2} <= used
    node.close()


@pytest.mark.parametrize("name", ["raw", "filtered"])
def test_single_sweep_matches_the_oracle(pkg, ctx, synth, scene, refs, name):
    """prepareFeatureFrame + optimizeTransform from a given pose: status, iterations and the three counters equal
    oracle.scanmatch_cubes's, the pose within 1e-4 m / 1e-5 rad -- the sweeps that run out of iterations included."""
    ref = refs[name]["ref"]
    node = _node(pkg, ctx, scene, filt=(name == "filtered"))
    exhausted = 0
    for k in range(4):
        c, s = scene["sweeps"][k]
        p0 = synth.perturb_pose(scene["poses"][k], seed=99 + k, dt=0.2, dr_deg=1.0)
        ok, pr, st_r = ref.match(c, s, p0)
        status, p, st = node.match(c, s, p0)
        print("%s sweep %d: status %d iterations %d line %d plane %d rows %d |dt| %.2e |dr| %.2e" %
              (name, k, status, st.iterations, st.n_line, st.n_plane, st.n_rows, np.abs(p[3:] - pr[3:]).max(), np.abs(p[:3] - pr[:3]).max()))
        assert (status == 0) == ok
        assert (st.iterations, st.n_line, st.n_plane, st.n_rows) == (st_r.iterations, st_r.n_line, st_r.n_plane, st_r.n_rows)
        assert np.abs(p[3:] - pr[3:]).max() <= TOL_T and np.abs(p[:3] - pr[:3]).max() <= TOL_R
        exhausted += int(st.iterations == 10 and status != 0)
    if name == "raw":
        assert exhausted > 0  # one sweep on the unfiltered map uses all ten iterations without meeting the thresholds
    node.close()


def test_single_sweep_at_a_tilted_pose_matches_the_oracle(pkg, ctx, synth, scene, refs):
    """The body of test_single_sweep_matches_the_oracle at roll 0.9, pitch -0.7, yaw 2.4 rad: loc_fit_kernel shares
    jacobian_row and block_accumulate with the sweep kernels, and every other frame of this file has roll, pitch ~ 0.01.
    The sweep is re-expressed for the tilted pose (scanmatch_ref.reexpress), so its points land where they did."""
    import scanmatch_ref
    ref = refs["filtered"]["ref"]
    node = _node(pkg, ctx, scene, filt=True)
    c, s = scene["sweeps"][0]
    p0 = synth.perturb_pose(scene["poses"][0], seed=99, dt=0.2, dr_deg=1.0)
    pn = p0.copy()
    pn[:3] = (0.9, -0.7, 2.4)
    c, s = scanmatch_ref.reexpress(c, p0, pn), scanmatch_ref.reexpress(s, p0, pn)
    ok, pr, st_r = ref.match(c, s, pn)
    status, p, st = node.match(c, s, pn)
    print("tilted: status %d iterations %d line %d plane %d rows %d |dt| %.2e |dr| %.2e" %
          (status, st.iterations, st.n_line, st.n_plane, st.n_rows, np.abs(p[3:] - pr[3:]).max(), np.abs(p[:3] - pr[:3]).max()))
    assert st_r.n_rows > 500 and st_r.iterations >= 2
    assert (status == 0) == ok
    assert (st.iterations, st.n_line, st.n_plane, st.n_rows) == (st_r.iterations, st_r.n_line, st_r.n_plane, st_r.n_rows)
    assert np.abs(p[3:] - pr[3:]).max() <= TOL_T and np.abs(p[:3] - pr[:3]).max() <= TOL_R
    node.close()


def test_trajectory_from_the_three_map_inputs(pkg, ctx, scene, refs, oracle, tmp_path):
    """Host clouds (raw and filtered), a directory written by lslam_fmap_save (filtered at load), and a map adopted from an
    lslam_fmap: every sweep's pose within the tolerances of the restatement's run, velocity to tolerance / dt, the reset sweep
    exactly."""
    four = scene["sweeps"][:4]
    for name in ("raw", "filtered"):
        node = _node(pkg, ctx, scene, filt=(name == "filtered"))
        _assert_run_close(ctx, _drive(node, scene, ctx, four), refs[name]["run"], "host clouds, " + name)
        node.close()
    fm = pkg.FeatureMap(ctx, *lr.DIMS)
    fm.add_feature_cloud(scene["map_corner"], scene["map_surf"], np.eye(4, dtype=np.float32))  # no active area: nothing filtered
    d = tmp_path / "map"
    d.mkdir()
    fm.save_cloud_to_files(str(d))
    # the saved map as the restatement reads it
    for label, filt in (("adopted", False), ("loaded", True)):
        ref = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
        ref.load_map(str(d), filter=filt)
        want = lr.run_trajectory(ref, dict(scene, sweeps=four), ref.pose_to_isometry)
        node = _node(pkg, ctx)
        if filt:
            node.load_map(d)
        else:
            node.set_map_from(fm)
        info = node.info()
        assert info["n_points"] == (len(ref.map[0]), len(ref.map[1])), label
        assert info["cubes_loaded"] == (len(ref.cubes[0]), len(ref.cubes[1]))
        assert info["cubes_with_tree"] == tuple(sum(len(v) >= 5 for v in ref.cubes[t].values()) for t in range(2))
        _assert_run_close(ctx, _drive(node, scene, ctx, four), want, label)
        node.close()
    fm.close()


def test_poses_do_not_depend_on_the_search_path(pkg, ctx, scene):
    runs = []
    for use_grid in (True, False):
        node = _node(pkg, ctx, scene, filt=True)
        node.set_search(use_grid)
        runs.append(_drive(node, scene, ctx))
        st = node.search_stats()
        print("grid %s: swept %d, proven by the grid %d, refused by the cube check %d, to trees %d" %
              (use_grid, st["swept"][1], st["grid_proven"][1], st["cube_refused"][1], st["to_trees"][1]))
        if use_grid:
            assert st["grid_proven"][1] > st["to_trees"][1] > 0 and st["cube_refused"][1] > 0
        else:
            assert st["grid_proven"][1] == 0 and st["to_trees"][1] > 0
        node.close()
    for (T, v, f, _), (T2, v2, f2, _) in zip(*runs):
        assert f == f2 and np.array_equal(bits(T), bits(T2))
        assert (v is None and v2 is None) or np.array_equal(bits(v), bits(v2))


def test_structures_are_built_once_and_survive_a_map_set(pkg, ctx, scene, small_problem, oracle):
    """The forest is built at the map set and never again; the grids once per sensor cube (they move when the fifth sweep
    crosses into the next cube); one host wait per sweep; a lslam_map_set on the context between two sweeps changes nothing,
    and the context's own scan match still agrees with the oracle afterwards."""
    node = _node(pkg, ctx, scene, filt=True)
    assert node.info()["structure_builds"] == 1 and node.info()["grid_builds"] == 0
    node.handle_initial_pose(ctx.pose_to_isometry(scene["start"]))
    seen = []
    for k, (c, s) in enumerate(scene["sweeps"]):
        node.process(c, s, ctx.pose_to_isometry(np.asarray(scene["poses"][k], np.float32)), 1_000_000_000 + k * 200_000_000)
        i = node.info()
        seen.append((i["structure_builds"], i["grid_builds"], i["grid_cube"]))
        assert node.search_stats()["host_waits"][0] == 1
    assert [x[:2] for x in seen] == [(1, 1)] * 4 + [(1, 2)]
    assert seen[0][2] == (60, 60, 5) and seen[4][2] == (61, 60, 5)
    node.close()
    pr = small_problem
    node = _node(pkg, ctx, scene, filt=True)
    plain = _drive(node, scene, ctx)
    node.close()
    node = _node(pkg, ctx, scene, filt=True)
    disturbed = _drive(node, scene, ctx, between=lambda k: ctx.map_set(pr["map_corner"], pr["map_surf"]))
    for (T, v, f, _), (T2, v2, f2, _) in zip(plain, disturbed):
        assert f == f2 and np.array_equal(bits(T), bits(T2))
    status, pose, st = ctx.scanmatch_full(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"], pr["init_pose"])
    ok, opose, ost = oracle.scanmatch_scan(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"], pr["init_pose"])
    assert (status == 0) == ok and st.iterations == ost.iterations and st.n_rows == ost.n_rows
    assert np.abs(pose[3:] - opose[3:]).max() <= TOL_T and np.abs(pose[:3] - opose[:3]).max() <= TOL_R
    node.close()


def test_load_edge_cases(pkg, ctx, scene, oracle, tmp_path):
    """A cube file listed twice (the later entry wins) and a missing PCD (skipped)."""
    fm = pkg.FeatureMap(ctx, *lr.DIMS)
    fm.add_feature_cloud(scene["map_corner"], scene["map_surf"], np.eye(4, dtype=np.float32))
    d = tmp_path / "map"
    d.mkdir()
    fm.save_cloud_to_files(str(d))
    fm.close()
    lines = open(d / "index.txt").read().splitlines()
    first = lines[0].split()
    # a decoy for the first cube, listed BEFORE the real entry; and an entry whose file does not exist
    decoy = np.zeros((7, 4), np.float32)
    decoy[:, 0] = np.arange(7)
    with open(d / "9000.pcd", "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
                 "COUNT 1 1 1 1\nWIDTH 7\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 7\nDATA binary\n").encode())
        f.write(decoy.tobytes())
    with open(d / "index.txt", "w") as f:
        f.write("9000 %s 7\n" % " ".join(first[1:5]))
        f.write("9001 1 60 60 5 12\n")
        f.write("\n".join(lines) + "\n")
    ref = lr.RefLocalization(oracle, lr.DIMS, lr.CUBE, lr.ORIGIN)
    ref.load_map(str(d))
    node = _node(pkg, ctx)
    node.load_map(d)
    info = node.info()
    assert info["n_points"] == (len(ref.map[0]), len(ref.map[1])) == (1481, 41611)
    c, s = scene["sweeps"][1]
    ok, pr, st_r = ref.match(c, s, scene["start"])
    status, p, st = node.match(c, s, scene["start"])
    assert (st.iterations, st.n_rows) == (st_r.iterations, st_r.n_rows)
    assert np.abs(p[3:] - pr[3:]).max() <= TOL_T and np.abs(p[:3] - pr[:3]).max() <= TOL_R
    node.close()


def test_sweep_edge_cases(pkg, ctx, scene, refs):
    import torch
    empty = np.zeros((0, 4), np.float32)
    I = np.eye(4, dtype=np.float32)
    # a sweep before the initial pose: dropped, nothing changes
    node = _node(pkg, ctx, scene, filt=True)
    c, s = scene["sweeps"][0]
    assert node.process(c, s, I, 1_000_000_000) is None and node.last_flags == 1
    assert node.info()["grid_builds"] == 0 and node.search_stats()["swept"][1] == 0
    # ... after which the trajectory is the one of a fresh node
    want = refs["filtered"]["run"]
    _assert_run_close(ctx, _drive(node, scene, ctx, scene["sweeps"][:4]), want, "after a dropped sweep")
    # empty clouds: the loop ends at its first row count, the pose is the prior
    T_before = node.lidar_mapped.copy()
    odom = ctx.pose_to_isometry(np.asarray(scene["poses"][3], np.float32))
    T = node.process(empty, empty, odom, 3_000_000_000)
    assert node.last_status == pkg.Status.TOO_FEW_MATCHES and node.last_stats.n_rows == 0
    assert np.abs(T - T_before).max() < 1e-5
    # a sensor within 3 cubes of the grid's edge: refused, state intact
    far = I.copy()
    far[0, 3] = 50.0 * 58  # cube 118 of 121
    node.handle_initial_pose(far)
    node.process(c, s, odom, 3_200_000_000)  # the prior is still in the middle: matched, then reset to the edge
    assert np.array_equal(node.lidar_mapped, far) and node.last_flags & 4
    before = (node.info(), node.search_stats())
    with pytest.raises(pkg.LslamError) as e:
        node.process(c, s, odom, 3_400_000_000)  # the prior is now at the edge: refused
    assert e.value.code == pkg.Status.ERR_INVALID and "within 3 cubes" in str(e.value)
    assert (node.info(), node.search_stats()) == before
    back = want[3][0]
    node.handle_initial_pose(back)
    T = node.process(c, s, odom, 3_600_000_000)  # a pending pose brings the node back: nothing to match, the pose is taken
    assert np.array_equal(T, back) and node.last_flags & 4 and node.last_stats.n_rows == 0
    node.close()
    # a map with a type absent
    node = _node(pkg, ctx)
    node.set_map(empty, scene["map_surf"], filter=True)
    assert node.info()["n_points"][0] == 0 and node.info()["cubes_with_tree"][0] == 0
    status, p, st = node.match(c, s, scene["start"])
    assert st.n_line == 0 and st.n_plane > 0
    node.close()
    # a device-pointer sweep equals the host-pointer sweep bit for bit
    runs = []
    for dev in (False, True):
        node = _node(pkg, ctx, scene, filt=True)
        sweeps = scene["sweeps"][:3]
        if dev:
            sweeps = [(torch.from_numpy(np.ascontiguousarray(a[:, :4])).cuda(), torch.from_numpy(np.ascontiguousarray(b[:, :4])).cuda())
                      for a, b in sweeps]
        runs.append(_drive(node, scene, ctx, sweeps))
        node.close()
    for (T1, v1, f1, st1), (T2, v2, f2, st2) in zip(*runs):
        assert f1 == f2 and np.array_equal(bits(T1), bits(T2)) and st1.n_rows == st2.n_rows


def test_destroy_orders(pkg, scene):
    """The context destroyed before the node, and the node before the context."""
    for ctx_first in (True, False):
        c = pkg.Context(0)
        node = _node(pkg, c, scene, filt=True)
        status, p, st = node.match(*scene["sweeps"][0], scene["start"])
        assert st.n_rows > 0
        if ctx_first:
            c.close()
            with pytest.raises(pkg.LslamError):
                node.match(*scene["sweeps"][0], scene["start"])
            node.close()
        else:
            node.close()
            c.close()


def test_cpp_localization_equals_the_python_mirror(pkg, synth, scene, tmp_path):
    """tests/cpp/localization_end_to_end.cpp (registration -> odometry -> localisation over a loaded map, in C++) on five sweeps:
    the same ABI calls as the Python mirrors, so the same flags, counters, poses and velocities, bit for bit."""
    from test_gpu_odom import _raw as sweep
    sr = pkg.scan_registration
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "localization_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "localization_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    dims = (21, 21, 21)
    ctx = pkg.Context(0)
    # the map in the odometry's frame: relative to the first sweep's sensor pose, in the registration's axes (x' = y, y' = z, z' = x)
    R0, t0 = synth.pose_to_Rt((0.0, 0.0, 0.3, 3.0, -2.0, synth.SENSOR_HEIGHT))

    def to_odom_frame(cloud):
        p = (cloud[:, :3].astype(np.float64) - t0) @ R0
        return np.concatenate([p[:, [1, 2, 0]], cloud[:, 3:4]], 1).astype(np.float32)
    fm = pkg.FeatureMap(ctx, *dims)
    fm.add_feature_cloud(to_odom_frame(scene["map_corner"]), to_odom_frame(scene["map_surf"]), np.eye(4, dtype=np.float32))
    d = tmp_path / "map"
    d.mkdir()
    fm.save_cloud_to_files(str(d))
    fm.close()
    reg, odo, fs = pkg.MultiScanRegistration(ctx), pkg.DeviceLaserOdometry(ctx), sr.FeatureSet(ctx)
    loc = pkg.LaserLocalization(ctx, *dims)
    loc.load_map(d)
    want = []
    with open(tmp_path / "session.bin", "wb") as fo:
        for k in range(5):
            stamp = 1_000_000_000 + k * 100_000_000
            raw = np.ascontiguousarray(sweep(synth, scene["world"], k)[:, :4], np.float32)
            fo.write(struct.pack("<IqI", 2, stamp, len(raw)))
            fo.write(raw.tobytes())
            reg.process(raw, stamp, fs)
            odo.process(fs)
            if k == 1:
                loc.handle_initial_pose(np.eye(4, dtype=np.float32))
            T = loc.process(np.array(odo.last_corner), np.array(odo.last_surf), odo.Tsum, stamp)
            st = loc.last_stats
            want.append((loc.last_flags, [loc.last_status, st.iterations, st.n_line, st.n_plane, st.n_rows] if T is not None else [-100, 0, 0, 0, 0],
                         loc.lidar_mapped.reshape(-1).copy(), np.zeros(3, np.float32) if loc.velocity is None else loc.velocity.copy()))
    for o in (loc, reg, odo, fs, ctx):
        o.close()
    out = subprocess.run([str(exe), str(tmp_path / "session.bin"), str(d)] + [str(v) for v in dims], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("SWEEP ")]
    assert len(lines) == 5 and "OK sweeps 5" in out.stdout
    for k, (w, (flags, counters, T, v)) in enumerate(zip(lines, want)):
        assert [int(x) for x in w[1:8]] == [k, flags] + counters, (k, w[:8], flags, counters)
        got = np.array([float.fromhex(x) for x in w[8:27]], np.float32)
        assert np.array_equal(bits(got[:16]), bits(T)) and np.array_equal(bits(got[16:]), bits(v)), k
    assert want[0][0] == 1 and want[1][0] & 4 and want[2][1][4] > 50  # dropped, reset, then matched against the map
