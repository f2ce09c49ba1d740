"""The localisation node's neighbour search (loc_probe_kernel / loc_tree_kernel, csrc/lslam_loc.hip) on the placed inputs of
tests/loc_search_cases.py: cube walls, exact ties, thin cubes, cubes the grids do not cover, a type without a grid, queries
outside the array and queries that are not numbers -- the tap's five against ``oracle.kdtree(cube).knn`` bit for bit for EVERY
query, no tie mask; the workgroup edges; the paged node over the same map; and the loop's gate (d2[4] < 5.0) and the grid's
GRID_FAR verdict through lslam_loc_match on a scene that holds still."""
import numpy as np
import pytest

import loc_search_cases as lc
import localization_ref as lr

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def case(oracle):
    return lc.Case(oracle)


def _node(pkg, ctx, clouds=None, dims=lc.DIMS, cube=lc.CUBE, grid=True):
    node = pkg.LaserLocalization(ctx, *dims, cube_size=cube, lidar_valid_distance=lc.VALID)
    if clouds is not None:
        node.set_map(clouds[0], clouds[1], filter=False)
    node.set_search(grid)
    return node


def _assert_equals_reference(got, ref, label):
    """xyz, d2 of every query equal the oracle tree's; how == 0 and zeros exactly where the reference has no tree."""
    xyz, d2, how = got
    assert np.array_equal(how != 0, ref.ok), (label, np.flatnonzero((how != 0) != ref.ok)[:10])
    wrong = np.flatnonzero(np.any(bits(d2) != bits(ref.d2), axis=1) | np.any(bits(xyz) != bits(ref.xyz), axis=(1, 2)))
    assert len(wrong) == 0, (label, wrong[:10], d2[wrong[:3]], ref.d2[wrong[:3]])
    assert not xyz[~ref.ok].any() and not d2[~ref.ok].any(), label


@pytest.fixture(scope="module")
def full(pkg, _session_ctx, case):
    """The whole query set through one node with the grids on: type 0, then type 1, back to back."""
    node = _node(pkg, _session_ctx, case.map)
    out = [node.debug_knn5(t, case.q[t]) for t in range(2)]
    info = node.info()
    node.close()
    return out, info


def test_every_query_equals_its_cube_tree(case, full):
    """Grids on.  Bit for bit against the oracle for every query; every tie, every border point and every query of the
    uncovered cube decided by the cube's tree; the jittered cloud reaches the grid path."""
    out, info = full
    assert info["grid_reach"] == lc.REACH and info["grid_on"] == (1, 1) and info["grid_cube"] == lc.ORIGIN
    for t in range(2):
        ref, kind = case.ref[t], case.kind[t]
        xyz, d2, how = out[t]
        print("type %d: %d queries, %d answered, %d ties, %d border points, how %s; by kind: %s" %
              (t, len(how), int(ref.ok.sum()), int(ref.tie.sum()), int(ref.border.sum()), np.bincount(how, minlength=3).tolist(),
               {k: np.bincount(how[kind == k], minlength=3).tolist() for k in sorted(set(kind.tolist()))}))
        _assert_equals_reference(out[t], ref, "grid on, type %d" % t)
        assert np.all(how[ref.tie] == 2) and np.all(how[ref.border] == 2) and np.all(how[kind == "uncovered cube"] == 2)
        assert np.all(how[np.isin(kind, ["empty cube", "thin 4", "outside the array", "1e30", "not finite"])] == 0)
        assert int((how[kind == "cloud"] == 1).sum()) >= 1


def test_tree_only_search_gives_the_same_bits(pkg, ctx, case, full):
    node = _node(pkg, ctx, case.map, grid=False)
    for t in range(2):
        got = node.debug_knn5(t, case.q[t])
        print("type %d, trees only: how %s" % (t, np.bincount(got[2], minlength=3).tolist()))
        _assert_equals_reference(got, case.ref[t], "trees only, type %d" % t)
        assert set(got[2][case.ref[t].ok].tolist()) == {2}
        assert np.array_equal(bits(got[0]), bits(full[0][t][0])) and np.array_equal(bits(got[1]), bits(full[0][t][1]))
    node.close()


def test_a_type_without_a_grid(pkg, ctx, oracle):
    """400 corner points over a 170 m box in one 200 m cube: no cell table is allowed that many cells, every corner query goes
    to the tree; the surf type keeps its grid."""
    clouds, q, ref = lc.make_nogrid_case(oracle)
    node = _node(pkg, ctx, clouds, lc.NOGRID_DIMS, lc.NOGRID_CUBE)
    got = [node.debug_knn5(t, q[t]) for t in range(2)]
    info = node.info()
    node.close()
    print("no corner grid: grid_on %s reach %d, how %s" % (info["grid_on"], info["grid_reach"], [np.bincount(g[2], minlength=3).tolist() for g in got]))
    assert info["grid_on"] == (0, 1)
    for t in range(2):
        _assert_equals_reference(got[t], ref[t], "no corner grid, type %d" % t)
    assert set(got[0][2][ref[0].ok].tolist()) == {2} and int((got[1][2] == 1).sum()) >= 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_the_first_n_queries_alone(pkg, ctx, case, full, n):
    """A fresh node, the first n queries (the same first query: the same grids): the first n rows of the full run."""
    node = _node(pkg, ctx, case.map)
    for t in range(2):
        got = node.debug_knn5(t, case.q[t][:n])
        for a, b in zip(got, full[0][t]):
            assert np.array_equal(a, b[:n]) if a.dtype == np.uint8 else np.array_equal(bits(a), bits(b[:n])), (t, n)
    node.close()


def test_the_paged_node_over_the_same_map(pkg, ctx, case, oracle, tmp_path):
    """The wall map binned on the device (lslam_fmap_add_feature_cloud) and written by lslam_fmap_save; index2.txt is index.txt
    less the origin.  The static node that loads the directory and the paged node opened on it (both filter every cube at 0.2 m)
    give the same tap bit for bit, and both equal the oracle trees of the restatement's load of the same files."""
    leaf = 0.2
    fm = pkg.FeatureMap(ctx, *lc.DIMS)
    fm.setup_world_cube_size(lc.CUBE)
    fm.add_feature_cloud(case.map[0], case.map[1], np.eye(4, dtype=F))  # no active area: nothing is filtered
    d = tmp_path / "map"
    d.mkdir()
    fm.save_cloud_to_files(str(d))
    fm.close()
    with open(d / "index2.txt", "w") as f:
        for line in open(d / "index.txt"):
            w = [int(v) for v in line.split()]
            f.write("%d %d %d %d %d %d\n" % (w[0], w[1], w[2] - lc.ORIGIN[0], w[3] - lc.ORIGIN[1], w[4] - lc.ORIGIN[2], w[5]))
    # the device put every map point -- the wall values among them -- into the cube the fixed cube_index names
    raw = lr.RefLocalization(oracle, lc.DIMS, lc.CUBE, lc.ORIGIN, map_filter_corner=leaf, map_filter_surf=leaf)
    raw.load_map(str(d), filter=False)
    for t in range(2):
        want = lc.bin_cubes(case.map[t])
        assert sorted(raw.cubes[t]) == sorted(want), t
        for c, pts in want.items():
            got = raw.cubes[t][c]
            assert np.array_equal(bits(got[np.argsort(got[:, 3], kind="stable")]), bits(pts)), (t, c)  # (the intensity is the point's number)
    ref = lr.RefLocalization(oracle, lc.DIMS, lc.CUBE, lc.ORIGIN, map_filter_corner=leaf, map_filter_surf=leaf)
    ref.load_map(str(d), filter=True)
    static = pkg.LaserLocalization(ctx, *lc.DIMS, map_filter_corner=leaf, map_filter_surf=leaf, cube_size=lc.CUBE, lidar_valid_distance=lc.VALID)
    static.load_map(d)
    paged = pkg.LaserLocalization(ctx, *lc.DIMS, map_filter_corner=leaf, map_filter_surf=leaf, cube_size=lc.CUBE, lidar_valid_distance=lc.VALID,
                                  dynamic_mode=True, files_directory=str(d))
    paged.update(np.zeros(3, F))
    assert tuple(paged.window_info()["centre"]) == (0, 0, 0)
    for t in range(2):
        want = lc.Reference(oracle, None, case.q[t], cubes=ref.cubes[t], cells=lc.cell_of(case.q[t]))
        a, b = static.debug_knn5(t, case.q[t]), paged.debug_knn5(t, case.q[t])
        print("type %d: filtered map %d points; static how %s, paged how %s; %d ties, %d border points" %
              (t, len(ref.map[t]), np.bincount(a[2], minlength=3).tolist(), np.bincount(b[2], minlength=3).tolist(), int(want.tie.sum()), int(want.border.sum())))
        _assert_equals_reference(a, want, "static, loaded, type %d" % t)
        _assert_equals_reference(b, want, "paged, type %d" % t)
        assert np.all(b[2][want.tie] == 2) and np.all(b[2][want.border] == 2)
    static.close()
    paged.close()


def test_the_gate_and_grid_far_through_the_loop(pkg, ctx, oracle):
    """lslam_loc_match on the scene that holds still (loc_search_cases.make_gate_scene; its conditions are checked on the CPU by
    tests/test_loc_search_cases.py): iterations and the three counters equal ``oracle.scanmatch_cubes``'s with the grids on and
    off -- the scan point with d2[4] one float below 5.0 is matched, the ones at 5.0, one float above and beyond the map are not
    -- the pose stays at the identity and is the same in every bit for both settings; the grid decides points when it is on."""
    s = lc.make_gate_scene()
    ok, pr, st_r = lc.gate_reference(oracle, s).match(s["corner"], s["surf"], np.zeros(6, F))
    assert ok and np.abs(pr).max() <= 1e-6
    runs = []
    for grid in (True, False):
        node = pkg.LaserLocalization(ctx, *lc.DIMS, filter_corner=lc.GATE_SCAN_LEAF, filter_surf=lc.GATE_SCAN_LEAF, cube_size=lc.CUBE,
                                     lidar_valid_distance=lc.VALID)
        node.set_map(s["map_corner"], s["map_surf"], filter=False)
        node.set_search(grid)
        status, p, st = node.match(s["corner"], s["surf"], np.zeros(6, F))
        stats, info = node.search_stats(), node.info()
        node.close()
        print("grid %s: status %d iterations %d line %d plane %d rows %d |pose| %.1e; swept %d proven by the grid %d refused %d to trees %d; grid_on %s"
              % (grid, status, st.iterations, st.n_line, st.n_plane, st.n_rows, np.abs(p).max(), stats["swept"][0], stats["grid_proven"][0],
                 stats["cube_refused"][0], stats["to_trees"][0], info["grid_on"]))
        assert (status == 0) == ok
        assert (st.iterations, st.n_line, st.n_plane, st.n_rows) == (st_r.iterations, st_r.n_line, st_r.n_plane, st_r.n_rows)
        assert np.abs(p).max() <= 1e-6
        if grid:
            # the two points beyond the grid's margin lie outside its interior cells: GRID_FAR, decided by the grid (on this
            # 0.5 m lattice the grid proves no five of its own: measured 2 of 130 by the grid, 128 by the trees)
            assert info["grid_on"][1] == 1 and stats["grid_proven"][0] >= 2
        else:
            assert stats["grid_proven"][0] == 0
        runs.append((status, p, st))
    assert runs[0][0] == runs[1][0] and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
