"""The conditions that make tests/test_gpu_localization_search.py meaningful, checked on the CPU with the oracle alone: the fixed
cube index on the cube walls (and what the earlier expression got wrong there), and that the wall map of
tests/loc_search_cases.py has the ties, the border points, the thin cubes and the agreement of oracle and brute force it is
meant to have; that the gate scene has its three fifth distances around 5.0 and holds still on the oracle."""
from fractions import Fraction

import numpy as np
import pytest

import loc_search_cases as lc
import localization_ref as lr
import paged_map_ref as pm

F = np.float32


@pytest.fixture(scope="module")
def case(oracle):
    return lc.Case(oracle)


def _exact_round(q):
    """Half away from zero of a float32, in rational arithmetic."""
    f = Fraction(float(q))
    n = int(abs(f) + Fraction(1, 2))  # floor(|q| + 1/2), exact
    return n if f >= 0 else -n


def test_cube_index_on_the_walls_is_exact_and_the_old_expression_was_not():
    """For cube sizes 10 and 50: every wall value of the first three walls on either side (the wall, two floats below, two
    above) lands where exact rounding of the float32 quotient puts it.  The expression the references carried until now --
    kept here as a local copy -- puts nextafter(25, 0) into cube 1 and nextafter(-25, 0) into cube -1 at cube size 50."""
    for size in (10.0, 50.0):
        vals = []
        for w in range(3):
            wall = F(size * (w + 0.5))
            five = [wall]
            for step in (F(0), F(np.inf)):
                v = np.nextafter(wall, step)
                five += [v, np.nextafter(v, step)]
            vals += five + [-v for v in five]
        vals = np.asarray(vals, F)
        want = np.array([_exact_round(v / F(size)) for v in vals])
        p = np.zeros((len(vals), 3), F)
        p[:, 1] = vals
        for origin in ((0, 0, 0), (4, 4, 2)):
            got = lr.cube_index(p, size, origin)
            assert np.array_equal(got[:, 1], want + origin[1]) and np.all(got[:, 0] == origin[0]), (size, origin)
        assert np.array_equal(pm.glo_idx(p, size)[:, 1], want)
    below = np.array([[np.nextafter(F(25), F(0)), np.nextafter(F(-25), F(0)), 0.0]], F)
    assert lr.cube_index(below, 50.0, (0, 0, 0)).tolist() == [[0, 0, 0]]
    assert lc.cube_index_old(below, 50.0, (0, 0, 0)).tolist() == [[1, -1, 0]]  # the old expression: wrong at one float per wall
    # half away from zero on the wall itself, as std::round
    on = np.array([[25.0, -25.0, 75.0]], F)
    assert lr.cube_index(on, 50.0, (0, 0, 0)).tolist() == [[1, -1, 2]]


def test_cube_index_of_what_is_not_a_number_is_no_cube():
    p = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf], [1e30, 1.0, 1.0], [np.nan] * 3], F)
    ijk = lr.cube_index(p, lc.CUBE, lc.ORIGIN)
    assert ijk[0].tolist() == [lr.NO_CUBE, 4, 2] and ijk[1, 1] == lr.NO_CUBE and ijk[2, 2] == lr.NO_CUBE and ijk[3, 0] == lr.NO_CUBE
    assert np.all(ijk[4] == lr.NO_CUBE)
    assert np.all(lc.cell_of(p) == -1)


def test_the_wall_map_is_what_it_says(case):
    for t in range(2):
        cloud, q, kind, ref = case.map[t], case.q[t], case.kind[t], case.ref[t]
        assert len(cloud) < 3000 and np.all(np.isfinite(cloud))
        cubes = ref.cubes

        def cell(w):
            return (w[0] + lc.ORIGIN[0]) + (w[1] + lc.ORIGIN[1]) * lc.DIMS[0] + (w[2] + lc.ORIGIN[2]) * lc.DIMS[0] * lc.DIMS[1]
        for n, w in lc.THIN.items():
            assert len(cubes[cell(w)]) == n, (t, n)
        assert cell(lc.EMPTY_CUBE) not in cubes
        assert len(cubes[0]) >= 5 and len(cubes[cell(lc.UNCOVERED_CUBE)]) >= 5 and len(cubes[cell(lc.CLOUD_CUBE)]) == 300
        assert max(abs(v) for v in lc.UNCOVERED_CUBE) > lc.REACH
        # the lattice straddles x = +5 and y = -5: four cubes, every one with a tree; the wall points' cubes too
        for w in ((0, 0, 0), (1, 0, 0), (0, -1, 0), (1, -1, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1)):
            assert len(cubes[cell(w)]) >= 5, w
        lat = lc.lattice_points()
        assert np.array_equal(lat * 4, np.round(lat * 4)) and {4.75, 5.0, 5.25} <= set(lat[:, 0].tolist()) and {-5.25, -5.0, -4.75} <= set(lat[:, 1].tolist())
        assert int(np.all(cloud[:, :3] == np.asarray(lc.DUP_POINT, F), axis=1).sum()) == 3
        # the first query: finite, in the centre cube, answered
        assert np.all(lc.cube_index(q[:1], lc.CUBE, lc.ORIGIN) == np.asarray(lc.ORIGIN)) and ref.ok[0]
        assert len(q) >= 513
        lattice = np.char.startswith(kind, "lattice")
        assert lattice.sum() == 240 and ref.ok[lattice].all()
        assert ref.tie[lattice].mean() >= 0.30, ref.tie[lattice].mean()
        assert ref.border.sum() >= 20 and ref.border[kind == "near a wall"].sum() >= 20
        assert ref.tie[kind == "duplicate"].all()
        # every wall value is queried on every wall, and the two sides of a wall are two cubes
        wq = q[kind == "wall value"]
        assert len(wq) == 30 and len(np.unique(ref.cell[kind == "wall value"])) == 7
        # what has no tree: the empty cube, the 4-point cube, outside, 1e30, not finite -- and nothing else
        none = np.isin(kind, ["empty cube", "thin 4", "outside the array", "1e30", "not finite"])
        assert np.array_equal(~ref.ok, none), (t, kind[ref.ok == none])
        assert (kind == "not finite").sum() == 12 and (kind == "outside the array").sum() == 6
        for n in (5, 6, 10, 11):
            assert ref.ok[kind == "thin %d" % n].all()
        cl = kind == "cloud"
        assert ref.ok[cl].all() and (~ref.tie[cl] & ~ref.border[cl]).sum() >= 100  # the generic case
        print("type %d: %d map points in %d cubes, %d queries: %d answered, %d ties (%.0f %% of the lattice queries), %d border points"
              % (t, len(cloud), len(cubes), len(q), ref.ok.sum(), ref.tie.sum(), 100 * ref.tie[lattice].mean(), ref.border.sum()))


def test_oracle_and_brute_force_agree_on_the_distances(case, oracle):
    """For every answered query the oracle tree's five distances are, as a multiset, the five smallest of the float32 brute
    force, bit for bit, and belong to the points returned; which of several tied points is returned is the oracle's alone."""
    for t in range(2):
        ref, q = case.ref[t], case.q[t]
        ok = ref.ok
        assert np.array_equal(np.sort(ref.d2[ok], axis=1).view(np.uint32), ref.brute_d2[ok].view(np.uint32))
        assert np.all(np.diff(ref.d2[ok], axis=1) >= 0)
        for i in np.flatnonzero(ok):
            pts = np.concatenate([ref.xyz[i], np.zeros((5, 1), F)], 1)
            assert np.array_equal(lc.dist2(q[i], pts).view(np.uint32), ref.d2[i].view(np.uint32))


def test_the_gridless_map_is_what_it_says(oracle):
    clouds, q, ref = lc.make_nogrid_case(oracle)
    # one cube holds all 400 corner points, and its box has more 0.6 m cells than 4 096 per point: no grid can be built
    assert len(ref[0].cubes) == 1 and len(ref[1].cubes) == 1
    ext = clouds[0][:, :3].max(0) - clouds[0][:, :3].min(0)
    assert np.prod(np.floor(ext / 0.6)) > 4096 * 4096
    assert ref[0].ok.sum() >= 250 and (~ref[0].ok).sum() >= 7 and ref[1].ok.all()


def test_the_gate_scene_holds_still_on_the_oracle(oracle):
    """The three gate points' fifth in-cube distances are 5.0, one float below and one float above (fp32 brute force); the far
    points lie beyond the surf map's box by sqrt(5) -+ 0.04 m and by more than 3 m, in the map's cube; the scan filter returns
    the scan's points unchanged; the oracle ends at the identity, converged, with every generic point and the gate point below
    5.0 matched and nothing else."""
    s = lc.make_gate_scene()
    ms, surf = s["map_surf"], s["surf"]
    assert np.array_equal(ms[:, :3] * 2, np.round(ms[:, :3] * 2)) and np.array_equal(s["map_corner"][:, :3] * 2, np.round(s["map_corner"][:, :3] * 2))
    assert len(np.unique(ms[:, :3], axis=0)) == len(ms)
    for cloud in (ms, s["map_corner"], surf):
        assert np.all(lc.cube_index(cloud, lc.CUBE, lc.ORIGIN) == np.asarray(lc.ORIGIN))
    assert F(lc.GATE_D2[1]) == np.nextafter(F(5), F(0)) and F(lc.GATE_D2[2]) == np.nextafter(F(5), F(10))
    for k, g in enumerate(s["gate"]):
        d = np.sort(lc.dist2(surf[g], ms))
        assert d[4] == F(lc.GATE_D2[k]) and d[3] < 1.5, (k, d[:6])
    lo = ms[:, 0].min()
    beyond = lo - surf[s["far"], 0]
    assert np.all(np.abs(beyond[:2] - np.sqrt(5.0)) < 0.05) and beyond[0] < np.sqrt(5.0) < beyond[1] and np.all(beyond[2:] > 3.0 + 0.1)
    for f in s["far"]:
        assert np.sort(lc.dist2(surf[f], ms))[4] > 5.0
    ref = lc.gate_reference(oracle, s)
    c, f = ref.prepare_frame(s["corner"], surf)
    assert len(c) == 0 and sorted(map(tuple, f.tolist())) == sorted(map(tuple, surf.tolist()))  # the filter: a permutation
    ok, pose, st = ref.match(s["corner"], surf, np.zeros(6, F))
    print("gate scene: %d surf map points, %d scan points (%d generic, 3 gate, 4 far); oracle ok %s iterations %d line %d plane %d rows %d |pose| %.1e"
          % (len(ms), len(surf), len(s["generic"]), ok, st.iterations, st.n_line, st.n_plane, st.n_rows, np.abs(pose).max()))
    assert ok and np.abs(pose).max() <= 1e-6
    assert (st.n_line, st.n_plane, st.n_rows) == (0, len(s["generic"]) + 1, len(s["generic"]) + 1) and st.n_rows >= 50
    # without the gate point below 5.0 there is one row less: it is the gate that decides the three
    ok2, _, st2 = ref.match(s["corner"], np.delete(surf, s["gate"][1], axis=0), np.zeros(6, F))
    assert ok2 and st2.n_plane == len(s["generic"])
