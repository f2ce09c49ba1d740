"""The x-subdivided cell tables of the grid sweep's first pass (csrc/lslam_grid.hpp CellGrid::xsub, knn5_grid<.., FINE>,
sweep_grid_kernel<256, LEAN, true>; include/lslam_c.h LSLAM_AB_GRID_CUBIC): each 0.6 m cell cut into S sub-cells
along x, the rows of a bounded probe clipped to sub-cells.  The same five neighbours as the cubic table's probe and the
kd-tree walk -- held to the oracle tap by tap -- from tables that are the same bytes build after build.

LSLAM_GRID_XSUB=S in the environment a context is made in forces S and sends explicit LSLAM_SEARCH_GRID calls and the taps
of lslam_sweep_ex through the fine tables too: every case here runs on a context of its own made that way."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AUTO, LANE, GRID = 0, 1, 3
CARRIED, FIRST = 0x400, 0x800
AB_GRID_GENERAL, AB_GRID_CUBIC = 256, 512
TOO_FEW_MATCHES = 5
TIMES = ("gpu_ms_total", "gpu_ms_sweep")
GRID_MAX_DIM, CELL = 2048, np.float32(0.6)
SUBS = (2, 3, 4)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stats_but_times(st):
    return [(name, getattr(st, name)) for name, _ in st._fields_ if name not in TIMES]


def rows_equal(a, b):
    """bench.py's rows_equal: match counts equal up to a handful of threshold-adjacent points."""
    return all(abs(int(x) - int(y)) <= max(2, int(1e-4 * max(x, y)))
               for x, y in ((a.n_rows, b.n_rows), (a.n_line, b.n_line), (a.n_plane, b.n_plane)))


@pytest.fixture(scope="module")
def prob(synth):
    """A map of a few thousand points (25 m around the origin of the small world) and two scans in it: 64 x 100, and 513
    points of it -- two workgroups and one with a single active lane."""
    pr = synth.make_problem(rings=64, azimuth_steps=100, world_half=60.0, map_radius=25.0)
    k = 256 if len(pr["corner"]) >= 256 else 0   # the surf list's last workgroup has ONE point either way
    small = (pr["corner"][:k], pr["surf"][:513 - k])
    assert len(small[0]) + len(small[1]) == 513 and len(small[1]) % 256 == 1
    return dict(map=(pr["map_corner"], pr["map_surf"]), scans={"513": small, "64x100": (pr["corner"], pr["surf"])},
                init=pr["init_pose"], gt=pr["gt_pose"])


@pytest.fixture(scope="module")
def fine_ctx(pkg):
    """One context per S, made with LSLAM_GRID_XSUB=S in the environment (read once, in lslam_ctx_create)."""
    import os
    made = {}

    def get(S):
        if S not in made:
            old = os.environ.get("LSLAM_GRID_XSUB")
            os.environ["LSLAM_GRID_XSUB"] = str(S)
            try:
                made[S] = pkg.Context(0)
            finally:
                if old is None:
                    del os.environ["LSLAM_GRID_XSUB"]
                else:
                    os.environ["LSLAM_GRID_XSUB"] = old
        return made[S]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def trees(oracle, prob):
    return oracle.kdtree(prob["map"][0]), oracle.kdtree(prob["map"][1])


@pytest.mark.parametrize("scan", ["513", "64x100"])
@pytest.mark.parametrize("S", SUBS)
def test_taps_of_every_sweep_of_the_loop_match_the_oracle(fine_ctx, oracle, prob, trees, S, scan):
    """tests/test_gpu_stack_shapes.py's check of the cubic table, over the fine one: sweep k + 1 of the loop is the tap right
    after a run cut at max_iterations = k (LSLAM_SWEEP_CARRIED: the CLIPPED state), the first LSLAM_SWEEP_FIRST.  Flags and
    coefficients of every point bit for bit; indices and distances bit for bit wherever d2[4] < 5."""
    c = fine_ctx(S)
    tc, ts = trees
    qc, qs = prob["scans"][scan]
    c.map_set(*prob["map"])
    c.scan_set(qc, qs)
    o = c.default_opts()
    o.search_mode = GRID
    pose = np.asarray(prob["init"], np.float32)
    n_sweeps = n_pts = 0
    for k in range(6):
        if k > 0:
            o.max_iterations = k
            _, pose, st = c.run(prob["init"], o)
            if st.iterations < k or st.converged:
                break
        f0, g0 = c.grid_fine_launches(), c.grid_launches()
        g = c.sweep(pose, jtj_mode=1, search_mode=GRID | (CARRIED if k > 0 else FIRST))
        assert c.grid_launches() == g0 + 1 and c.grid_fine_launches() == f0 + 1   # the general FINE instantiation, with taps
        r = oracle.sweep(tc, ts, qc, qs, pose)
        assert np.array_equal(g["flags"], r["flags"]), (k, np.argwhere(g["flags"] != r["flags"])[:5].tolist())
        assert np.array_equal(bits(g["coeff"]), bits(r["coeff"])), k
        looked_up = (r["flags"] & 1) != 0
        assert np.array_equal(g["idx"][looked_up], r["idx"][looked_up]), (k, np.argwhere((g["idx"] != r["idx"]).any(1) & looked_up)[:5].tolist())
        assert np.array_equal(bits(g["d2"])[looked_up], bits(r["d2"])[looked_up]), k
        assert g["sums"][27] == r["sums"][27] and g["sums"][28] == r["sums"][28]
        n_sweeps += 1
        n_pts += int(looked_up.sum())
    assert c.grid_fine_info()["xsub"] == (S, S)
    assert n_sweeps >= 3 and n_pts > 300, (n_sweeps, n_pts)


def run_modes(c_fine, c_cubic, maps, scans, inits, **opts):
    """-> {mode: (poses, stats)} of the batch through the fine tables (lean and general), the cubic table and the kd-tree walk"""
    out = {}
    for name, c, mode, ab in (("fine", c_fine, GRID, 0), ("fine_general", c_fine, GRID, AB_GRID_GENERAL), ("cubic", c_cubic, GRID, 0),
                              ("lane", c_cubic, LANE, 0)):
        c.map_set(*maps)
        c.scan_set_batch(scans)
        o = c.default_opts()
        o.search_mode = mode
        o.ab_switches = ab
        for k, v in opts.items():
            setattr(o, k, v)
        f0, l0, g0 = c.grid_fine_launches(), c.grid_lean_launches(), c.grid_launches()
        _, p, st = c.run_batch(np.asarray(inits, np.float32), o)
        fine, lean, grid = c.grid_fine_launches() - f0, c.grid_lean_launches() - l0, c.grid_launches() - g0
        if name.startswith("fine"):
            assert grid > 0 and fine == grid and lean == (grid if ab == 0 else 0), (name, fine, lean, grid)
        else:
            assert fine == 0
        out[name] = (p.copy(), st)
    return out


def held_to_the_cubic_table(res, what=""):
    """Lean and general over the fine table: the same bits.  Fine against cubic: iterations equal, rows equal as bench.py's
    rows_equal has it, poses within ten times what the cubic table and the kd-tree walk differ by on this very problem --
    the bound the library's search modes are held to against each other.  (The three group their sums differently -- which
    points pass 2 adds -- so their poses differ in the last bits from a loop's second iteration on.)"""
    (pf, sf), (pg, sg), (pc, sc), (pl, sl) = res["fine"], res["fine_general"], res["cubic"], res["lane"]
    assert np.array_equal(bits(pf), bits(pg))
    for a, b in zip(sf, sg):
        assert stats_but_times(a) == stats_but_times(b)
    d_ref = float(np.abs(pc.astype(np.float64) - pl).max())
    d_fine = float(np.abs(pf.astype(np.float64) - pc).max())
    print("%s pose difference: cubic against kd-tree walk %.3g, fine against cubic %.3g (bound %.3g)" % (what, d_ref, d_fine, 10 * d_ref))
    for a, b, l in zip(sf, sc, sl):
        assert a.status == b.status and a.iterations == b.iterations == l.iterations and a.converged == b.converged
        assert rows_equal(a, b) and rows_equal(a, l)
    assert d_fine <= 10.0 * d_ref, (what, d_fine, d_ref)
    return sf


@pytest.mark.parametrize("S", SUBS)
def test_poses_and_statistics_match_the_cubic_table(fine_ctx, ctx, prob, S):
    """Both scans as one batch.  Measured on MI355X: the cubic table against the kd-tree walk 2.38e-07 (one fp32 place of a
    2 m coordinate), so the bound is 2.38e-06; the fine tables against the cubic one 0 for S = 2, 3 and 4 -- on these small
    problems the same points are proven in the same pass.  (On the shapes below the first figure is 0 to 9.3e-10 and the
    fine tables' difference 0 as well.)"""
    scans = [prob["scans"]["513"], prob["scans"]["64x100"]]
    inits = [prob["init"], prob["init"]]
    st = held_to_the_cubic_table(run_modes(fine_ctx(S), ctx, prob["map"], scans, inits), "S=%d" % S)
    assert all(s.sweeps >= 3 for s in st)


def test_a_scan_beyond_the_margin_and_a_point_that_is_not_a_number(fine_ctx, ctx, prob):
    qc, qs = prob["scans"]["64x100"]
    qs = qs.copy()
    qs[7, 0] = np.nan
    qs[300, 2] = np.inf
    far = np.asarray(prob["init"], np.float32).copy()
    far[3] += 400.0
    for S in SUBS:
        res = run_modes(fine_ctx(S), ctx, prob["map"], [(qc, qs), (qc, qs)], [prob["init"], far])
        st = held_to_the_cubic_table(res, "S=%d, NaN point" % S)
        assert st[0].n_plane > 100 and st[1].status == TOO_FEW_MATCHES and st[1].n_line == 0 and st[1].n_plane == 0


def expected_xsub(pts, S):
    """GridDev::build's rule: the largest S' <= S with nx <= GRID_MAX_DIM and the table within its cell limits."""
    F = np.float32
    margin = int(F(2.2361) / CELL) + 3
    lo, hi = pts[:, :3].min(0).astype(F), pts[:, :3].max(0).astype(F)
    org = (lo - F(margin) * CELL).astype(F)
    dims = np.floor(((hi - org).astype(F) * (F(1.0) / CELL)).astype(F)).astype(np.int64) + 1 + margin
    cap = min(1 << 26, 4096 * max(len(pts), 4096))
    while S > 1 and (dims[0] * S > GRID_MAX_DIM or dims[0] * S * dims[1] * dims[2] > cap):
        S -= 1
    return S


@pytest.mark.parametrize("half_width, lowered_to", [(175.0, {2: 2, 3: 3, 4: 3}), (400.0, {2: 1, 3: 1, 4: 1})])
def test_a_map_so_wide_that_xsub_is_lowered(fine_ctx, ctx, prob, half_width, lowered_to):
    """Two far points stretch the box along x: 350 m -> 604 cells, four sub-cells each would be 2 416 > GRID_MAX_DIM, three
    fit; 800 m -> 1 354 cells, not even two fit: the "fine" table is a cubic one.  The reported value, and the results."""
    mc, ms = prob["map"]
    ext = np.array([[-half_width, 0, 0, 0], [half_width, 0, 0, 0]], np.float32)
    maps = (np.concatenate([mc, ext]), np.concatenate([ms, ext]))
    for S in SUBS:
        c = fine_ctx(S)
        res = run_modes(c, ctx, maps, [prob["scans"]["64x100"]], [prob["init"]])
        held_to_the_cubic_table(res, "S=%d, %g m wide" % (S, 2 * half_width))
        want = lowered_to[S]
        assert expected_xsub(maps[0], S) == want and expected_xsub(maps[1], S) == want
        assert c.grid_fine_info()["xsub"] == (want, want), (S, c.grid_fine_info())


def test_a_row_longer_than_64_candidates_and_duplicate_map_points(fine_ctx, ctx, prob):
    """Eighty map points within 5 cm of a scan point's image: its row overflows the candidate id -- unproven, searched in the
    tree, not wrong.  Fifty map points twice: exact ties, which only nanoflann's visit order decides -- pass 2."""
    mc, ms = prob["map"]
    qc, qs = prob["scans"]["64x100"]
    rng = np.random.default_rng(3)
    near = ms[np.argsort(np.linalg.norm(ms[:, :3] - [3.0, -2.0, 0.0], axis=1))[5], :3]
    blob = np.c_[near + rng.uniform(0, 0.05, (80, 3)), np.zeros(80)].astype(np.float32)
    dup = ms[rng.choice(len(ms), 50, replace=False)]
    maps = (mc, np.concatenate([ms, blob, dup]))
    for S in SUBS:
        st = held_to_the_cubic_table(run_modes(fine_ctx(S), ctx, maps, [(qc, qs)], [prob["init"]]), "S=%d, blob and duplicates" % S)
        assert st[0].n_plane > 100


def test_the_table_is_the_same_bytes_build_after_build_and_every_point_in_its_sub_cell(fine_ctx, prob):
    F = np.float32
    for S in SUBS:
        c = fine_ctx(S)
        c.map_set(*prob["map"])
        c.scan_set(*prob["scans"]["513"])
        o = c.default_opts()
        o.search_mode = GRID
        c.run(prob["init"], o)   # the first call that wants them builds them
        for which, src in ((0, prob["map"][0]), (1, prob["map"][1])):
            dims, geom, cs, pts = c.grid_fine_table(which)
            dims2, geom2, cs2, pts2 = c.grid_fine_table(which, rebuild=True)
            assert np.array_equal(dims, dims2) and geom.tobytes() == geom2.tobytes()
            assert cs.tobytes() == cs2.tobytes() and pts.tobytes() == pts2.tobytes()
            nx, ny, nz, xsub = (int(v) for v in dims)
            assert xsub == S and len(pts) == len(src) and cs[0] == 0 and cs[-1] == len(pts) and np.all(np.diff(cs.astype(np.int64)) >= 0)
            org, cell, inv_cx = geom[:3], geom[3], geom[4]
            assert inv_cx == F(F(S) / cell)
            inv_c = F(1.0) / cell
            ix = np.floor(((pts[:, 0] - org[0]).astype(F) * inv_cx).astype(F)).astype(np.int64)   # the two fp32 operations
            iy = np.floor(((pts[:, 1] - org[1]).astype(F) * inv_c).astype(F)).astype(np.int64)
            iz = np.floor(((pts[:, 2] - org[2]).astype(F) * inv_c).astype(F)).astype(np.int64)
            cellno = ix + nx * (iy + ny * iz)
            pos = np.arange(len(pts))
            assert np.all(cs[cellno] <= pos) and np.all(pos < cs[cellno + 1])
            orig = pts[:, 3].copy().view(np.uint32).astype(np.int64)
            assert np.array_equal(np.sort(orig), np.arange(len(src))) and np.array_equal(pts[:, :3], src[orig, :3].astype(F))
            same_cell = cellno[1:] == cellno[:-1]
            assert np.all(orig[1:][same_cell] > orig[:-1][same_cell])   # original-index order inside a sub-cell


@pytest.fixture(scope="module")
def six_full(synth):
    """Six 64 x 1800 matches (one scan of the small world under six initial poses): more than two wavefronts per SIMD."""
    pr = synth.make_problem(rings=64, azimuth_steps=1800, world_half=60.0)
    inits = np.stack([synth.perturb_pose(pr["gt_pose"], seed=70 + k) for k in range(6)])
    return dict(map=(pr["map_corner"], pr["map_surf"]), scans=[(pr["corner"], pr["surf"])] * 6, inits=inits)


def test_launch_counters_who_takes_the_fine_tables(pkg, ctx, six_full):
    """AUTO on a throughput-bound batch: every grid launch over the fine tables (built once, reported).  Explicit GRID,
    LSLAM_AB_GRID_CUBIC and a map with deferred trees: none."""
    ctx.map_set(*six_full["map"])
    ctx.scan_set_batch(six_full["scans"])
    o = ctx.default_opts()
    res = {}
    for name, mode, ab in (("auto", AUTO, 0), ("grid", GRID, 0), ("auto_cubic", AUTO, AB_GRID_CUBIC), ("lane", LANE, 0)):
        o.search_mode, o.ab_switches = mode, ab
        f0, g0 = ctx.grid_fine_launches(), ctx.grid_launches()
        _, p, st = ctx.run_batch(six_full["inits"], o)
        res[name] = (p.copy(), st, ctx.grid_fine_launches() - f0, ctx.grid_launches() - g0)
    assert res["auto"][3] > 0 and res["auto"][2] == res["auto"][3]
    info = ctx.grid_fine_info()
    assert info["xsub"][0] >= 2 and info["xsub"][0] == info["xsub"][1] and info["build_ms"] > 0.0
    assert res["grid"][3] > 0 and res["grid"][2] == 0
    assert res["auto_cubic"][3] > 0 and res["auto_cubic"][2] == 0
    # the switch restores the explicit grid sweep's bytes; the fine tables' poses are within the modes' bound of them
    assert np.array_equal(bits(res["auto_cubic"][0]), bits(res["grid"][0]))
    for a, b in zip(res["auto"][1], res["grid"][1]):
        assert a.iterations == b.iterations and rows_equal(a, b)
    d_ref = float(np.abs(res["grid"][0].astype(np.float64) - res["lane"][0]).max())
    d_fine = float(np.abs(res["auto"][0].astype(np.float64) - res["grid"][0]).max())
    print("six 64 x 1800: cubic against kd-tree walk %.3g, fine against cubic %.3g" % (d_ref, d_fine))
    assert res["lane"][3] == 0 and d_fine <= 10.0 * d_ref
    c2 = pkg.Context(0)
    try:
        c2.defer_trees(True)
        c2.map_set(*six_full["map"])
        c2.scan_set_batch(six_full["scans"])
        o2 = c2.default_opts()
        f0, g0 = c2.grid_fine_launches(), c2.grid_launches()
        c2.run_batch(six_full["inits"], o2)
        assert c2.grid_launches() > g0 and c2.lazy_trees()[0] == 1
        assert c2.grid_fine_launches() == f0 and c2.grid_fine_info()["xsub"] == (0, 0)
    finally:
        c2.close()
