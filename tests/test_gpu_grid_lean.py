"""The lean instantiation of the grid sweep's first pass (sweep_grid_kernel<256, true>): the production loop's
launches -- MFMA sums, no taps, the fifth-distance gate, the bounded search, no counters -- run a kernel with
everything else folded away at compile time.  Same statements on the same values: the SAME BITS as the general
instantiation, which lslam_opts.ab_switches & LSLAM_AB_GRID_GENERAL (256) brings back; every launch that needs one of the
folded paths still takes the general kernel (lslam_debug_grid_lean_launches counts the lean ones)."""
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


@pytest.fixture(scope="module")
def six(synth):
    """The map of the small problem and six different 16 x 900 scans in it, with initial poses a few sweeps away."""
    pr0 = synth.make_problem(rings=16, azimuth_steps=900, world_half=60.0)
    scans, inits = [], []
    for k in range(6):
        pr = synth.make_problem(rings=16, azimuth_steps=900, world_half=60.0, seed=k)
        scans.append((pr["corner"], pr["surf"]))
        inits.append(synth.perturb_pose(pr["gt_pose"], seed=40 + k))
    return dict(map=(pr0["map_corner"], pr0["map_surf"]), scans=scans, inits=np.stack(inits))


def lean_and_general(ctx, inits, **opts):
    """The resident batch through the grid sweep with the lean kernel and with the general one: byte-equal poses, equal
    stats but for the two times; the lean counter moves in the first run only.  -> (poses, stats) of the lean run."""
    o = ctx.default_opts()
    o.search_mode = GRID
    for k, v in opts.items():
        setattr(o, k, v)
    res = []
    for ab in (0, AB_GRID_GENERAL):
        o.ab_switches = ab
        lean0, grid0 = ctx.grid_lean_launches(), ctx.grid_launches()
        _, p, st = ctx.run_batch(inits, o)
        lean, grid = ctx.grid_lean_launches() - lean0, ctx.grid_launches() - grid0
        assert grid > 0
        assert (lean == grid) if ab == 0 else (lean == 0), (ab, lean, grid)
        res.append((p.copy(), st))
    (p_lean, s_lean), (p_gen, s_gen) = res
    assert np.array_equal(bits(p_lean), bits(p_gen))
    for a, b in zip(s_lean, s_gen):
        assert stats_but_times(a) == stats_but_times(b)
    return p_lean, s_lean


@pytest.mark.parametrize("in_flight", [0, 4])
def test_lean_equals_general_bit_for_bit(ctx, six, in_flight):
    ctx.map_set(*six["map"])
    ctx.scan_set_batch(six["scans"])
    _, st = lean_and_general(ctx, six["inits"], scans_in_flight=in_flight)
    assert all(s.sweeps >= 2 for s in st)  # loops with carried bounds (prev_valid) in them


def test_launch_shapes_without_and_with_compaction(ctx, six):
    """Three scans: every workgroup of the batch in every sweep (nb_total); five: from a loop's second sweep on only the
    workgroups of the scans still running (active_blocks)."""
    ctx.map_set(*six["map"])
    for n in (3, 5):
        ctx.scan_set_batch(six["scans"][:n])
        _, st = lean_and_general(ctx, six["inits"][:n])
        assert len(st) == n and all(s.sweeps >= 2 for s in st)


def test_a_workgroup_with_one_active_lane_and_a_scan_without_corners(ctx, six):
    corner, surf = six["scans"][0]
    empty = np.zeros((0, 4), np.float32)
    ctx.map_set(*six["map"])
    ctx.scan_set_batch([(corner, surf[:257])])  # the surf list's second workgroup has a single point
    lean_and_general(ctx, six["inits"][:1])
    ctx.scan_set_batch([(empty, surf)])
    _, st = lean_and_general(ctx, six["inits"][:1])
    assert st[0].n_line == 0 and st[0].n_plane > 0


def test_a_scan_beyond_the_maps_margin(ctx, six):
    """Every point farther than the gate from every map point (GRID_FAR): nothing fetched, nothing listed, too few matches."""
    ctx.map_set(*six["map"])
    ctx.scan_set_batch(six["scans"][:1])
    far = six["inits"][:1].copy()
    far[0, 3] += 400.0
    _, st = lean_and_general(ctx, far)
    assert st[0].status == TOO_FEW_MATCHES and st[0].n_line == 0 and st[0].n_plane == 0


@pytest.mark.parametrize("max_iterations", [1, 3])
def test_loops_cut_short(ctx, six, max_iterations):
    """One iteration: a first sweep only (nothing carried, prev_valid = 0); three: carried bounds, no scan converged yet."""
    ctx.map_set(*six["map"])
    ctx.scan_set_batch(six["scans"])
    _, st = lean_and_general(ctx, six["inits"], max_iterations=max_iterations)
    assert all(s.iterations <= max_iterations for s in st) and any(s.iterations == max_iterations for s in st)


@pytest.mark.parametrize("what", ["jtj_mode", "debug_stats"])
def test_launches_that_need_a_folded_path_take_the_general_kernel(ctx, six, what):
    """The shuffle sums and the counters: no lean launch, and the results the lean loop gives (the shuffle
    sums are another order of the same terms: its counts, its pose to rounding)."""
    ctx.map_set(*six["map"])
    ctx.scan_set_batch(six["scans"])
    o = ctx.default_opts()
    o.search_mode = GRID
    _, p_ref, s_ref = ctx.run_batch(six["inits"], o)
    p_ref = p_ref.copy()
    if what == "jtj_mode":
        o.jtj_mode = 0
    else:
        o.debug_stats = 1
    lean0, grid0 = ctx.grid_lean_launches(), ctx.grid_launches()
    _, p, st = ctx.run_batch(six["inits"], o)
    assert ctx.grid_launches() > grid0 and ctx.grid_lean_launches() == lean0
    if what == "jtj_mode":
        for a, b in zip(s_ref, st):
            assert (a.status, a.iterations, a.n_rows, a.n_line, a.n_plane, a.converged) == (b.status, b.iterations, b.n_rows, b.n_line, b.n_plane, b.converged)
        assert np.abs(p - p_ref).max() <= 2e-6
    else:
        assert np.array_equal(bits(p), bits(p_ref))
        for a, b in zip(s_ref, st):
            assert stats_but_times(a) == stats_but_times(b)


def test_the_taps_take_the_general_kernel(ctx, small_problem):
    """lslam_sweep_ex with the per-point taps: no lean launch; neighbours, distances, flags and coefficients are the tree sweep's."""
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set(pr["corner"], pr["surf"])
    a = ctx.sweep(pr["init_pose"], jtj_mode=1, search_mode=LANE)
    lean0, grid0 = ctx.grid_lean_launches(), ctx.grid_launches()
    b = ctx.sweep(pr["init_pose"], jtj_mode=1, search_mode=GRID)
    assert ctx.grid_launches() > grid0 and ctx.grid_lean_launches() == lean0
    assert np.array_equal(a["flags"], b["flags"]) and np.array_equal(a["idx"], b["idx"])
    assert np.array_equal(bits(a["d2"]), bits(b["d2"])) and np.array_equal(bits(a["coeff"]), bits(b["coeff"]))


def test_fine_score_runs_lean_sweeps_and_a_general_resweep(ctx, small_problem):
    """fine_score: the loop's sweeps are the production loop's (lean), the _fineScore re-sweep -- unbounded, gated on the nearest
    neighbour, over the converged scans -- is one launch of the general kernel; the tree sweep's score2 / percent2."""
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set(pr["corner"], pr["surf"])
    o = ctx.default_opts()
    o.fine_score = 1
    o.search_mode = LANE
    _, _, s_lane = ctx.run(pr["init_pose"], o)
    o.search_mode = GRID
    res = {}
    for ab in (0, AB_GRID_GENERAL):
        o.ab_switches = ab
        lean0, grid0 = ctx.grid_lean_launches(), ctx.grid_launches()
        _, pose, st = ctx.run(pr["init_pose"], o)
        res[ab] = (pose.copy(), st, ctx.grid_lean_launches() - lean0, ctx.grid_launches() - grid0)
    pose, st, lean, grid = res[0]
    assert st.converged == 1 and lean >= 2 and grid == lean + 1
    assert res[AB_GRID_GENERAL][2] == 0 and res[AB_GRID_GENERAL][3] == grid
    assert np.array_equal(bits(pose), bits(res[AB_GRID_GENERAL][0]))
    assert stats_but_times(st) == stats_but_times(res[AB_GRID_GENERAL][1])
    assert s_lane.converged == 1 and st.percent2 == s_lane.percent2 and abs(st.score2 - s_lane.score2) <= 1e-6 * max(1.0, abs(s_lane.score2))


def test_wavefronts_that_take_the_resort_branch_fetch_by_index(ctx):
    """The lean kernel hands the points of the five survivors on to the fit unless a lane of the wavefront had to re-sort its
    six (two of them within 2^-13 of each other), in which case the wavefront gathers by index as the general kernel does.  A
    lattice of 0.4 m jittered by a micrometre, scan points ON map points at a first pose that is the identity: near-ties in
    every wavefront of that sweep, fewer as the poses move.  Lean against general bit for bit; the kd-tree walk's counts."""
    spacing, jitter = 0.4, 1e-6
    rng = np.random.default_rng(int(spacing * 1000 + jitter * 100))
    g = np.arange(-12.0, 12.0, spacing, dtype=np.float32)
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size, np.float32)], 1)
    h = np.arange(0.0, 5.0, spacing, dtype=np.float32)
    wx, wz = np.meshgrid(g, h)
    wall1 = np.stack([wx.ravel(), np.full(wx.size, 5.3, np.float32), wz.ravel()], 1)
    wall2 = np.stack([np.full(wx.size, -7.1, np.float32), wx.ravel(), wz.ravel()], 1)
    poles = np.concatenate([np.stack([np.full(len(h), x, np.float32), np.full(len(h), y, np.float32), h], 1)
                            for x, y in rng.uniform(-10, 10, (12, 2))])
    planes = np.concatenate([ground, wall1, wall2])
    pts = np.concatenate([planes, poles]).astype(np.float32)
    pts = (pts + rng.uniform(-jitter, jitter, pts.shape)).astype(np.float32)
    n_planes = len(planes)

    def cloud(xyz):
        return np.concatenate([xyz, np.zeros((len(xyz), 1))], 1).astype(np.float32)

    surf = cloud(np.concatenate([pts[rng.integers(0, n_planes, 2000)],
                                 pts[rng.integers(0, n_planes, 6000)] + rng.normal(0, 0.05, (6000, 3))]))
    corner = cloud(pts[rng.integers(n_planes, len(pts), 600)] + rng.normal(0, 0.02, (600, 3)))
    inits = np.array([[0, 0, 0, 0, 0, 0], [0.002, -0.003, 0.004, 0.03, -0.02, 0.01]], np.float32)
    ctx.map_set(pts, pts)
    ctx.scan_set_batch([(corner, surf), (corner, surf)])
    _, st = lean_and_general(ctx, inits)
    o = ctx.default_opts()
    o.search_mode = LANE
    _, _, s_lane = ctx.run_batch(inits, o)
    for a, b in zip(st, s_lane):
        assert (a.status, a.iterations, a.n_rows, a.n_line, a.n_plane) == (b.status, b.iterations, b.n_rows, b.n_line, b.n_plane)
    assert all(s.n_rows > 1000 for s in st)
