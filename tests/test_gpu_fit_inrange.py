"""The in-range fit (csrc/lslam_device.hpp: div_inrange, sqrt_inrange, FitRange): in the lean sweep kernels the plane
and line fits divide and take square roots without the range steps `/` and sqrtf compile to, watch their operands, and a
wavefront with one operand outside the range fits again as every other kernel does.  Checked here on the device:
the two chains beside `/` and sqrtf on the operands of real fits and on the range's edges; whole fits on real neighbour sets,
in range and general; a batch with the switch on and off (LSLAM_FIT_INRANGE, read when a context is made); and a map whose
floor lies at z = 0 exactly, whose plane fits the guard refuses, against the general kernels
(tests/test_gpu_grid_lean.py, test_gpu_queue_lean.py, test_gpu_run_schedule.py and test_gpu_grid_xsub.py hold the lean kernels to
the general ones on everything else)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = 3
AB_GRID_GENERAL = 256
TIMES = ("gpu_ms_total", "gpu_ms_sweep")
FIT_LO, FIT_HI = np.float32(2.0 ** -30), np.float32(2.0 ** 30)
FP = C.POINTER(C.c_float)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stats_but_times(st):
    return [(name, getattr(st, name)) for name, _ in st._fields_ if name not in TIMES]


def ops(ctx, a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    out = np.zeros((len(a), 8), np.float32)
    rc = ctx.lib.lslam_debug_fit_inrange_ops(ctx.h, a.ctypes.data_as(FP), b.ctypes.data_as(FP), len(a), out.ctypes.data_as(FP))
    assert rc == 0, rc
    return out


def fits(ctx, nb, x, is_surf):
    nb, x = np.ascontiguousarray(nb, np.float32), np.ascontiguousarray(x, np.float32)
    n = len(x)
    assert nb.shape == (n, 5, 4) and x.shape == (n, 4)
    oi, og, fl = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.float32), np.zeros(n, np.int32)
    rc = ctx.lib.lslam_debug_fit_inrange_fits(ctx.h, nb.ctypes.data_as(FP), x.ctypes.data_as(FP), n, int(is_surf), oi.ctypes.data_as(FP),
                                              og.ctypes.data_as(FP), fl.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return oi, og, fl


def xyz0(p):
    p = np.asarray(p, np.float32)
    return np.concatenate([p[:, :3], np.zeros((len(p), 1), np.float32)], 1)


@pytest.fixture(scope="module")
def real_fits(_session_ctx, synth, small_problem):
    """One 16 x 1800 scan at its true pose against the small map: per scan point its five map neighbours (the library's own
    search) -> {type: (neighbours [n, 5, 4], points [n, 4])}, computed once."""
    ctx, pr = _session_ctx, small_problem
    corner, surf, gt = synth.make_scan(pr["world"], 16, 1800, gt_pose=tuple(float(v) for v in pr["gt_pose"]), seed=311)
    R, t = synth.pose_to_Rt(gt)
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    out = {}
    for which, pts, m in ((0, corner, pr["map_corner"]), (1, surf, pr["map_surf"])):
        x = xyz0((pts[:, :3].astype(np.float64) @ R.T + t).astype(np.float32))
        idx, d2 = ctx.knn5(which, x)
        near = (idx >= 0).all(1) & (d2[:, 4] < 5.0)
        out[which] = (xyz0(m)[idx[near].reshape(-1)].reshape(-1, 5, 4), x[near])
    assert len(out[0][1]) > 200 and len(out[1][1]) > 2000
    return out


def edge_values():
    v = []
    for e in (-30, -29, -1, 0, 1, 28, 29):
        for m in (0, 1, 0x400000, 0x7FFFFE, 0x7FFFFF):
            for s in (0, 0x80000000):
                v.append(s | ((e + 127) << 23) | m)
    v += [0x4E800000, 0xCE800000]  # +-FIT_HI
    return np.array(v, np.uint32).view(np.float32)


def test_chains_beside_division_and_square_root(ctx, real_fits):
    """div_inrange / sqrt_inrange beside `/` and sqrtf in one kernel: the operands of real plane fits -- coordinates, their
    sums, column norms and the norms' ratios, as the fit pairs them -- and every pair of the edge list; equal bit for bit
    wherever the guard lets the pair through, and it lets all the real ones through but a handful."""
    nb, x = real_fits[1]
    n = min(len(nb), 1500)
    p = nb[:n, :, :3]
    col = np.sqrt((p.astype(np.float32) ** 2).sum(1, dtype=np.float32))  # [n, 3] column norms
    sums = p.sum(1, dtype=np.float32)
    a = np.concatenate([p[:, 1:, 0].reshape(-1), sums.reshape(-1), col[:, 1], col[:, 2], x[:n, 0], (col ** 2).reshape(-1)])
    b = np.concatenate([np.repeat(col[:, 0] + np.abs(p[:, 0, 0]), 4), np.repeat(col[:, 0], 3), col[:, 0], col[:, 1], col[:, 2],
                        np.repeat(col[:, 1], 3)])
    assert len(a) == len(b) and len(a) > 4000
    e = edge_values()
    ea, eb = np.repeat(e, len(e)), np.tile(e, len(e))
    za = np.zeros(len(e), np.float32)  # +0 over every denominator
    a, b = np.concatenate([a, ea, za]).astype(np.float32), np.concatenate([b, eb, e]).astype(np.float32)
    out = ops(ctx, a, b)
    verdict = out[:, 4].view(np.int32)
    a_ok, b_ok = (verdict & 1) != 0, (verdict & 2) != 0
    # the guard: the range, and no denominator with its mantissa all ones
    assert np.array_equal(a_ok, (np.abs(a) >= FIT_LO) & (np.abs(a) <= FIT_HI))
    assert np.array_equal(b_ok, (np.abs(b) >= FIT_LO) & (np.abs(b) <= FIT_HI) & ((bits(b) & 0x7FFFFF) != 0x7FFFFF))
    n_real = len(a) - len(ea) - len(za)
    print("real operand pairs:", n_real, "refused:", int((~(a_ok & b_ok))[:n_real].sum()), "edge pairs:", len(ea))
    assert (a_ok & b_ok)[:n_real].mean() > 0.99
    ok = (a_ok | (bits(a) == 0)) & b_ok
    assert ok.sum() > n_real
    assert np.array_equal(bits(out[ok, 0]), bits(out[ok, 1]))
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(out[ok, 1]), bits(a[ok] / b[ok]))  # (the device's `/` is the correctly rounded one)
    # the square root's own range: 2^-96 <= x < inf, and +0
    sq = np.concatenate([np.abs(a), np.array([2.0 ** -96, 2.0 ** -95, 3.0e38, 0.0], np.float32)]).astype(np.float32)
    so = ops(ctx, sq, np.ones_like(sq))
    assert np.array_equal(bits(so[:, 2]), bits(so[:, 3]))
    assert np.array_equal(bits(so[:, 3]), bits(np.sqrt(sq)))


def test_reciprocal_of_five_literal(ctx):
    """FIT_RCP5 is what the chain's two refinement steps make of v_rcp_f32(5.0f) on this device, and dividing by 5 from it
    equals `/ 5.0f`."""
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(4096) * np.exp(rng.uniform(-12, 12, 4096))).astype(np.float32)
    out = ops(ctx, a, np.full(len(a), 5.0, np.float32))
    assert np.all(bits(out[:, 5]) == bits(out[:, 6])) and bits(out[:1, 6])[0] == 0x3E4CCCCD
    assert np.array_equal(bits(out[:, 7]), bits(a / np.float32(5.0)))
    assert np.array_equal(bits(out[:, 7]), bits(out[:, 1]))


@pytest.mark.parametrize("which", [0, 1])
def test_whole_fits_on_real_neighbours(ctx, real_fits, which):
    """find_line + the corner coefficient (0) and find_plane + the surf coefficient (1), in range and as every other kernel
    has them, one fit per lane on the scan's real neighbour sets: same verdicts, same bits.  (The line fit's divisions guard
    themselves; a plane fit whose guard refuses an operand is fitted again in the sweep kernels: bit 4.)"""
    nb, x = real_fits[which]
    oi, og, fl = fits(ctx, nb, x, which)
    refused = (fl & 16) != 0
    print("fits:", len(x), "matched:", int(((fl & 8) != 0).sum()), "kept:", int(((fl & 2) != 0).sum()), "refused by the guard:", int(refused.sum()))
    assert ((fl & 8) != 0).sum() > len(x) // 4 and ((fl & 2) != 0).sum() > len(x) // 8
    assert refused.mean() < 0.01
    ok = ~refused
    assert np.array_equal((fl[ok] >> 0) & 1, (fl[ok] >> 1) & 1) and np.array_equal((fl[ok] >> 2) & 1, (fl[ok] >> 3) & 1)
    assert np.array_equal(bits(oi[ok]), bits(og[ok]))


def test_fits_outside_the_range_are_refused(ctx, real_fits):
    """The real neighbour sets with a coordinate outside the range -- the floor moved to z = 0 exactly; everything scaled by
    2^-40, by 2^40; one coordinate a NaN, an infinity: the plane fit's guard refuses every one of them (the sweep kernels then
    fit again), and the line fit, whose divisions fall back one group at a time, equals the general one to the bit."""
    nb, x = real_fits[1]
    nb, x = nb[:512].copy(), x[:512].copy()
    cases = []
    flat = nb.copy()
    flat[:, :, 2] = 0.0
    cases.append(("z = 0", flat, x))
    cases.append(("2^-40", nb * np.float32(2.0 ** -40), x * np.float32(2.0 ** -40)))
    cases.append(("2^40", nb * np.float32(2.0 ** 40), x * np.float32(2.0 ** 40)))
    for bad in (np.nan, np.inf):
        c = nb.copy()
        c[:, 3, 1] = bad
        cases.append((str(bad), c, x))
    for name, cn, cx in cases:
        _, _, fl = fits(ctx, cn, cx, 1)
        assert np.all((fl & 16) != 0), name
    nbc, xc = real_fits[0]
    nbc, xc = nbc[:512], xc[:512]
    for s in (2.0 ** -40, 2.0 ** -20, 2.0 ** 20, 2.0 ** 40):
        oi, og, fl = fits(ctx, nbc * np.float32(s), xc * np.float32(s), 0)
        assert np.array_equal((fl >> 0) & 5, (fl >> 1) & 5), s
        assert np.array_equal(bits(oi), bits(og)), s


def carried_state(ctx, n_points):
    q = np.zeros((n_points, 4), np.float32)
    lb = np.zeros(n_points, np.float32)
    n = ctx.lib.lslam_debug_cert_state(ctx.h, q.ctypes.data_as(FP), lb.ctypes.data_as(FP), n_points)
    assert n == n_points, (n, n_points)
    return q, lb


def batch_of_three(c, synth, pr, scans, ab=0, search_mode=None):
    inits = np.stack([synth.perturb_pose(pr["gt_pose"], seed=70 + k, dt=0.1 + 0.1 * k, dr_deg=0.5 + 0.5 * k) for k in range(3)])
    c.map_set(pr["map_corner"], pr["map_surf"])
    c.scan_set_batch(scans)
    o = c.default_opts()
    if search_mode is not None:
        o.search_mode = search_mode
    o.ab_switches = ab
    for _ in range(3):  # (a call sizes its first launches from the calls before it: tests/test_gpu_queue_lean.py)
        c.run_batch(inits, o)
    before = c.fit_inrange_launches(), c.grid_lean_launches()
    rc, poses, st = c.run_batch(inits, o)
    after = c.fit_inrange_launches(), c.grid_lean_launches()
    n = sum(len(a) + len(b) for a, b in scans)
    return int(rc), poses.copy(), [stats_but_times(s) for s in st], carried_state(c, n), (after[0] - before[0], after[1] - before[1])


@pytest.mark.parametrize("search", ["auto", "grid"])
def test_switch_on_and_off(pkg, synth, small_problem, monkeypatch, search):
    """Three 16 x 1800 scans on a context made with LSLAM_FIT_INRANGE=1 and on one made with =0, through the default search
    (AUTO: a batch this small stays with the per-lane tree sweep, which has no lean kernel -- nothing may change) and through the
    grid sweep (every lean launch takes the in-range instantiation with the switch on, none with it off): poses, every stats
    field but the two times and the bytes the sweeps carry per point are equal."""
    pr = small_problem
    scans = []
    for k in range(3):
        corner, surf, _ = synth.make_scan(pr["world"], 16, 1800, gt_pose=tuple(float(v) for v in pr["gt_pose"]), seed=500 + k)
        scans.append((corner, surf))
    mode = GRID if search == "grid" else None
    res = {}
    for switch in ("1", "0"):  # a context of its own each: what a sweep does not write of the carried arrays is the context's history
        monkeypatch.setenv("LSLAM_FIT_INRANGE", switch)
        c = pkg.Context(0)
        try:
            res[switch] = batch_of_three(c, synth, pr, scans, search_mode=mode)
        finally:
            c.close()
    on, off = res["1"], res["0"]
    print(search, "in-range / lean launches, on:", on[4], "off:", off[4])
    assert on[4][0] == on[4][1] and off[4] == (0, on[4][1])
    if search == "grid":
        assert on[4][1] > 0
    assert on[0] == off[0]
    assert np.array_equal(bits(on[1]), bits(off[1]))
    assert on[2] == off[2]
    if search == "grid":  # (the per-lane sweep of a batch this small writes neither array: what is read back there is whatever the allocation held)
        # prev_q, every point's; the hint array beside it is written for listed points only: the rest is the allocation's, per context
        assert np.array_equal(bits(on[3][0]), bits(off[3][0]))
    assert all(dict(s)["sweeps"] >= 2 for s in on[2])


def test_a_floor_at_zero_takes_the_fallback(ctx, synth, small_problem, real_fits):
    """The small map with its floor moved to z = 0 exactly: the third column of every floor fit is zero, outside the range, so
    those wavefronts fit again with `/` and sqrtf -- and the lean kernels still equal the general ones (ab_switches 256) in
    poses, stats and carried bytes."""
    pr = dict(small_problem)
    ms = np.array(pr["map_surf"], np.float32, copy=True)
    floor = np.abs(ms[:, 2]) < 0.1
    assert floor.sum() > 1000
    ms[floor, 2] = 0.0
    pr["map_surf"] = ms
    scans = [(pr["corner"], pr["surf"])] * 3
    lean = batch_of_three(ctx, synth, pr, scans, ab=0, search_mode=GRID)
    gen = batch_of_three(ctx, synth, pr, scans, ab=AB_GRID_GENERAL, search_mode=GRID)
    assert lean[4][0] > 0 and lean[4][0] == lean[4][1] and gen[4] == (0, 0)
    assert lean[0] == gen[0]
    assert np.array_equal(bits(lean[1]), bits(gen[1]))
    assert lean[2] == gen[2]
    assert np.array_equal(bits(lean[3][0]), bits(gen[3][0])) and np.array_equal(bits(lean[3][1]), bits(gen[3][1]))
    assert sum(dict(s)["n_plane"] for s in lean[2]) > 0
    # ... and the guard does refuse such fits: five floor points under one scan point
    five = ms[floor][:5 * 64].reshape(-1, 5, 4).copy()
    five[:, :, 3] = 0.0
    _, _, fl = fits(ctx, five, np.tile(np.array([[1.0, 2.0, 1.5, 0.0]], np.float32), (len(five), 1)), 1)
    assert np.all((fl & 16) != 0)
