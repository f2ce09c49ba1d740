"""Joint LiDAR + stereo system (BASELINE configs[4]) on the device, through the C ABI, against the
oracle.  PARITY UNPINNED against the reference (it has no code for the visual term): the oracle is
checked by tests/test_oracle_stereo.py against a float64 finite-difference statement of the model.

Tolerances: the rows are fp32 on both sides with the same operation order up to the accumulation
(sequential fp32 in the oracle, one MFMA chain per wavefront + fp64 across blocks on the device), so
the sums are held, entry by entry, to the float64 sum of the ORACLE's rows: within K_s = 194 units
u[k] = 2**-24 * sum |r_i r_j| (tests/scanmatch_ref.py: derived from the chain's length, above ten times
the measured pairwise-fp32 floor of 2.0) -- at the near-identity pose and at two tilted poses of the
general family, landmarks drawn in the camera's view at each.  Counters exact, poses within
1e-4 m / 1e-5 rad (the north-star bar)."""
import importlib
import threading

import numpy as np
import pytest

import scanmatch_ref
from test_oracle_stereo import default_cam
from test_scanmatch_ref import stereo_cases

pytestmark = pytest.mark.gpu

synth = importlib.import_module("the-cooper-mapper_amd.synth")


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def gpu_cam(ctx, ocam):
    cam = ctx.default_stereo_cam()
    for f, _ in type(ocam)._fields_:
        setattr(cam, f, getattr(ocam, f))
    return cam


@pytest.fixture(scope="module")
def case(small_problem):
    pr = small_problem
    pts = np.concatenate([pr["map_corner"], pr["map_surf"]])
    return synth.make_stereo(pts, pr["gt_pose"], n=1500)


@pytest.fixture(scope="module")
def posed_cases(small_problem):
    return stereo_cases(small_problem)  # the near-identity pose (= `case` at the pose below) and two tilted family poses


def assert_stereo_sums_per_entry(got, oracle, lm, ob, w, ocam, pose, label):
    """Counters equal the oracle's; each of the 27 sums within K_s units of the float64 sum of the oracle's rows."""
    ref, rows = oracle.stereo_sums(lm, ob, w, ocam, pose, want_rows=True)
    assert int(got[27]) == int(ref[27]) and int(got[31]) == int(ref[28]), label
    assert got[28] == 0 and got[29] == 0 and got[30] == 0, label
    S, u = scanmatch_ref.stereo_sums64(rows)
    un = scanmatch_ref.units(got, S, u)
    assert un.max() <= scanmatch_ref.K_S, (label, "entry %d: %.1f units" % (un.argmax(), un.max()), un.round(1).tolist())
    return float(un.max()), int(ref[28])


@pytest.mark.parametrize("gate", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 257, None])
def test_stereo_sums_match_oracle(ctx, oracle, small_problem, case, posed_cases, gate, n):
    ocam = default_cam(gate_outliers=gate, weight=1.0)
    assert np.array_equal(posed_cases[0][1], case[0])  # the first case is the one this test has always used
    worst = 0.0
    for name, lm, ob, w, pose in posed_cases:
        lm, ob, w = lm[:n], ob[:n], w[:n]
        ctx.stereo_set(lm, ob, w, gpu_cam(ctx, ocam))
        got = ctx.stereo_sums(pose)
        ctx.stereo_clear()
        un, used = assert_stereo_sums_per_entry(got, oracle, lm, ob, w, ocam, pose, (name, gate, n))
        worst = max(worst, un)
    print("gate %d n %s: max %.2f units (K_s = %.0f)" % (gate, n, worst, scanmatch_ref.K_S))


def test_default_cam_and_argument_checks(pkg, ctx):
    cam = ctx.default_stereo_cam()
    assert cam.fx == 700.0 and abs(cam.huber_stereo ** 2 - 7.815) < 1e-4 and abs(cam.huber_mono ** 2 - 5.991) < 1e-4
    with pytest.raises(pkg.LslamError):
        ctx.stereo_sums(np.zeros(6))  # nothing set
    bad = ctx.default_stereo_cam()
    bad.fx = 0.0
    with pytest.raises(pkg.LslamError):
        ctx.stereo_set(np.zeros((1, 3)), np.zeros((1, 3)), None, bad)
    ctx.stereo_set(np.zeros((0, 3)), np.zeros((0, 3)))  # n = 0: clears


def test_joint_scan_match_matches_oracle(ctx, oracle, small_problem, case):
    pr = small_problem
    lm, ob, w = case
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    s0, pose0, st0 = ctx.scanmatch_scan(pr["corner"], pr["surf"], pr["init_pose"])
    # weight 0: zero rows join the sums -> the LiDAR-only pose bit for bit, more rows counted
    ctx.stereo_set(lm, ob, w, gpu_cam(ctx, default_cam(weight=0.0)))
    sz, posez, stz = ctx.scanmatch_scan(pr["corner"], pr["surf"], pr["init_pose"])
    assert np.array_equal(bits(posez), bits(pose0)) and stz.iterations == st0.iterations and stz.n_rows > st0.n_rows
    for weight, gate in ((1e-3, 0), (1e-2, 0), (1e-3, 1)):
        ocam = default_cam(weight=weight, gate_outliers=gate)
        ctx.stereo_set(lm, ob, w, gpu_cam(ctx, ocam))
        s, pose, st = ctx.scanmatch_scan(pr["corner"], pr["surf"], pr["init_pose"])
        ok, opose, ost, used = oracle.scanmatch_joint(pr["map_corner"], pr["map_surf"], pr["corner"], pr["surf"],
                                                      lm, ob, w, ocam, pr["init_pose"])
        assert st.iterations == ost.iterations and st.converged == ost.converged
        # the two poses differ in the last bits from the first joint solve on: a borderline fit may flip
        assert abs(st.n_line - ost.n_line) <= 2 and abs(st.n_plane - ost.n_plane) <= 2 and abs(st.n_rows - ost.n_rows) <= 6
        assert np.abs(pose[3:] - opose[3:]).max() <= 1e-4 and np.abs(pose[:3] - opose[:3]).max() <= 1e-5
        assert not np.array_equal(bits(pose), bits(pose0))
    ctx.stereo_clear()
    s1, pose1, st1 = ctx.scanmatch_scan(pr["corner"], pr["surf"], pr["init_pose"])
    assert np.array_equal(bits(pose1), bits(pose0))  # cleared: back to the LiDAR-only loop


def test_stereo_carries_a_scan_with_too_few_lidar_rows(ctx, oracle, small_problem, case):
    pr = small_problem
    lm, ob, w = case
    qc, qs = pr["corner"][:5], pr["surf"][:20]
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    s0, pose0, st0 = ctx.scanmatch_scan(qc, qs, pr["init_pose"])
    assert st0.iterations == 0 and int(s0) == 5  # LSLAM_TOO_FEW_MATCHES
    ocam = default_cam(weight=1e-2)
    ctx.stereo_set(lm, ob, w, gpu_cam(ctx, ocam))
    opts = ctx.default_opts()
    opts.max_iterations = 20
    s, pose, st = ctx.scanmatch_scan(qc, qs, pr["init_pose"], opts)
    oopts = oracle.default_opts()
    oopts.max_iterations = 20
    ok, opose, ost, used = oracle.scanmatch_joint(pr["map_corner"], pr["map_surf"], qc, qs, lm, ob, w, ocam,
                                                  pr["init_pose"], oopts)
    ctx.stereo_clear()
    assert st.iterations == ost.iterations > 0
    assert np.abs(pose[3:] - opose[3:]).max() <= 1e-4 and np.abs(pose[:3] - opose[:3]).max() <= 1e-5


def test_batch_with_stereo_is_refused(pkg, ctx, small_problem, case):
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set_batch([(pr["corner"], pr["surf"]), (pr["corner"], pr["surf"])])
    ctx.stereo_set(*case)
    with pytest.raises(pkg.LslamError):
        ctx.run_batch(np.stack([pr["init_pose"], pr["init_pose"]]))
    ctx.stereo_clear()
    ctx.run_batch(np.stack([pr["init_pose"], pr["init_pose"]]))


def test_sharded_joint_two_ranks(pkg, ctx, small_problem, case):
    """configs[4] at N>1: every rank holds a shard of the scan points AND of the observations; the
    stereo sums ride in the same 32-double all-reduce (a local sum stands in for RCCL here)."""
    import torch
    pr = small_problem
    lm, ob, w = case
    cam = gpu_cam(ctx, default_cam(weight=1e-3))
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.stereo_set(lm, ob, w, cam)
    status, pose, st = ctx.scanmatch_scan(pr["corner"], pr["surf"], pr["init_pose"])
    ctx.stereo_clear()
    dist = importlib.import_module("the-cooper-mapper_amd.dist")
    world = 2
    xs = [torch.zeros(32, dtype=torch.float64, device="cuda") for _ in range(world)]
    bar = threading.Barrier(world)
    out, err = [None] * world, []

    def rank_main(r):
        try:
            c = pkg.Context(0)
            c.map_set(pr["map_corner"], pr["map_surf"])
            cb, ce = dist.shard_range(len(pr["corner"]), r, world)
            sb, se = dist.shard_range(len(pr["surf"]), r, world)
            ob_, oe = dist.shard_range(len(lm), r, world)
            c.scan_set(pr["corner"][cb:ce], pr["surf"][sb:se])
            c.stereo_set(lm[ob_:oe], ob[ob_:oe], w[ob_:oe], cam)

            def allreduce(ptr, n):
                bar.wait()
                if r == 0:
                    tot = xs[0] + xs[1]
                    xs[0].copy_(tot)
                    xs[1].copy_(tot)
                    torch.cuda.synchronize()
                bar.wait()
            out[r] = c.run_sharded(pr["init_pose"], allreduce, xs[r])
            c.close()
        except Exception as e:  # pragma: no cover
            err.append(e)
            bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for r in range(world):
        s2, p2, st2 = out[r]
        assert st2.iterations == st.iterations and st2.n_rows == st.n_rows
        assert np.abs(p2[3:] - pose[3:]).max() <= 1e-5 and np.abs(p2[:3] - pose[:3]).max() <= 1e-6
    assert np.array_equal(bits(out[0][1]), bits(out[1][1]))
