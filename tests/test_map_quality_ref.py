"""CPU-side checks of the map-quality feature (include/lslam_c.h lslam_mapq_*, lslam_traj_*): the two restatements of the
trajectory evaluation against each other and against lslam_traj_eval (host code: runs without a GPU), the ABI of the new
structs, and reference-only sanity checks of the scenes tests/test_gpu_map_quality.py uses, so that its conditions are not met
by luck."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import map_quality_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("the-cooper-mapper_amd.capi")


@pytest.fixture(scope="module")
def mq(pkg):
    return importlib.import_module("the-cooper-mapper_amd.map_quality")


def make_traj(seed=0, n_est=300, n_ref=120, outliers=3):
    rng = np.random.default_rng(seed)
    rs = np.sort(rng.uniform(0.0, 60.0, n_ref))
    es = np.sort(rng.uniform(-1.0, 61.0, n_est))
    es[5] = 0.5 * (rs[20] + rs[21])  # an exact tie in time (up to the rounding of the mean): the later sample
    path = lambda t: np.stack([2.0 * t, 30.0 * np.sin(0.1 * t), 0.05 * t], 1)
    rx = path(rs) + rng.normal(0, 0.02, (n_ref, 3))
    ex = path(es) + rng.normal(0, 0.05, (n_est, 3))
    ex[rng.choice(n_est, outliers, replace=False)] += 25.0  # beyond the 10 m gate
    return es, ex, rs, rx


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("gate", [10.0, 0.0, 0.5])
def test_the_two_trajectory_restatements_agree(gate):
    es, ex, rs, rx = make_traj()
    lit = ref.traj_literal(es, ex, rs, rx, gate)
    vec = ref.traj_vectorised(es, ex, rs, rx, gate)
    assert lit["n_used"] == vec["n_used"] and lit["n_gated"] == vec["n_gated"] and lit["n_used"] > 100
    if gate == 10.0:
        assert lit["n_gated"] == 3
    assert same(lit["max"], vec["max"])  # a maximum has no order
    # the sums differ in order only (numpy sums pairwise): n * eps * the largest term
    tol = len(es) * np.finfo(np.float64).eps
    assert np.all(np.abs(lit["mean"] - vec["mean"]) <= tol * np.maximum(lit["max"], 1.0))
    assert np.all(np.abs(lit["var"] - vec["var"]) <= 4 * tol * np.maximum(lit["max"], 1.0) ** 2)
    assert abs(lit["mean_dt"] - vec["mean_dt"]) <= tol
    # the maxima are taken before the gate: with outliers beyond it they exceed every used difference
    if lit["n_gated"]:
        assert lit["max"][3] > max(gate, 1e-9) and lit["mean"][3] <= gate


def test_the_ring_of_the_reference_forgets_old_fixes():
    """The literal restatement keeps the reference's ring: with room for 16 fixes an early estimate is paired with the oldest fix
    still held, not with its nearest."""
    es, ex, rs, rx = make_traj()
    full = ref.traj_literal(es, ex, rs, rx, 0.0)
    ring = ref.traj_literal(es, ex, rs, rx, 0.0, store_num=16)
    assert ring["n_used"] == full["n_used"] and ring["mean"][3] > 10 * full["mean"][3]


def planted(seed=3, n=80, noise=0.0, reflect=False):
    rng = np.random.default_rng(seed)
    from keyframe_store_ref import random_se3
    T = random_se3(rng, 20.0).astype(np.float64)
    R = T[:3, :3]
    R, _ = np.linalg.qr(R)  # exactly orthonormal in fp64
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    e = rng.uniform(-30, 30, (n, 3))
    if reflect:
        e[:, 2] *= 1e-3  # nearly planar, noisy: the unconstrained optimum may be a reflection
    r = e @ R.T + T[:3, 3] + rng.normal(0, noise, (n, 3)) if noise else e @ R.T + T[:3, 3]
    return e, r, R, T[:3, 3]


def test_alignment_recovers_a_planted_transform_and_refuses_collinear_input():
    e, r, R, t = planted()
    ok, R2, t2, rmse, s = ref.align(e, r)
    assert ok and np.abs(R2 - R).max() < 1e-12 and np.abs(t2 - t).max() < 1e-11 and rmse < 1e-11
    line = np.outer(np.linspace(0, 50, 40), [1.0, 2.0, -0.5])
    assert not ref.align(line, line + [1, 2, 3])[0]
    assert not ref.align(e[:2], r[:2])[0]
    # a nearly planar, noisy set: the rotation is still proper
    e, r, R, t = planted(seed=4, noise=0.05, reflect=True)
    ok, R2, _, _, _ = ref.align(e, r)
    assert ok and abs(np.linalg.det(R2) - 1.0) < 1e-12


def call_traj(mq, es, ex, rs, rx, gate=None, align=False):
    return mq.trajectory_eval(es, ex, rs, rx, gate=gate, align=align)


@pytest.mark.parametrize("gate", [None, 0.0, 0.5])
def test_lslam_traj_eval_equals_the_literal_restatement_bit_for_bit(mq, gate):
    es, ex, rs, rx = make_traj(seed=1)
    got = call_traj(mq, es, ex, rs, rx, gate)
    lit = ref.traj_literal(es, ex, rs, rx, 10.0 if gate is None else gate)
    assert got["n_used"] == lit["n_used"] and got["n_gated"] == lit["n_gated"]
    for key in ("mean", "var", "max"):
        assert same(got[key], lit[key]), key
    assert same([got["mean_dt"]], [lit["mean_dt"]])
    assert not got["aligned"] and np.isnan(got["ate_rmse"]) and np.array_equal(got["T_align"], np.eye(4))


def test_lslam_traj_eval_edge_cases(mq):
    es, ex, rs, rx = make_traj(seed=2)
    none = call_traj(mq, es[:0], ex[:0], rs, rx)
    assert none["n_used"] == 0 and np.all(np.isnan(none["mean"])) and np.all(np.isnan(none["var"])) and np.all(none["max"] == 0)
    no_ref = call_traj(mq, es, ex, rs[:0], rx[:0])
    assert no_ref["n_used"] == 0 and no_ref["n_gated"] == 0
    one = call_traj(mq, es[:1], ex[:1], rs[:1], rx[:1], gate=0.0)
    assert one["n_used"] == 1 and np.all(np.isnan(one["var"])) and np.all(np.isfinite(one["mean"]))
    gated = call_traj(mq, es, ex + 100.0, rs, rx)
    assert gated["n_used"] == 0 and gated["n_gated"] == len(es) and gated["max"][3] > 100 and np.isnan(gated["mean_dt"])
    pkg_err = importlib.import_module("the-cooper-mapper_amd.capi").LslamError
    with pytest.raises(pkg_err) as e:
        call_traj(mq, es, ex, rs, rx, gate=-1.0)
    assert "gate" in str(e.value)


def test_lslam_traj_eval_alignment_against_the_restatement(mq):
    """The aligned figures.  Bound: the library forms the SVD of the 3x3 matrix H through the eigenvectors of H^T H, which
    squares H's condition: a rotation error of order eps * (s0 / s1)^2, times the lever arm for the translation and the RMSE.
    numpy's SVD errs by eps * s0 / s1.  With C = 64 as the constant for the handful of 3x3 products on either side the test
    allows C * eps * (s0 / s1)^2 on R and that times the data's extent on t and on the RMSE."""
    for seed, noise in ((5, 0.0), (6, 0.03), (7, 0.5)):
        e, r, R, t = planted(seed=seed, noise=noise)
        stamps = np.arange(len(e), dtype=np.float64)
        got = call_traj(mq, stamps, e, stamps, r, gate=0.0, align=True)
        ok, R2, t2, rmse, s = ref.align(e, r)
        assert ok and got["aligned"]
        bound = 64 * np.finfo(np.float64).eps * (s[0] / s[1]) ** 2
        extent = np.abs(np.concatenate([e, r])).max()
        T = got["T_align"]
        print("align seed %d: |dR| %.3g (bound %.3g) |dt| %.3g |drmse| %.3g" % (seed, np.abs(T[:3, :3] - R2).max(), bound,
                                                                               np.abs(T[:3, 3] - t2).max(), abs(got["ate_rmse"] - rmse)))
        assert np.abs(T[:3, :3] - R2).max() <= bound
        assert np.abs(T[:3, 3] - t2).max() <= bound * extent
        assert abs(got["ate_rmse"] - rmse) <= bound * extent
        assert np.array_equal(T[3], [0, 0, 0, 1]) and abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
        # the unaligned figures are those of the call without alignment
        plain = call_traj(mq, stamps, e, stamps, r, gate=0.0)
        assert same(plain["mean"], got["mean"]) and same(plain["var"], got["var"])
    # a reflection would fit a nearly planar noisy set better: the library answers with a rotation, as the restatement does
    e, r, R, t = planted(seed=4, noise=0.05, reflect=True)
    stamps = np.arange(len(e), dtype=np.float64)
    got = call_traj(mq, stamps, e, stamps, r, gate=0.0, align=True)
    ok, R2, t2, rmse, s = ref.align(e, r)
    assert got["aligned"] and abs(np.linalg.det(got["T_align"][:3, :3]) - 1.0) < 1e-12
    assert np.abs(got["T_align"][:3, :3] - R2).max() <= 64 * np.finfo(np.float64).eps * (s[0] / s[1]) ** 2
    # collinear pairs, and fewer than three: no alignment, the unaligned figures only
    line = np.outer(np.linspace(0, 50, 40), [1.0, 2.0, -0.5])
    got = call_traj(mq, np.arange(40.0), line, np.arange(40.0), line + [1, 2, 3], gate=0.0, align=True)
    assert not got["aligned"] and np.isnan(got["ate_rmse"]) and np.array_equal(got["T_align"], np.eye(4)) and got["n_used"] == 40
    got = call_traj(mq, np.arange(2.0), e[:2], np.arange(2.0), r[:2], gate=0.0, align=True)
    assert not got["aligned"] and got["n_used"] == 2


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_default_params_write_every_byte(pkg, capi):
    lib = pkg.load_library()
    for cls, fn in ((capi.LslamMapqParams, lib.lslam_mapq_default_params), (capi.LslamTrajParams, lib.lslam_traj_default_params)):
        images = []
        for fill in (0xFF, 0x5A):
            p = cls()
            C.memset(C.byref(p), fill, C.sizeof(p))
            fn(C.byref(p))
            assert list(p.reserved) == [0] * len(p.reserved)
            images.append(bytes(C.string_at(C.byref(p), C.sizeof(p))))
        assert images[0] == images[1]
    p = capi.LslamMapqParams()
    lib.lslam_mapq_default_params(C.byref(p))
    assert (p.radius, p.min_neighbors, p.lambda_floor) == (np.float32(0.3), 5, 1e-8)
    t = capi.LslamTrajParams()
    lib.lslam_traj_default_params(C.byref(t))
    assert (t.gate, t.align) == (10.0, 0)


def test_struct_sizes_equal_the_c_compilers(pkg, capi, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "lslam_c.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(lslam_mapq_params),'
                   ' sizeof(lslam_mapq_stats), sizeof(lslam_traj_params), sizeof(lslam_traj_stats));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    lib = pkg.load_library()
    mirrors = [C.sizeof(capi.LslamMapqParams), C.sizeof(capi.LslamMapqStats), C.sizeof(capi.LslamTrajParams), C.sizeof(capi.LslamTrajStats)]
    assert sizes == mirrors
    assert sizes == [lib.lslam_sizeof_mapq_params(), lib.lslam_sizeof_mapq_stats(), lib.lslam_sizeof_traj_params(), lib.lslam_sizeof_traj_stats()]


def test_mapq_eval_fails_loudly_without_a_context(pkg, capi):
    """No context, no evaluation: a null ctx is refused with a named cause, and without a GPU no context can be made."""
    import torch
    lib = pkg.load_library()
    pts = np.zeros((8, 4), np.float32)
    st = capi.LslamMapqStats()
    rc = lib.lslam_mapq_eval(None, pts.ctypes.data_as(C.c_void_p), 8, 16, None, 0, 0, None, C.byref(st), None, None, None)
    assert rc == pkg.Status.ERR_INVALID and b"no context" in lib.lslam_last_error()
    assert lib.lslam_mapq_fmap(None, 1, None, C.byref(st)) < 0 and lib.lslam_mapq_keyframes(None, 0, None, None, 1, None, C.byref(st)) < 0
    if not torch.cuda.is_available():
        with pytest.raises(pkg.LslamError) as e:
            pkg.Context(0)
        assert e.value.code == pkg.Status.ERR_HIP


def test_the_trajectory_unit_compiles_without_hip(tmp_path):
    """csrc/lslam_traj.hip is plain C++: a host compiler builds it with the stand-alone program tools/cpp/traj_eval_asan.cpp."""
    exe = tmp_path / "traj"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-x", "c++", os.path.join(ROOT, "the-cooper-mapper_amd", "csrc", "lslam_traj.hip"),
                           os.path.join(ROOT, "tools", "cpp", "traj_eval_asan.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "traj_eval ok" in out.stdout, out.stdout + out.stderr


# ---- the scenes of the GPU tests, on the reference alone ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.ACCURACY_SCENES))
def test_accuracy_scenes_are_mostly_defined_with_a_sparse_point(name):
    cloud, params, (st, lam, ent, cnt) = ref.scene_reference(name)
    assert len(cloud) <= 4000
    finite = st["n_query"] - st["n_nonfinite"]
    assert st["n_defined"] >= 0.95 * finite and st["n_sparse"] >= 1, st
    assert np.all(np.diff(lam[np.isfinite(ent)], axis=1) >= 0)
    if name == "plane":  # the floor engages: l0 is exactly zero somewhere, the entropy stays finite
        assert (lam[:, 0] <= 0.0).sum() > 0.9 * st["n_defined"] and np.all(np.isfinite(ent[np.isfinite(lam[:, 0])]))
    if name == "line":
        d = np.isfinite(ent)
        assert np.all(lam[d, 1] < 1e-8) and np.all(lam[d, 2] > 1e-6)
    if name == "lattice":  # neighbours on the radius: the count of an inner point is what the strict < gives, to rounding
        r2 = float(ref.radius2(params["radius"]))
        d2 = ref.d2_f32(cloud[:729], cloud[364:365])[:, 0]  # the centre of the 9^3 lattice
        assert (np.abs(d2 - r2) < 1e-6).sum() >= 6  # the six axis neighbours at three steps, and more
        assert cnt[364] == (d2 < r2).sum()


def test_double_wall_against_single_wall_on_the_reference():
    one, _, _, _ = ref.evaluate(ref.two_walls(0.0), radius=0.3)
    two, _, _, _ = ref.evaluate(ref.two_walls(0.2), radius=0.3)
    print("MPV single %.3g double %.3g; MME single %.4f double %.4f" % (one["mean_plane_variance"], two["mean_plane_variance"],
                                                                         one["mean_entropy"], two["mean_entropy"]))
    assert 0.5e-4 < one["mean_plane_variance"] < 2e-4  # sigma^2 = 1e-4
    assert two["mean_plane_variance"] >= 10 * one["mean_plane_variance"]
    assert two["mean_entropy"] > one["mean_entropy"]


def test_displaced_keyframe_on_the_reference():
    clouds, poses, moved = ref.keyframe_scene()
    good, _, _, _ = ref.evaluate(ref.assemble(clouds, poses), radius=0.3)
    bad, _, _, _ = ref.evaluate(ref.assemble(clouds, moved), radius=0.3)
    print("MPV true poses %.3g, one keyframe displaced %.3g" % (good["mean_plane_variance"], bad["mean_plane_variance"]))
    assert good["n_defined"] >= 0.95 * good["n_query"] and bad["n_defined"] >= 0.95 * bad["n_query"]
    assert good["mean_plane_variance"] <= 0.1 * bad["mean_plane_variance"]
