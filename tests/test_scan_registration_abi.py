"""CPU-side checks of the registration node (lslam_sreg_*, MultiScanRegistration): the entry points are declared, exported
and refuse a null handle and a null context with their outputs reading "nothing"; the mirrors exist and the C++ one compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SREG = ["lslam_sreg_create", "lslam_sreg_destroy", "lslam_sreg_imu_push", "lslam_sreg_imu_info", "lslam_sreg_imu_clear",
        "lslam_sreg_process", "lslam_sreg_cloud"]


def _capi():
    from importlib import import_module
    return import_module("the-cooper-mapper_amd.capi")


def test_sreg_entry_points_are_declared_and_listed(pkg):
    capi = _capi()
    txt = open(os.path.join(ROOT, "include", "lslam_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lslam_sreg_[a-z0-9_]+)\s*\(", code))
    assert declared == set(SREG)
    lib = capi.load_library()
    for name in SREG:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert "#define LSLAM_ABI_VERSION 7" in txt and abs(lib.lslam_abi_version()) == 7  # no struct changed: the version stays
    assert pkg.MultiScanRegistration is pkg.scan_registration.MultiScanRegistration
    for method in ("handle_imu_message", "handle_imu_quaternion", "handle_cloud_message", "process", "cloud", "imu_clear"):
        assert callable(getattr(pkg.MultiScanRegistration, method))


def test_sreg_stats_size_equals_the_c_compilers(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "lslam_c.h"\nint main(void){printf("%zu\\n", sizeof(lslam_sreg_stats));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)], text=True)) == C.sizeof(_capi().LslamSregStats)


def test_sreg_entry_points_refuse_null_handles(pkg):
    capi = _capi()
    lib = capi.load_library()
    fp = C.POINTER(C.c_float)
    pts = np.ones((3, 4), np.float32)
    counts = (C.c_size_t * 4)(7, 7, 7, 7)
    trans = np.full(12, 7.0, np.float32)
    stats = capi.LslamSregStats()
    stats.sweeps, stats.n_points = 7, 7
    n = C.c_size_t(7)
    size = C.c_int32(7)
    pos, vel, la = (C.c_double * 3)(7, 7, 7), (C.c_double * 3)(7, 7, 7), (C.c_double * 3)(0, 0, 9.81)
    calls = {
        "lslam_sreg_imu_push": lambda: lib.lslam_sreg_imu_push(None, 1, 0.0, 0.0, 0.0, la),
        "lslam_sreg_imu_info": lambda: lib.lslam_sreg_imu_info(None, C.byref(size), pos, vel),
        "lslam_sreg_imu_clear": lambda: lib.lslam_sreg_imu_clear(None),
        "lslam_sreg_process": lambda: lib.lslam_sreg_process(None, pts.ctypes.data_as(C.c_void_p), 3, 16, 1, None, counts,
                                                             trans.ctypes.data_as(fp), C.byref(stats)),
        "lslam_sreg_cloud": lambda: lib.lslam_sreg_cloud(None, None, 0, C.byref(n), None),
    }
    assert sorted(calls) == sorted(set(SREG) - {"lslam_sreg_create", "lslam_sreg_destroy"})
    for name, call in calls.items():
        assert call() == pkg.Status.ERR_INVALID, name
        msg = lib.lslam_last_error().decode()
        assert msg.split(":")[0] == name and "null node" in msg, (name, msg)
    # outputs of a refused call read "nothing"
    assert list(counts) == [0, 0, 0, 0] and np.all(trans == 0) and stats.sweeps == 0 and stats.n_points == 0
    assert n.value == 0 and size.value == 0 and list(pos) == [0, 0, 0] and list(vel) == [0, 0, 0]
    h = C.c_void_p(1)
    assert lib.lslam_sreg_create(None, None, -15.0, 15.0, 16, 0.1, 200, C.byref(h)) == pkg.Status.ERR_INVALID
    assert "lslam_sreg_create: null context" in lib.lslam_last_error().decode() and not h.value
    lib.lslam_sreg_destroy(None)  # a no-op, like free(NULL)


def test_rpy_from_quaternion_is_tfs_first_solution(pkg):
    """getRPY's default solution: pitch in [-pi/2, pi/2]; composing Rz(yaw) Ry(pitch) Rx(roll) gives the rotation back."""
    rng = np.random.default_rng(2)
    for _ in range(50):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        x, y, z, w = q
        Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        r, p, yw = pkg.scan_registration.rpy_from_quaternion(x, y, z, w)
        assert -np.pi / 2 <= p <= np.pi / 2
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(yw), np.sin(yw)
        Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
        Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
        Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
        assert np.abs(Rz @ Ry @ Rx - Rq).max() <= 1e-12


def test_cpp_registration_mirror_compiles(pkg, tmp_path):
    """include/lslam_pipeline.hpp with MultiScanRegistration builds with g++ -std=c++11 -Wall -Werror; without a GPU the
    program reports the missing backend and exits non-zero."""
    import torch
    exe = tmp_path / "registration_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "registration_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    if not torch.cuda.is_available():
        (tmp_path / "none.bin").write_bytes(b"")
        out = subprocess.run([str(exe), str(tmp_path / "none.bin")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "backend unavailable" in out.stderr
