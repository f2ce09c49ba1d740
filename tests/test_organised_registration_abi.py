"""CPU-side checks of the registration node for organised clouds (lslam_oreg_*, OrganisedScanRegistration): the entry points
are declared, exported and refuse a null handle and a null context with their outputs reading "nothing"; the mirrors exist and
the C++ one compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OREG = ["lslam_oreg_create", "lslam_oreg_destroy", "lslam_oreg_imu_push", "lslam_oreg_imu_info", "lslam_oreg_imu_clear",
        "lslam_oreg_process", "lslam_oreg_cloud"]


def _capi():
    from importlib import import_module
    return import_module("the-cooper-mapper_amd.capi")


def test_oreg_entry_points_are_declared_exported_and_listed(pkg):
    capi = _capi()
    txt = open(os.path.join(ROOT, "include", "lslam_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lslam_oreg_[a-z0-9_]+)\s*\(", code))
    assert declared == set(OREG)
    assert {k for k in capi.SYMBOLS if k.startswith("lslam_oreg_")} == set(OREG)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib_path()], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("lslam_oreg_")}
    assert exported == set(OREG)
    lib = capi.load_library()
    for name in OREG:
        assert hasattr(lib, name), name
    assert "#define LSLAM_ABI_VERSION 7" in txt and abs(lib.lslam_abi_version()) == 7  # no struct changed: the version stays
    assert pkg.OrganisedScanRegistration is pkg.scan_registration.OrganisedScanRegistration
    assert "OrganisedScanRegistration" in pkg.__all__ and pkg.OrganisedScanRegistration.SYSTEM_DELAY == 2
    for method in ("handle_imu_message", "handle_imu_quaternion", "handle_cloud_message", "process", "cloud", "imu_info", "imu_clear",
                   "close"):
        assert callable(getattr(pkg.OrganisedScanRegistration, method))


def test_oreg_stats_size_equals_the_c_compilers(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lslam_c.h"\nint main(void){printf("%zu %zu %zu\\n", '
                   'sizeof(lslam_oreg_stats), offsetof(lslam_oreg_stats, n_points), offsetof(lslam_oreg_stats, bytes_down));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    S = _capi().LslamOregStats
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [C.sizeof(S), S.n_points.offset, S.bytes_down.offset]


def test_oreg_entry_points_refuse_null_handles(pkg):
    capi = _capi()
    lib = capi.load_library()
    fp = C.POINTER(C.c_float)
    pts = np.ones((2, 3, 4), np.float32)
    counts = (C.c_size_t * 4)(7, 7, 7, 7)
    trans = np.full(12, 7.0, np.float32)
    stats = capi.LslamOregStats()
    stats.sweeps, stats.n_cells, stats.n_points, stats.launches = 7, 7, 7, 7
    n = C.c_size_t(7)
    size = C.c_int32(7)
    pos, vel, la = (C.c_double * 3)(7, 7, 7), (C.c_double * 3)(7, 7, 7), (C.c_double * 3)(0, 0, 9.81)
    calls = {
        "lslam_oreg_imu_push": lambda: lib.lslam_oreg_imu_push(None, 1, 0.0, 0.0, 0.0, la),
        "lslam_oreg_imu_info": lambda: lib.lslam_oreg_imu_info(None, C.byref(size), pos, vel),
        "lslam_oreg_imu_clear": lambda: lib.lslam_oreg_imu_clear(None),
        "lslam_oreg_process": lambda: lib.lslam_oreg_process(None, pts.ctypes.data_as(C.c_void_p), 2, 3, 16, 12, 1, None, counts,
                                                             trans.ctypes.data_as(fp), C.byref(stats)),
        "lslam_oreg_cloud": lambda: lib.lslam_oreg_cloud(None, None, 0, C.byref(n), None),
    }
    assert sorted(calls) == sorted(set(OREG) - {"lslam_oreg_create", "lslam_oreg_destroy"})
    for name, call in calls.items():
        assert call() == pkg.Status.ERR_INVALID, name
        msg = lib.lslam_last_error().decode()
        assert msg.split(":")[0] == name and "null node" in msg, (name, msg)
    # outputs of a refused call read "nothing"
    assert list(counts) == [0, 0, 0, 0] and np.all(trans == 0)
    assert stats.sweeps == 0 and stats.n_cells == 0 and stats.n_points == 0 and stats.launches == 0
    assert n.value == 0 and size.value == 0 and list(pos) == [0, 0, 0] and list(vel) == [0, 0, 0]
    h = C.c_void_p(1)
    assert lib.lslam_oreg_create(None, None, 0.1, 2.5, 200, C.byref(h)) == pkg.Status.ERR_INVALID
    assert "lslam_oreg_create: null context" in lib.lslam_last_error().decode() and not h.value
    lib.lslam_oreg_destroy(None)  # a no-op, like free(NULL)


def test_pack_organised_puts_the_ring_in_the_low_half_of_the_fourth_word(pkg):
    sr = pkg.scan_registration
    xyz = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)
    ring = np.array([[0, 1, 65535], [1000, 7, 256]], np.uint16)
    cells = sr.pack_organised(xyz, ring)
    assert cells.shape == (2, 3, 4) and cells.dtype == np.float32 and np.array_equal(cells[..., :3], xyz[..., :3])
    assert np.array_equal(cells[..., 3].view(np.uint32), ring.astype(np.uint32))
    assert np.array_equal(cells.view(np.uint16).reshape(2, 3, 8)[..., 6], ring)  # the uint16 at byte 12 of a cell


def test_cpp_organised_registration_mirror_compiles(pkg, tmp_path):
    """include/lslam_pipeline.hpp with OrganisedScanRegistration builds with g++ -std=c++11 -Wall -Werror; without a GPU the
    program reports the missing backend and exits non-zero."""
    import torch
    exe = tmp_path / "organised_registration_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "organised_registration_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    if not torch.cuda.is_available():
        (tmp_path / "none.bin").write_bytes(b"")
        out = subprocess.run([str(exe), str(tmp_path / "none.bin")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "backend unavailable" in out.stderr
