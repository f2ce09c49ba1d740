"""CPU-side checks of the sliding-window local mapper (lslam_lmap_*, LaserMappingLocal): the entry points are declared,
exported and refuse a null handle; the C++ mirror compiles; the reference helper's window rule (tests/local_map_ref.py)
does what LocalFeatureMap::clean does, off-by-one included."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LMAP = ["lslam_lmap_create", "lslam_lmap_destroy", "lslam_lmap_setup_queue_distance", "lslam_lmap_setup_filter_size",
        "lslam_lmap_add_data_frame", "lslam_lmap_add_data_frame_device", "lslam_lmap_surround_to_map_counts",
        "lslam_lmap_get_surround", "lslam_lmap_info", "lslam_lmap_get_frames", "lslam_lmap_stats", "lslam_lmap_clear"]


def _capi():
    from importlib import import_module
    return import_module("the-cooper-mapper_amd.capi")


def test_lmap_entry_points_are_declared_and_listed(pkg):
    capi = _capi()
    txt = open(os.path.join(ROOT, "include", "lslam_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lslam_lmap_[a-z0-9_]+)\s*\(", code))
    assert declared == set(LMAP)
    lib = capi.load_library()
    for name in LMAP:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert "#define LSLAM_ABI_VERSION 7" in txt and abs(lib.lslam_abi_version()) == 7
    assert pkg.LocalFeatureMap is not None and pkg.LaserMappingLocal is not None


def test_lmap_entry_points_refuse_a_null_handle(pkg):
    lib = _capi().load_library()
    fp = C.POINTER(C.c_float)
    T = np.eye(4, dtype=np.float32)
    pts = np.zeros((3, 4), np.float32)
    n = C.c_size_t(7)
    m = C.c_size_t(7)
    nf = C.c_int32(7)
    calls = {
        "lslam_lmap_setup_queue_distance": lambda: lib.lslam_lmap_setup_queue_distance(None, 30.0),
        "lslam_lmap_setup_filter_size": lambda: lib.lslam_lmap_setup_filter_size(None, 0.2, 0.4),
        "lslam_lmap_add_data_frame": lambda: lib.lslam_lmap_add_data_frame(None, pts.ctypes.data_as(C.c_void_p), 3, pts.ctypes.data_as(C.c_void_p),
                                                                            3, 16, T.ctypes.data_as(fp)),
        "lslam_lmap_add_data_frame_device": lambda: lib.lslam_lmap_add_data_frame_device(None, None, 0, None, 0, T.ctypes.data_as(fp)),
        "lslam_lmap_surround_to_map_counts": lambda: lib.lslam_lmap_surround_to_map_counts(None, C.byref(n), C.byref(m)),
        "lslam_lmap_get_surround": lambda: lib.lslam_lmap_get_surround(None, None, 0, C.byref(n), None, 0, C.byref(m)),
        "lslam_lmap_info": lambda: lib.lslam_lmap_info(None, C.byref(nf), None, None, None),
        "lslam_lmap_get_frames": lambda: lib.lslam_lmap_get_frames(None, 0, C.byref(nf), None, None, None, 0, None, 0),
        "lslam_lmap_stats": lambda: lib.lslam_lmap_stats(None, None, None, None),
        "lslam_lmap_clear": lambda: lib.lslam_lmap_clear(None),
    }
    assert sorted(calls) == sorted(set(LMAP) - {"lslam_lmap_create", "lslam_lmap_destroy"})
    for name, call in calls.items():
        assert call() == pkg.Status.ERR_INVALID, name
        msg = lib.lslam_last_error().decode()
        assert name.startswith(msg.split(":")[0]) and "null local map" in msg, (name, msg)
    assert n.value == 0 and m.value == 0 and nf.value == 0  # outputs of a refused call read "nothing"
    h = C.c_void_p(1)
    assert lib.lslam_lmap_create(None, 0, 0, 0, C.byref(h)) == pkg.Status.ERR_INVALID
    assert "null ctx" in lib.lslam_last_error().decode() and not h.value
    lib.lslam_lmap_destroy(None)  # a no-op, like free(NULL)


def test_cpp_local_mapping_mirror_compiles(pkg, tmp_path):
    """include/lslam_pipeline.hpp with LaserMappingLocal / LocalFeatureMap builds with g++ -std=c++11 -Wall -Werror; without a
    GPU the program reports the missing backend and exits non-zero."""
    import torch
    exe = tmp_path / "local_mapping_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "local_mapping_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    if not torch.cuda.is_available():
        (tmp_path / "none.bin").write_bytes(b"")
        out = subprocess.run([str(exe), str(tmp_path / "none.bin")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "backend unavailable" in out.stderr


def test_reference_window_rule():
    """LocalFeatureMap::clean on hand-made accum sequences: nothing under the threshold, n + 1 erased when n qualify, everything
    (the new frame included) after one step of the threshold or more."""
    from local_map_ref import RefLocalFeatureMap, frames_to_erase
    assert frames_to_erase([0.0, 10.0, 20.0, 29.9], 29.9, 30.0) == 0
    assert frames_to_erase([0.0, 10.0, 20.0, 30.0], 30.0, 30.0) == 2          # accum 0 <= 30 - 30: one qualifies, two go
    assert frames_to_erase([0.0, 0.5, 1.0, 20.0, 31.0], 31.0, 30.0) == 4      # 0, 0.5, 1.0 qualify: four go
    assert frames_to_erase([0.0, 10.0, 20.0, 51.0], 51.0, 30.0) == 4          # three qualify: the whole queue goes
    assert frames_to_erase([5.0], 5.0, 30.0) == 0
    # through the container: poses along x, one empty cloud per frame (no oracle call is made for empty clouds)
    fm = RefLocalFeatureMap(oracle=None)
    empty = np.zeros((0, 4), np.float32)

    def at(x):
        T = np.eye(4, dtype=np.float32)
        T[0, 3] = x
        return T
    for x in (0.0, 10.0, 20.0, 29.0):
        fm.add_data_frame(empty, empty, at(x))
    assert len(fm.queue) == 4 and fm.accum == 29.0 and fm.evicted == 0
    fm.add_data_frame(empty, empty, at(31.0))       # accum 31: frame 0 (accum 0) qualifies -> frames 0 and 1 go
    assert [f[2] for f in fm.queue] == [20.0, 29.0, 31.0] and fm.evicted == 2
    fm.add_data_frame(empty, empty, at(62.0))       # a 31 m step: all three qualify -> four erased, the new frame with them
    assert fm.queue == [] and fm.accum == 62.0 and fm.evicted == 6
    c, s = fm.get_surround_feature()
    assert len(c) == 0 and len(s) == 0
    fm.add_data_frame(empty, empty, at(62.5))       # the updater is not re-armed by an empty queue: the path goes on
    assert len(fm.queue) == 1 and fm.accum == 62.5
    # a rotated previous pose: the step is measured in the previous frame, its length is the same
    fm.clear()
    R = np.eye(4, dtype=np.float32)
    R[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    fm.add_data_frame(empty, empty, R)
    R2 = R.copy()
    R2[:3, 3] = [3.0, 4.0, 0.0]
    fm.add_data_frame(empty, empty, R2)
    assert fm.accum == 5.0
