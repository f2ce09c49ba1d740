"""CPU-side checks of the survey-cloud extractor's surface (lslam_survey_*, lslam_voxel_grid_min, the stage taps): declared,
exported and bound; the defaults are the reference's literals; struct layouts as the C compiler's; the C++ mirror compiles;
the command line refuses a missing file before it touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SURVEY = ["lslam_survey_default_params", "lslam_survey_extract", "lslam_survey_extract_file", "lslam_survey_info", "lslam_survey_get",
          "lslam_survey_save", "lslam_survey_destroy", "lslam_voxel_grid_min", "lslam_debug_survey_normals", "lslam_debug_survey_knn",
          "lslam_debug_survey_region", "lslam_debug_survey_boundary"]


def _capi():
    from importlib import import_module
    return import_module("the-cooper-mapper_amd.capi")


def test_survey_entry_points_are_declared_exported_and_listed(pkg):
    capi = _capi()
    txt = open(os.path.join(ROOT, "include", "lslam_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(lslam_(?:debug_)?survey_[a-z0-9_]+|lslam_voxel_grid_min)\s*\(", code))
    assert declared == set(SURVEY)
    lib = capi.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(lslam_(?:debug_)?survey_[a-z0-9_]+|lslam_voxel_grid_min)\b", exported)) == set(SURVEY)
    for name in SURVEY:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert "#define LSLAM_ABI_VERSION 7" in txt and abs(lib.lslam_abi_version()) == 7  # no existing struct changed: the version stays
    assert pkg.survey_map is not None and "SurveyMap" in pkg.__all__


def test_default_params_are_the_reference_literals(pkg):
    capi = _capi()
    lib = capi.load_library()
    images = []
    for fill in (0xFF, 0x5A):  # every byte is written
        p = capi.LslamSurveyParams()
        C.memset(C.byref(p), fill, C.sizeof(p))
        lib.lslam_survey_default_params(C.byref(p))
        images.append(bytes(C.string_at(C.byref(p), C.sizeof(p))))
    assert images[0] == images[1]
    # feature_extracter.cpp:50-56,68,88,110-111; pcl_util.h:133,138,160-168
    assert (p.partition_leaf, p.partition_min_points) == (50.0, 1000)
    assert (p.filter_leaf, p.filter_min_points, p.normal_radius) == (np.float32(0.05), 3, np.float32(0.05))
    assert (p.knn_k, p.cluster_min, p.cluster_max, p.curvature_threshold) == (60, 50, 1000000, 1.0)
    assert p.smoothness_angle == np.float32(3.0 / 180.0 * np.pi)
    assert p.boundary_radius == np.float32(0.1) and p.boundary_angle == 3.14159 / 2.0 * 0.9
    assert (p.feature_leaf, p.feature_min_points) == (np.float32(0.2), 3)
    assert (tuple(p.cube_dims), tuple(p.cube_origin), p.cube_size) == ((21, 21, 21), (10, 5, 10), 50.0)
    assert p.knn_cell == 0.0 and p.reserved == 0
    import survey_map_ref as R
    for k, v in R.DEFAULTS.items():
        got = getattr(p, k)
        assert (tuple(got) == tuple(v)) if hasattr(got, "__len__") else (float(got) == float(np.float32(v) if k != "boundary_angle" and isinstance(v, float) else v)), k


def test_struct_sizes_equal_the_c_compilers(tmp_path):
    capi = _capi()
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lslam_c.h"\nint main(void){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(lslam_survey_params), sizeof(lslam_survey_stats), offsetof(lslam_survey_params, cube_dims), '
                   'offsetof(lslam_survey_params, knn_cell));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(capi.LslamSurveyParams), C.sizeof(capi.LslamSurveyStats), capi.LslamSurveyParams.cube_dims.offset,
                     capi.LslamSurveyParams.knn_cell.offset] == [96, 112, 64, 88]


def test_entry_points_refuse_bad_arguments(pkg):
    capi = _capi()
    lib = capi.load_library()
    h = C.c_void_p(1)
    assert lib.lslam_survey_extract(None, None, 0, 12, None, C.byref(h)) == pkg.Status.ERR_INVALID and not h.value
    assert lib.lslam_survey_extract_file(None, b"/nonexistent.pcd", None, C.byref(h)) == pkg.Status.ERR_INVALID
    st = capi.LslamSurveyStats()
    assert lib.lslam_survey_info(None, C.byref(st)) == pkg.Status.ERR_INVALID
    assert lib.lslam_survey_get(None, None, 0, None, 0) == pkg.Status.ERR_INVALID
    assert lib.lslam_survey_save(None, b"/tmp") == pkg.Status.ERR_INVALID
    n = C.c_size_t(7)
    assert lib.lslam_voxel_grid_min(None, None, 0, 16, 0.5, 3, None, 0, C.byref(n)) == pkg.Status.ERR_INVALID
    assert lib.lslam_debug_survey_knn(None, None, 0, 60, 0.0, None) == pkg.Status.ERR_INVALID
    lib.lslam_survey_destroy(None)  # a no-op, like free(NULL)


def test_cpp_mirror_compiles(pkg, tmp_path):
    """include/lslam_survey_map.hpp builds with g++ -std=c++11 -Wall -Werror; without a GPU its example reports the missing backend."""
    import torch
    exe = tmp_path / "survey_map_end_to_end"
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "survey_map_end_to_end.cpp"), "-o", str(exe),
                           "-L", libdir, "-llslam_hip", "-Wl,-rpath," + libdir])
    if not torch.cuda.is_available():
        (tmp_path / "none.bin").write_bytes(b"")
        out = subprocess.run([str(exe), str(tmp_path / "none.bin"), str(tmp_path), "4.0"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "backend unavailable" in out.stderr


def test_command_line_refuses_a_missing_file(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "feature_extracter.py"), str(tmp_path / "missing.pcd"), str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "no such file" in out.stderr and not (tmp_path / "out").exists()
