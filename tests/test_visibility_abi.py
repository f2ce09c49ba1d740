"""The visibility votes' boundary without a GPU: header, ctypes binding and library agree on the new symbols and on the two
structs' sizes; the defaults are the documented ones and write every byte; the ABI version stays 7; null handles are refused."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIS_SYMBOLS = {"lslam_vis_default_params", "lslam_sizeof_vis_params", "lslam_sizeof_vis_stats", "lslam_vis_setup", "lslam_vis_info",
               "lslam_vis_range_image", "lslam_vis_votes", "lslam_vis_votes_device", "lslam_vis_filter_device", "lslam_vis_add_to_fmap",
               "lslam_debug_vis_votes"}


def _capi():
    return __import__("importlib").import_module("the-cooper-mapper_amd.capi")


def test_every_visibility_symbol_is_declared_exported_and_bound(pkg):
    from test_abi import header_symbols
    capi = _capi()
    assert {s for s in header_symbols() if "_vis_" in s} == VIS_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.lib_path()], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if re.search(r"\blslam\w*_vis_", l)} == VIS_SYMBOLS
    assert {s for s in capi.SYMBOLS if "_vis_" in s} == VIS_SYMBOLS
    lib = pkg.load_library()
    assert lib.lslam_abi_version() == 7
    txt = open(os.path.join(ROOT, "include", "lslam_c.h")).read()
    assert re.search(r"#define LSLAM_ABI_VERSION 7\b", txt)
    # the kernel's shape is exported for the tests that straddle it, and the Python mirror states the same numbers
    tile, chunk = (int(re.search(r"#define %s (\d+)" % n, txt).group(1)) for n in ("LSLAM_VIS_POINT_TILE", "LSLAM_VIS_KF_CHUNK"))
    assert (tile, chunk) == (pkg.visibility.POINT_TILE, pkg.visibility.KF_CHUNK)


def test_struct_sizes_equal_the_c_compilers_and_the_librarys(pkg, tmp_path):
    capi = _capi()
    lib = pkg.load_library()
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lslam_c.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(lslam_vis_params), sizeof(lslam_vis_stats), offsetof(lslam_vis_params, up_axis), '
                   'offsetof(lslam_vis_stats, is_set), offsetof(lslam_vis_stats, vote_launches));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(capi.LslamVisParams), C.sizeof(capi.LslamVisStats), capi.LslamVisParams.up_axis.offset,
                     capi.LslamVisStats.is_set.offset, capi.LslamVisStats.vote_launches.offset]
    assert sizes[:2] == [44, 80]
    assert lib.lslam_sizeof_vis_params() == 44 and lib.lslam_sizeof_vis_stats() == 80


def test_defaults_are_the_documented_ones_and_write_every_byte(pkg):
    import visibility_ref as V
    capi = _capi()
    lib = pkg.load_library()
    images = []
    for fill in (0xFF, 0x5A):
        p = capi.LslamVisParams()
        C.memset(C.byref(p), fill, C.sizeof(p))
        lib.lslam_vis_default_params(C.byref(p))
        assert (p.n_row, p.n_col, p.window, p.min_free_votes, p.up_axis) == (16, 360, 1, 2, 1)
        assert (p.fov_down_deg, p.fov_up_deg, p.min_range, p.max_range) == (-16.0, 16.0, 1.0, 80.0)
        assert p.abs_margin == 0.5 and p.rel_margin == np.float32(0.02)
        images.append(bytes(C.string_at(C.byref(p), C.sizeof(p))))
    assert images[0] == images[1]
    lib.lslam_vis_default_params(None)  # a no-op
    q = pkg.visibility.vis_params()
    assert set(V.DEFAULTS) == set(pkg.visibility.PARAM_FIELDS)
    for k, v in V.DEFAULTS.items():  # the reference's defaults are the library's
        assert np.float32(getattr(q, k)) == np.float32(v), k


def test_null_handles_are_refused_and_the_outputs_are_left_alone(pkg):
    capi = _capi()
    lib = pkg.load_library()
    INVALID = int(pkg.Status.ERR_INVALID)
    ids, T = np.zeros(1, np.int32), np.eye(4, dtype=np.float32).reshape(1, 16)
    ip, fp = ids.ctypes.data_as(C.POINTER(C.c_int32)), T.ctypes.data_as(C.POINTER(C.c_float))
    pts = np.ones((3, 4), np.float32)
    votes = np.full(3, 0xA5A5A5A5, np.uint32)
    assert lib.lslam_vis_setup(None, None) == INVALID
    assert "null keyframe store" in lib.lslam_last_error().decode()
    assert lib.lslam_vis_votes(None, 1, ip, fp, pts.ctypes.data_as(C.c_void_p), 3, 16, votes.ctypes.data_as(C.POINTER(C.c_uint32))) == INVALID
    assert "null keyframe store" in lib.lslam_last_error().decode()
    assert (votes == 0xA5A5A5A5).all()  # a refused call changes nothing, the caller's output included
    assert lib.lslam_vis_votes_device(None, 1, ip, fp, None, 0, None) == INVALID
    kept = C.c_size_t(77)
    assert lib.lslam_vis_filter_device(None, 1, ip, fp, None, 0, None, C.byref(kept)) == INVALID and kept.value == 77
    removed = (C.c_size_t * 2)(5, 6)
    assert lib.lslam_vis_add_to_fmap(None, 0, None, fp, 1, ip, fp, removed) == INVALID and tuple(removed) == (5, 6)
    img = np.full(4, 3.0, np.float32)
    assert lib.lslam_vis_range_image(None, 0, img.ctypes.data_as(C.POINTER(C.c_float))) == INVALID and (img == 3.0).all()
    assert lib.lslam_debug_vis_votes(None, 1) == INVALID
    st = capi.LslamVisStats()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    assert lib.lslam_vis_info(None, C.byref(st)) == INVALID
    assert bytes(C.string_at(C.byref(st), C.sizeof(st))) == bytes(C.sizeof(st))  # zeroed, as lslam_sc_info does


def test_python_parameters_refuse_unknown_names(pkg):
    with pytest.raises(TypeError):
        pkg.visibility.vis_params(n_rows=16)
    p = pkg.visibility.vis_params(dict(n_col=900), window=0, up_axis=2)
    assert (p.n_col, p.window, p.up_axis, p.n_row) == (900, 0, 2, 16)
    assert pkg.visibility.vis_params(p).n_col == 900
    nf, nh = pkg.visibility.split_votes(np.array([3 | (2 << 16)], np.uint32))
    assert (nf.tolist(), nh.tolist()) == ([3], [2])
    assert pkg.visibility.dynamic_mask(np.array([2, 1, 2 | (2 << 16)], np.uint32), 2).tolist() == [True, False, False]


def test_graph_refuses_remove_dynamic_without_a_resident_store(pkg):
    """Checked before anything is created: no device needed."""
    with pytest.raises(ValueError, match="remove_dynamic"):
        pkg.Graph(remove_dynamic=True)
