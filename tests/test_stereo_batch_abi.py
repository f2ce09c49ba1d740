"""CPU-side checks of the joint batch entry points (lslam_stereo_set_batch / _sums_batch): declared, exported, and a NULL
context is an error, not a crash."""
import ctypes as C

import numpy as np


def test_stereo_batch_entry_points_refuse_a_null_context(pkg):
    from importlib import import_module
    capi = import_module("the-cooper-mapper_amd.capi")
    assert "lslam_stereo_set_batch" in capi.SYMBOLS and "lslam_stereo_sums_batch" in capi.SYMBOLS
    lib = capi.load_library()
    cam = capi.LslamStereoCam()
    lib.lslam_stereo_default_cam(C.byref(cam))
    lm = np.zeros((2, 3), np.float32)
    fp = C.POINTER(C.c_float)
    offsets = (C.c_size_t * 3)(0, 1, 2)
    rc = lib.lslam_stereo_set_batch(None, 2, lm.ctypes.data_as(fp), lm.ctypes.data_as(fp), None, offsets, C.byref(cam))
    assert rc == pkg.Status.ERR_INVALID
    assert "null ctx" in lib.lslam_last_error().decode()
    poses = np.zeros((2, 6), np.float32)
    sums = np.zeros((2, 32))
    rc = lib.lslam_stereo_sums_batch(None, 2, poses.ctypes.data_as(fp), sums.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == pkg.Status.ERR_INVALID
    assert not sums.any()
