"""Host-side mirror of the reference's ``featureExtracter`` executable (io_module/feature_extracter.cpp over util/pcl_util.h and
util/voxel_grid_partition.hpp) on ``lslam_survey_*`` (``csrc/lslam_survey.hip``, include/lslam_c.h): a dense survey cloud
becomes the corner / surf cube map that :class:`~.laser_localization.LaserLocalization` loads.

``extract(ctx, cloud)`` returns a :class:`SurveyMap` whose clouds stay on the device; ``save(directory)`` writes ``index.txt``
and ``<count>.pcd`` as ``lslam_fmap_save`` does.  The ``debug_*`` functions are the stage taps the tests use.  ROS parameters
are not mirrored; ``extract_file`` reads its PCD through the library's reader (ascii or binary).
"""
import ctypes as C

import numpy as np

from .capi import LslamError, LslamSurveyParams, LslamSurveyStats, c_int32_p, c_uint8_p
from .feature_map import _fp, _xyzi


def default_params(lib):
    p = LslamSurveyParams()
    lib.lslam_survey_default_params(C.byref(p))
    return p


def make_params(lib, **kw):
    """The reference's literals with some replaced: scalar fields by name, ``cube_dims`` / ``cube_origin`` as triples."""
    p = default_params(lib)
    for k, v in kw.items():
        if k in ("cube_dims", "cube_origin"):
            for d in range(3):
                getattr(p, k)[d] = int(v[d])
        elif not hasattr(p, k):
            raise TypeError("lslam_survey_params has no field %r" % k)
        else:
            setattr(p, k, v)
    return p


def _check(lib, rc):
    if rc != 0:
        raise LslamError(rc, lib.lslam_last_error().decode())


def _f4(a):
    """(n, >= 3) -> contiguous (n, 4) float32, w = 0 where the input has none."""
    a = np.asarray(a, np.float32)
    out = np.zeros((len(a), 4), np.float32)
    out[:, :min(4, a.shape[1])] = a[:, :4]
    return out


class SurveyMap:
    """The result of one extraction (``lslam_survey``): owns its device buffers until ``close``."""

    def __init__(self, ctx, cloud, params=None, pcd_path=None, **kw):
        self.lib = ctx.lib
        self.ctx = ctx
        self.h = None
        self.params = params if params is not None else make_params(self.lib, **kw)
        h = C.c_void_p()
        if pcd_path is not None:
            _check(self.lib, self.lib.lslam_survey_extract_file(ctx.h, str(pcd_path).encode(), C.byref(self.params), C.byref(h)))
        else:
            c = np.ascontiguousarray(cloud, np.float32)
            if c.ndim != 2 or c.shape[1] < 3:
                raise ValueError("cloud must be (n, >= 3) float32")
            _check(self.lib, self.lib.lslam_survey_extract(ctx.h, c.ctypes.data_as(C.c_void_p), len(c), c.shape[1] * 4,
                                                           C.byref(self.params), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lslam_survey_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        st = LslamSurveyStats()
        _check(self.lib, self.lib.lslam_survey_info(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in LslamSurveyStats._fields_}

    def clouds(self):
        """-> (corner (n, 4), surf (m, 4)) float32 {x, y, z, 0}, axes permuted as the reference does, block order."""
        st = self.info()
        c, s = np.zeros((st["n_corner"], 4), np.float32), np.zeros((st["n_surf"], 4), np.float32)
        _check(self.lib, self.lib.lslam_survey_get(self.h, _fp(c) if len(c) else None, len(c), _fp(s) if len(s) else None, len(s)))
        return c, s

    def save(self, directory):
        _check(self.lib, self.lib.lslam_survey_save(self.h, str(directory).encode()))


def extract(ctx, cloud, params=None, **kw):
    return SurveyMap(ctx, cloud, params, **kw)


def voxel_grid_min(ctx, cloud, leaf, min_points):
    """pcl::VoxelGrid with setMinimumPointsNumberPerVoxel(min_points) -> (m, 4) float32."""
    c = _xyzi(cloud)
    out = np.zeros((max(len(c), 1), 4), np.float32)
    n = C.c_size_t()
    _check(ctx.lib, ctx.lib.lslam_voxel_grid_min(ctx.h, c.ctypes.data_as(C.c_void_p), len(c), c.shape[1] * 4, float(leaf),
                                                 int(min_points), _fp(out), len(out), C.byref(n)))
    return out[:n.value].copy()


def debug_normals(ctx, surface, queries, radius):
    """-> (normals (q, 4) {nx, ny, nz, curvature}, NaN when undefined; neighbour counts (q,))."""
    s, q = _f4(surface), _f4(queries)
    out, cnt = np.zeros((len(q), 4), np.float32), np.zeros(len(q), np.int32)
    _check(ctx.lib, ctx.lib.lslam_debug_survey_normals(ctx.h, _fp(s), len(s), _fp(q), len(q), float(radius), _fp(out),
                                                       cnt.ctypes.data_as(c_int32_p)))
    return out, cnt


def debug_knn(ctx, pts, k, cell=0.0):
    """-> (n, k) int32 neighbour lists by (fp32 squared distance, index), -1 past the cloud's size."""
    p = _f4(pts)
    out = np.zeros((len(p), int(k)), np.int32)
    _check(ctx.lib, ctx.lib.lslam_debug_survey_knn(ctx.h, _fp(p), len(p), int(k), float(cell), out.ctypes.data_as(c_int32_p)))
    return out


def debug_region(ctx, normals_curv, lists, cos_threshold):
    """-> (labels (n,) int32: the seed point of every point's region; label-sweep launches)."""
    nc = np.ascontiguousarray(normals_curv, np.float32)
    li = np.ascontiguousarray(lists, np.int32)
    out, sweeps = np.zeros(len(nc), np.int32), C.c_int32()
    _check(ctx.lib, ctx.lib.lslam_debug_survey_region(ctx.h, _fp(nc), len(nc), li.ctypes.data_as(c_int32_p), li.shape[1],
                                                      float(cos_threshold), out.ctypes.data_as(c_int32_p), C.byref(sweeps)))
    return out, sweeps.value


def debug_boundary(ctx, pts, normals, radius, angle_threshold):
    """-> (flags (n,) bool, largest gaps (n,) float64)."""
    p, nn = _f4(pts), _f4(normals)
    flags, gaps = np.zeros(len(p), np.uint8), np.zeros(len(p), np.float64)
    _check(ctx.lib, ctx.lib.lslam_debug_survey_boundary(ctx.h, _fp(p), _fp(nn), len(p), float(radius), float(angle_threshold),
                                                        flags.ctypes.data_as(c_uint8_p), gaps.ctypes.data_as(C.POINTER(C.c_double))))
    return flags.astype(bool), gaps


def extract_file(ctx, pcd_path, params=None, **kw):
    """The extraction of a PCD file (ascii or binary; the library's reader refuses ``binary_compressed``)."""
    return SurveyMap(ctx, None, params, pcd_path=pcd_path, **kw)
