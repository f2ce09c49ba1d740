"""Floor detection on the device (``csrc/lslam_floor.hip``, ``lslam_floor_*`` of include/lslam_c.h): the ground plane of a
cloud by a deterministic RANSAC -- height-band candidates, hashed three-point hypotheses, fp32 inlier counts, lowest index on
ties, an fp64 refit.  The header states the semantics completely; ``tests/floor_ref.py`` restates them in numpy.

Clouds are ``(n, 4)`` float32 ``{x, y, z, intensity}`` on the host, or a device pointer with a count.  Results are dicts:
``plane`` (4,) float64 with a unit normal, ``n_candidates``, ``n_inliers``, ``best_hypothesis``, ``best_count``,
``rms_distance``, ``status`` (``FLOOR_*``).
"""
import ctypes as C

import numpy as np

from .capi import (FLOOR_FEW_CANDIDATES, FLOOR_FEW_INLIERS, FLOOR_NO_HYPOTHESIS, FLOOR_OK, FLOOR_STEEP, LslamError,
                   LslamFloorParams, LslamFloorResult, c_float_p, c_int32_p, load_library)

PARAM_FIELDS = ("up", "sensor_height", "height_clip_range", "max_range", "n_hypotheses", "inlier_threshold", "min_inliers",
                "max_normal_angle_deg", "refit_iterations", "seed")
STATUS_NAMES = {FLOOR_OK: "OK", FLOOR_FEW_CANDIDATES: "FEW_CANDIDATES", FLOOR_NO_HYPOTHESIS: "NO_HYPOTHESIS",
                FLOOR_FEW_INLIERS: "FEW_INLIERS", FLOOR_STEEP: "STEEP"}


def floor_params(params=None, **kw):
    """-> :class:`LslamFloorParams`: the library's defaults, then ``params`` (a dict or an LslamFloorParams), then ``kw``."""
    p = LslamFloorParams()
    load_library().lslam_floor_default_params(C.byref(p))
    if isinstance(params, LslamFloorParams):
        C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        params = None
    for k, v in dict(params or {}, **kw).items():
        if k not in PARAM_FIELDS:
            raise TypeError("floor_params: unknown parameter %r" % k)
        if k == "up":
            p.up[0], p.up[1], p.up[2] = (float(x) for x in v)
        else:
            setattr(p, k, v)
    return p


def _check(lib, rc):
    if rc < 0:
        raise LslamError(rc, lib.lslam_last_error().decode())


def detect(ctx, cloud, params=None):
    """``lslam_floor_detect``: the floor of a host cloud ((n, 3 or more) float32-convertible; x, y, z are read)."""
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("cloud must be (n, >= 3), got %r" % (a.shape,))
    if a.shape[1] < 4:
        a = np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 4 - a.shape[1]), np.float32)], axis=1))
    p, r = floor_params(params), LslamFloorResult()
    _check(ctx.lib, ctx.lib.lslam_floor_detect(ctx.h, a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4, C.byref(p), C.byref(r)))
    return r.as_dict()


def detect_device(ctx, d_xyzi, n, params=None):
    """``lslam_floor_detect_device``: a packed {x, y, z, -} cloud in the context's device memory (a pointer, or a contiguous
    (n, 4) float32 torch tensor on the GPU)."""
    if hasattr(d_xyzi, "data_ptr"):
        d_xyzi = d_xyzi.data_ptr()
    p, r = floor_params(params), LslamFloorResult()
    _check(ctx.lib, ctx.lib.lslam_floor_detect_device(ctx.h, C.c_void_p(int(d_xyzi or 0)), int(n), C.byref(p), C.byref(r)))
    return r.as_dict()


def debug_hypotheses(ctx):
    """``lslam_debug_floor_hypotheses`` of the context's last single-cloud detection -> dict: ``cand_idx`` int32[K],
    ``triples`` int32[H, 3], ``planes`` float32[H, 4], ``counts`` int32[H] (-1 degenerate, -2 steep)."""
    lib = ctx.lib
    nk, nh = C.c_size_t(), C.c_size_t()
    _check(lib, lib.lslam_debug_floor_hypotheses(ctx.h, None, 0, C.byref(nk), None, None, None, 0, C.byref(nh)))
    K, H = nk.value, nh.value
    idx, tri = np.zeros(max(K, 1), np.int32), np.zeros((H, 3), np.int32)
    pl, cnt = np.zeros((H, 4), np.float32), np.zeros(H, np.int32)
    _check(lib, lib.lslam_debug_floor_hypotheses(ctx.h, idx.ctypes.data_as(c_int32_p), K, C.byref(nk), tri.ctypes.data_as(c_int32_p),
                                                 pl.ctypes.data_as(c_float_p), cnt.ctypes.data_as(c_int32_p), H, C.byref(nh)))
    return dict(cand_idx=idx[:K], triples=tri, planes=pl, counts=cnt)
