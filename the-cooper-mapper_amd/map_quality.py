"""Map quality (``csrc/lslam_mapq.hip``, ``lslam_mapq_*`` of include/lslam_c.h) and trajectory evaluation
(``csrc/lslam_traj.hip``, ``lslam_traj_*``).  Mean map entropy (MME) and mean plane variance (MPV) are the usual
ground-truth-free crispness measures of a point-cloud map: per point the covariance of its neighbourhood within a radius, from
it the entropy of the fitted Gaussian and the variance along the neighbourhood's normal; lower is crisper.  The sums are
integers, so the figures are bit-identical from run to run and for any order of the cloud.  The header states the semantics
completely; ``tests/map_quality_ref.py`` restates them in numpy.

:func:`evaluate` is the general form; ``FeatureMap.quality``, ``KeyframeStore.map_quality`` and ``Graph.map_quality`` score
clouds where they already lie in device memory.  :func:`trajectory_eval` is the reference's ``map_evaluation/Evaluation.cpp``
on arrays (host, fp64, no device needed), with a rigidly aligned ATE the reference does not have.
"""
import ctypes as C

import numpy as np

from .capi import (LslamError, LslamMapqParams, LslamMapqStats, LslamTrajParams, LslamTrajStats, c_double_p, c_int32_p,
                   load_library)

PARAM_FIELDS = ("radius", "min_neighbors", "lambda_floor")
TRAJ_PARAM_FIELDS = ("gate", "align")


def mapq_params(params=None, **kw):
    """-> :class:`LslamMapqParams`: the library's defaults, then ``params`` (a dict or an LslamMapqParams), then ``kw``."""
    p = LslamMapqParams()
    load_library().lslam_mapq_default_params(C.byref(p))
    if isinstance(params, LslamMapqParams):
        C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        params = None
    for k, v in dict(params or {}, **kw).items():
        if k not in PARAM_FIELDS:
            raise TypeError("mapq_params: unknown parameter %r" % k)
        setattr(p, k, int(v) if k == "min_neighbors" else float(v))
    return p


def _raise(lib, rc):
    if rc < 0:
        raise LslamError(rc, lib.lslam_last_error().decode())


def _is_device(x):
    return hasattr(x, "data_ptr")


def _device_points(x):
    if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[1] == 4 and x.element_size() == 4):
        raise ValueError("device points must be a contiguous (n, 4) float32 tensor on the GPU")
    return x


def _host_points(points):
    a = np.ascontiguousarray(points, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("points must be (n, >= 3), got %r" % (a.shape,))
    return a


def evaluate(ctx, surface, queries=None, params=None, per_point=False, **kw):
    """MME / MPV of ``queries`` (None: the surface itself) against ``surface`` -> the stats as a dict; with
    ``per_point=True`` -> (stats, lambda3 (nq, 3) float64, entropy (nq,) float64, count (nq,) int32), NaN where a point is
    sparse or not finite.  Host arrays ``(n, >= 3)`` float32 are uploaded (``lslam_mapq_eval``); contiguous ``(n, 4)``
    float32 torch tensors on the context's device are evaluated where they are (``lslam_mapq_eval_device``) and the
    per-point outputs are tensors there.  Keywords: :func:`mapq_params`'."""
    lib = ctx.lib
    p = mapq_params(params, **kw)
    st = LslamMapqStats()
    if _is_device(surface):
        import torch
        s = _device_points(surface)
        q = None if queries is None else _device_points(queries)
        nq = s.shape[0] if q is None else q.shape[0]
        l3 = h = cnt = None
        if per_point:
            l3 = torch.empty((nq, 3), dtype=torch.float64, device=s.device)
            h = torch.empty((nq,), dtype=torch.float64, device=s.device)
            cnt = torch.empty((nq,), dtype=torch.int32, device=s.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        if q is not None and nq == 0:  # an empty query cloud of its own is not "no queries": hand over a pointer that is not null
            q = torch.zeros((1, 4), dtype=torch.float32, device=s.device)
        _raise(lib, lib.lslam_mapq_eval_device(ctx.h, ptr(s), s.shape[0], ptr(q), nq, C.byref(p), C.byref(st), ptr(l3), ptr(h), ptr(cnt)))
        return (st.as_dict(), l3, h, cnt) if per_point else st.as_dict()
    s = _host_points(surface)
    q = None if queries is None else _host_points(queries)
    nq = len(s) if q is None else len(q)
    l3 = np.full((nq, 3), np.nan) if per_point else None
    h = np.full((nq,), np.nan) if per_point else None
    cnt = np.zeros((nq,), np.int32) if per_point else None
    _raise(lib, lib.lslam_mapq_eval(ctx.h, s.ctypes.data_as(C.c_void_p), len(s), s.shape[1] * 4,
                                    None if q is None else q.ctypes.data_as(C.c_void_p), nq, 0 if q is None else q.shape[1] * 4,
                                    C.byref(p), C.byref(st), None if l3 is None else l3.ctypes.data_as(c_double_p),
                                    None if h is None else h.ctypes.data_as(c_double_p),
                                    None if cnt is None else cnt.ctypes.data_as(c_int32_p)))
    return (st.as_dict(), l3, h, cnt) if per_point else st.as_dict()


def fmap_quality(fmap, which="surf", params=None, **kw):
    """``lslam_mapq_fmap``: the whole cube map of one feature type where it lies -> the stats as a dict."""
    p = mapq_params(params, **kw)
    st = LslamMapqStats()
    _raise(fmap.lib, fmap.lib.lslam_mapq_fmap(fmap.h, _which(which), C.byref(p), C.byref(st)))
    return st.as_dict()


def keyframes_quality(store, ids, poses, which="surf", params=None, **kw):
    """``lslam_mapq_keyframes``: the named keyframes' clouds at ``poses`` (one 4x4, graph <- sensor, each) as one cloud ->
    the stats as a dict."""
    p = mapq_params(params, **kw)
    st = LslamMapqStats()
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    T = np.ascontiguousarray(np.asarray(poses, np.float64).astype(np.float32)).reshape(len(ids), 16)
    _raise(store.lib, store.lib.lslam_mapq_keyframes(store.h, len(ids), ids.ctypes.data_as(c_int32_p),
                                                     T.ctypes.data_as(C.POINTER(C.c_float)), _which(which), C.byref(p), C.byref(st)))
    return st.as_dict()


def _which(which):
    if which in ("corner", 0):
        return 0
    if which in ("surf", 1):
        return 1
    raise ValueError("which is \"corner\" / 0 or \"surf\" / 1, got %r" % (which,))


def trajectory_eval(est_stamp, est_xyz, ref_stamp, ref_xyz, gate=None, align=False):
    """``lslam_traj_eval``: each estimate against the reference sample nearest in time (``ref_stamp`` ascending) -> dict with
    ``n_used``, ``n_gated``, ``mean`` / ``var`` / ``max`` (4,) of |dx|, |dy|, |dz| and the distance, ``mean_dt`` and, with
    ``align=True``, ``aligned``, ``ate_rmse`` and ``T_align`` (4, 4).  ``gate`` [m]: None: the reference's 10 m; 0: none."""
    lib = load_library()
    p = LslamTrajParams()
    lib.lslam_traj_default_params(C.byref(p))
    if gate is not None:
        p.gate = float(gate)
    p.align = 1 if align else 0
    es = np.ascontiguousarray(est_stamp, np.float64).reshape(-1)
    ex = np.ascontiguousarray(est_xyz, np.float64).reshape(-1, 3)
    rs = np.ascontiguousarray(ref_stamp, np.float64).reshape(-1)
    rx = np.ascontiguousarray(ref_xyz, np.float64).reshape(-1, 3)
    if len(es) != len(ex) or len(rs) != len(rx):
        raise ValueError("trajectory_eval: one stamp per position")
    st = LslamTrajStats()
    dp = lambda a: a.ctypes.data_as(c_double_p)
    _raise(lib, lib.lslam_traj_eval(dp(es), dp(ex), len(es), dp(rs), dp(rx), len(rs), C.byref(p), C.byref(st)))
    return dict(n_used=int(st.n_used), n_gated=int(st.n_gated), mean=np.array(st.mean), var=np.array(st.var), max=np.array(st.max),
                mean_dt=float(st.mean_dt), aligned=bool(st.aligned), ate_rmse=float(st.ate_rmse),
                T_align=np.array(st.T_align).reshape(4, 4))
