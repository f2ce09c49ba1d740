"""Visibility votes over the keyframe store (``csrc/lslam_vis.hip``, ``lslam_vis_*`` of include/lslam_c.h): the final map
without moving objects.  A point is dynamic when other keyframes looked through the place where it is: each keyframe gets a
coarse range image, a query point is projected into each voter's image, and integer free / hit votes decide.  The header
states the semantics completely; ``tests/visibility_ref.py`` restates them in numpy.

The functions here are what :class:`KeyframeStore`'s ``vis_*`` methods call.  Voters are named by keyframe id with one 4x4
pose (graph <- sensor) each; query points are ``(n, >= 3)`` float32 on the host or a contiguous ``(n, 4)`` float32 torch
tensor on the store's device.
"""
import ctypes as C

import numpy as np

from .capi import LslamError, LslamVisParams, LslamVisStats, c_float_p, c_int32_p, load_library

PARAM_FIELDS = ("n_row", "n_col", "fov_down_deg", "fov_up_deg", "min_range", "max_range", "window", "abs_margin", "rel_margin",
                "min_free_votes", "up_axis")
POINT_TILE, KF_CHUNK = 256, 16  # LSLAM_VIS_POINT_TILE, LSLAM_VIS_KF_CHUNK


def vis_params(params=None, **kw):
    """-> :class:`LslamVisParams`: the library's defaults, then ``params`` (a dict or an LslamVisParams), then ``kw``."""
    p = LslamVisParams()
    load_library().lslam_vis_default_params(C.byref(p))
    if isinstance(params, LslamVisParams):
        C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        params = None
    for k, v in dict(params or {}, **kw).items():
        if k not in PARAM_FIELDS:
            raise TypeError("vis_params: unknown parameter %r" % k)
        setattr(p, k, v)
    return p


def split_votes(votes):
    """The packed words ``n_free | n_hit << 16`` -> (n_free, n_hit) int32 arrays."""
    v = np.asarray(votes, np.uint32)
    return (v & 0xFFFF).astype(np.int32), (v >> 16).astype(np.int32)


def dynamic_mask(votes, min_free_votes):
    """The header's rule: dynamic iff ``n_free >= min_free_votes and n_free > n_hit``."""
    nf, nh = split_votes(votes)
    return (nf >= int(min_free_votes)) & (nf > nh)


def _check(store, rc):
    if rc < 0:
        raise LslamError(rc, store.lib.lslam_last_error().decode())
    return rc


def _voters(ids, poses):
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    T = np.ascontiguousarray(np.asarray(poses, np.float64).astype(np.float32)).reshape(len(ids), 16)
    return ids, T


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
    if a.shape[1] < 4:
        a = np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 4 - a.shape[1]), np.float32)], axis=1))
    return a


def setup(store, params=None, **kw):
    """``lslam_vis_setup``: install the parameters (what is not named keeps its default).  Other parameters than those in
    force drop the range images held."""
    p = vis_params(params, **kw)
    _check(store, store.lib.lslam_vis_setup(store.h, C.byref(p)))


def info(store):
    st = LslamVisStats()
    _check(store, store.lib.lslam_vis_info(store.h, C.byref(st)))
    out = {k: getattr(st.params, k) for k in PARAM_FIELDS}
    out.update(is_set=bool(st.is_set), n_images=st.n_images, image_bytes=st.image_bytes, image_launches=st.image_launches,
               vote_launches=st.vote_launches)
    return out


def range_image(store, kid):
    """Keyframe ``kid``'s range image (parity tap) -> (n_row, n_col) float32, +inf where nothing was seen."""
    i = info(store)
    out = np.zeros((max(i["n_row"], 1), max(i["n_col"], 1)), np.float32)
    _check(store, store.lib.lslam_vis_range_image(store.h, int(kid), out.ctypes.data_as(c_float_p)))
    return out


def votes(store, ids, poses, points):
    """The packed votes of the named voters on ``points`` -> uint32 (n,) (a torch int32 tensor for device points: the same
    bits)."""
    ids, T = _voters(ids, poses)
    if _is_device(points):
        import torch
        pts = _device_points(points)
        out = torch.zeros(pts.shape[0], dtype=torch.int32, device=pts.device)
        _check(store, store.lib.lslam_vis_votes_device(store.h, len(ids), ids.ctypes.data_as(c_int32_p), T.ctypes.data_as(c_float_p),
                                                       C.c_void_p(pts.data_ptr()), pts.shape[0], C.c_void_p(out.data_ptr())))
        return out
    a = _host_points(points)
    out = np.zeros(len(a), np.uint32)
    _check(store, store.lib.lslam_vis_votes(store.h, len(ids), ids.ctypes.data_as(c_int32_p), T.ctypes.data_as(c_float_p),
                                            a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4,
                                            out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def filter_points(store, ids, poses, points):
    """The points that are not dynamic, in input order (``lslam_vis_filter_device``; host points are uploaded first) ->
    (m, 4) float32, on the side the input was on."""
    import torch
    ids, T = _voters(ids, poses)
    host = not _is_device(points)
    if host:
        pts = torch.from_numpy(_host_points(points)[:, :4].copy()).to("cuda:%d" % store.ctx.device)
    else:
        pts = _device_points(points)
    out = torch.empty_like(pts)
    kept = C.c_size_t()
    _check(store, store.lib.lslam_vis_filter_device(store.h, len(ids), ids.ctypes.data_as(c_int32_p), T.ctypes.data_as(c_float_p),
                                                    C.c_void_p(pts.data_ptr()), pts.shape[0], C.c_void_p(out.data_ptr()),
                                                    C.byref(kept)))
    out = out[:kept.value]
    return out.cpu().numpy() if host else out


def add_to_fmap(store, kid, fmap, tf, ids, poses):
    """``KeyframeStore.add_to_fmap`` with the filter in front -> (corner, surf) points left out."""
    ids, T = _voters(ids, poses)
    tf = np.ascontiguousarray(tf, dtype=np.float32).reshape(16)
    removed = (C.c_size_t * 2)()
    _check(store, store.lib.lslam_vis_add_to_fmap(store.h, int(kid), fmap.h, tf.ctypes.data_as(c_float_p), len(ids),
                                                  ids.ctypes.data_as(c_int32_p), T.ctypes.data_as(c_float_p), removed))
    return int(removed[0]), int(removed[1])
