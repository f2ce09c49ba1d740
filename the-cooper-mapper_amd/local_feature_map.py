"""Host-side mirror of ``lidar_slam::LocalFeatureMap<PointXYZI>`` (/root/reference/L_SLAM/src/io_module/
LocalFeatureMap.h with FrameUpdater.hpp) over the C ABI: the frames of the last ``queue_distance`` metres of
path, resident in HBM (``csrc/lslam_lmap.hip``) -- ``addDataFrame`` with its ``clean()`` (n frames behind -> n + 1
erased), ``getSurroundFeature`` (the window concatenated in queue order, VoxelGrid 0.2 over the corners and 0.4 over
the surfaces).  Method names follow the reference in snake_case; clouds are ``(n, 4)`` float32 ``{x, y, z, intensity}``.

The one difference from the reference: its queue grows without bound when the sensor stands still; this one is created
with ``max_points`` per type and ``max_frames`` and refuses (``LslamError``, nothing changed) an add that would exceed one.
"""
import ctypes as C

import numpy as np

from .capi import LslamError, c_float_p, c_int32_p
from .feature_map import _fp, _xyzi

MODE_DEFAULT, MODE_REFILTER, MODE_KEY_ORDERED, MODE_ALWAYS_RESORT = 0, 1, 2, 4  # include/lslam_c.h LSLAM_LMAP_*


class LocalFeatureMap:
    def __init__(self, ctx, max_points=0, max_frames=0, mode=MODE_DEFAULT, queue_distance=None, filter_corner=None,
                 filter_surf=None):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        rc = self.lib.lslam_lmap_create(ctx.h, int(max_points), int(max_frames), int(mode), C.byref(h))
        if rc != 0:
            raise LslamError(rc, self.lib.lslam_last_error().decode())
        self.h = h
        if queue_distance is not None:
            self.setup_queue_distance(queue_distance)
        if filter_corner is not None or filter_surf is not None:
            self.setup_filter_size(0.2 if filter_corner is None else filter_corner, 0.4 if filter_surf is None else filter_surf)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lslam_lmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise LslamError(rc, self.lib.lslam_last_error().decode())
        return rc

    def setup_queue_distance(self, metres):
        self._check(self.lib.lslam_lmap_setup_queue_distance(self.h, float(metres)))

    def setup_filter_size(self, corner, surf):
        """Not in the reference (its leaves are fixed at 0.2 / 0.4); refused once a frame has been added."""
        self._check(self.lib.lslam_lmap_setup_filter_size(self.h, float(corner), float(surf)))

    def add_data_frame(self, corner, surf, tf):
        """featureMapUpdate + addDataFrame: the clouds transformed by the 4x4 ``tf``, pushed; then ``clean()``.  Two torch
        tensors on the context's device ((n, 4) float32, contiguous) are taken where they are."""
        T = np.ascontiguousarray(tf, dtype=np.float32).reshape(16)
        if hasattr(corner, "data_ptr") and hasattr(surf, "data_ptr"):
            for x in (corner, surf):
                if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[1] == 4 and x.element_size() == 4):
                    raise ValueError("device clouds must be contiguous (n, 4) float32 tensors on the GPU")
            self._check(self.lib.lslam_lmap_add_data_frame_device(self.h, C.c_void_p(corner.data_ptr()), corner.shape[0],
                                                                  C.c_void_p(surf.data_ptr()), surf.shape[0], _fp(T)))
            return
        c, s = _xyzi(corner), _xyzi(surf)
        if c.shape[1] != s.shape[1]:
            raise ValueError("corner and surf clouds must share a point layout")
        self._check(self.lib.lslam_lmap_add_data_frame(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p), len(s),
                                                       c.shape[1] * 4, _fp(T)))

    def surround_to_map_counts(self):
        """The filtered window becomes ``ctx``'s map without leaving HBM -> (n_corner, n_surf); (0, 0): the empty map."""
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_lmap_surround_to_map_counts(self.h, C.byref(nc), C.byref(ns)))
        return nc.value, ns.value

    def get_surround_feature(self):
        """-> (corner (n, 4), surf (m, 4)) on the host."""
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_lmap_get_surround(self.h, None, 0, C.byref(nc), None, 0, C.byref(ns)))
        c, s = np.zeros((nc.value, 4), np.float32), np.zeros((ns.value, 4), np.float32)
        self._check(self.lib.lslam_lmap_get_surround(self.h, _fp(c), len(c), C.byref(nc), _fp(s), len(s), C.byref(ns)))
        return c, s

    def info(self):
        nf, acc, ev = C.c_int32(), C.c_double(), C.c_int64()
        live = (C.c_size_t * 2)()
        self._check(self.lib.lslam_lmap_info(self.h, C.byref(nf), C.byref(acc), live, C.byref(ev)))
        return dict(n_frames=nf.value, accum_distance=acc.value, n_corner=live[0], n_surf=live[1], frames_evicted=ev.value)

    def get_frames(self):
        """The queue, oldest frame first -> list of (corner (n, 4), surf (m, 4), accum_distance) (debug tap)."""
        i = self.info()
        nf = C.c_int32()
        acc = np.zeros(max(i["n_frames"], 1), np.float64)
        cnt = np.zeros((max(i["n_frames"], 1), 2), np.int32)
        c, s = np.zeros((i["n_corner"], 4), np.float32), np.zeros((i["n_surf"], 4), np.float32)
        self._check(self.lib.lslam_lmap_get_frames(self.h, len(acc), C.byref(nf), acc.ctypes.data_as(C.POINTER(C.c_double)),
                                                   cnt.ctypes.data_as(c_int32_p), _fp(c), len(c), _fp(s), len(s)))
        out, ac, as_ = [], 0, 0
        for k in range(nf.value):
            out.append((c[ac:ac + cnt[k, 0]].copy(), s[as_:as_ + cnt[k, 1]].copy(), float(acc[k])))
            ac += cnt[k, 0]
            as_ += cnt[k, 1]
        return out

    def stats(self):
        """Per type and sweep so far: (new points merged into the ordered window, ordered window sorted as a whole, window re-filtered)."""
        m, r, f = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.lslam_lmap_stats(self.h, C.byref(m), C.byref(r), C.byref(f)))
        return m.value, r.value, f.value

    def clear(self):
        self._check(self.lib.lslam_lmap_clear(self.h))

    def clean(self):
        """LocalFeatureMap::clean: nothing to do -- :meth:`add_data_frame` cleans, as the reference's addDataFrame does."""
