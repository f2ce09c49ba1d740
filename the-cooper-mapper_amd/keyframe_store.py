"""The pose graph's keyframe clouds resident in HBM (``csrc/lslam_kfs.hip``, ``lslam_kfs_*`` of include/lslam_c.h): a
keyframe's corner and surface cloud are uploaded once, and the steps of ``pose_graph::Graph`` / ``LoopDetector`` that use
them -- the loop detector's coarse and fine alignment, ``getFinalFeatureMap``'s filter, match and ``addFeatureCloud`` -- name
them by id and move no point between host and device.  Clouds are ``(n, 4)`` float32 ``{x, y, z, intensity}``; ids are
0, 1, 2, ... in order of insertion.

Like :class:`LocalFeatureMap`, the store has limits where the reference's vector grows without bound: an add past
``max_points`` per type or ``max_keyframes`` raises :class:`LslamError` and changes nothing.
"""
import ctypes as C

import numpy as np

from .capi import LslamError, LslamKfsStats, LslamScParams, LslamScStats, LslamStats, c_int32_p
from .feature_map import _fp, _xyzi

# lslam_kfs_loop_match's *stage (include/lslam_c.h LSLAM_KFS_*)
EMPTY_REFERENCE, ICP_REJECTED, MATCH_FAILED, LOOP_ACCEPTED = 0, 1, 2, 3
MAX_CANDIDATES = 6  # loop_detector.hpp:141
SC_PARAM_FIELDS = ("n_ring", "n_sector", "max_range", "height_offset", "up_axis")


def sc_shift_guess(shift, n_sector, up_axis):
    """The pose of the query in the candidate's frame that a scan-context shift stands for (include/lslam_c.h, SHIFT): the
    rotation by ``shift * 2 pi / n_sector`` about the up axis, zero translation -> 4x4 float32, ``loop_match``'s ``guess``."""
    psi = float(shift) * (2.0 * np.pi / float(n_sector))
    c, s = np.cos(psi), np.sin(psi)
    T = np.eye(4)
    if int(up_axis) == 1:  # about +y: z -> x
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
    else:  # about +z: x -> y
        T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    return T.astype(np.float32)


class KeyframeStore:
    def __init__(self, ctx, max_points=0, max_keyframes=0, slab_points=0):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        rc = self.lib.lslam_kfs_create(ctx.h, int(max_points), int(max_keyframes), int(slab_points), C.byref(h))
        if rc != 0:
            raise LslamError(rc, self.lib.lslam_last_error().decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lslam_kfs_destroy(self.h)
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

    def __len__(self):
        return self.info()["n_keyframes"]

    def add(self, corner, surf):
        """-> the new keyframe's id.  Two torch tensors on the context's device ((n, 4) float32, contiguous) are copied
        device to device (``lslam_kfs_add_device``); anything else is uploaded, both clouds behind one wait."""
        kid = C.c_int32(-1)
        if hasattr(corner, "data_ptr") and hasattr(surf, "data_ptr"):
            for x in (corner, surf):
                if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[1] == 4 and x.element_size() == 4):
                    raise ValueError("device clouds must be contiguous (n, 4) float32 tensors on the GPU")
            self._check(self.lib.lslam_kfs_add_device(self.h, C.c_void_p(corner.data_ptr()), corner.shape[0],
                                                      C.c_void_p(surf.data_ptr()), surf.shape[0], C.byref(kid)))
            return kid.value
        c, s = _xyzi(corner), _xyzi(surf)
        if c.shape[1] != s.shape[1]:
            raise ValueError("corner and surf clouds must share a point layout")
        self._check(self.lib.lslam_kfs_add(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p), len(s),
                                           c.shape[1] * 4, C.byref(kid)))
        return kid.value

    def counts(self, kid):
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_kfs_counts(self.h, int(kid), C.byref(nc), C.byref(ns)))
        return nc.value, ns.value

    def get(self, kid, which):
        """One cloud back on the host; ``which``: 0 corner, 1 surf -> (n, 4) float32."""
        n = self.counts(kid)[int(which)]
        out = np.zeros((n, 4), np.float32)
        got = C.c_size_t()
        self._check(self.lib.lslam_kfs_get(self.h, int(kid), int(which), _fp(out), n, C.byref(got)))
        return out

    def view(self, kid):
        """-> (corner device pointer, n_corner, surf device pointer, n_surf); the pointers stay valid until clear / close."""
        pc, ps = C.c_void_p(), C.c_void_p()
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_kfs_view(self.h, int(kid), C.byref(pc), C.byref(nc), C.byref(ps), C.byref(ns)))
        return pc.value or 0, nc.value, ps.value or 0, ns.value

    def info(self):
        st = LslamKfsStats()
        self._check(self.lib.lslam_kfs_info(self.h, C.byref(st)))
        return dict(n_keyframes=st.n_keyframes, n_corner=st.n_points[0], n_surf=st.n_points[1], n_slabs=st.n_slabs,
                    bytes_held=st.bytes_held, cloud_bytes_uploaded=st.cloud_bytes_uploaded,
                    cloud_bytes_downloaded=st.cloud_bytes_downloaded)

    def clear(self):
        self._check(self.lib.lslam_kfs_clear(self.h))

    @staticmethod
    def _candidates(ids, rel_T):
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        T = np.ascontiguousarray(rel_T, np.float32).reshape(len(ids), 16)
        return ids, T

    def debug_local_clouds(self, ids, rel_T):
        """The loop detector's reference clouds (debug tap): candidate ``ids[0]``'s clouds as they are, the others transformed
        by ``rel_T[k]`` (4x4 float32; ``rel_T[0]`` is not read) and appended -> (corner (n, 4), surf (m, 4))."""
        ids, T = self._candidates(ids, rel_T)
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_kfs_debug_local_clouds(self.h, len(ids), ids.ctypes.data_as(c_int32_p), _fp(T), None, 0,
                                                          C.byref(nc), None, 0, C.byref(ns)))
        c, s = np.zeros((nc.value, 4), np.float32), np.zeros((ns.value, 4), np.float32)
        self._check(self.lib.lslam_kfs_debug_local_clouds(self.h, len(ids), ids.ctypes.data_as(c_int32_p), _fp(T), _fp(c), len(c),
                                                          C.byref(nc), _fp(s), len(s), C.byref(ns)))
        return c, s

    def loop_match(self, ids, rel_T, new_id, guess, opts=None, icp_max_iterations=10):
        """``LoopDetector::matching_nearest`` behind its gating, on the device (``lslam_kfs_loop_match``) -> dict: ``stage``
        (EMPTY_REFERENCE / ICP_REJECTED / MATCH_FAILED / LOOP_ACCEPTED), ``guess`` (4x4 float32), ``fitness``,
        ``icp_iterations``, ``stats`` (the scan match's lslam_stats)."""
        ids, T = self._candidates(ids, rel_T)
        g = np.array(guess, dtype=np.float32).reshape(16)
        stage, its, fit, st = C.c_int32(), C.c_int32(), C.c_double(), LslamStats()
        self._check(self.lib.lslam_kfs_loop_match(self.h, len(ids), ids.ctypes.data_as(c_int32_p), _fp(T), int(new_id), _fp(g),
                                                  int(icp_max_iterations), C.byref(opts) if opts is not None else None,
                                                  C.byref(stage), C.byref(fit), C.byref(its), C.byref(st)))
        return dict(stage=stage.value, guess=g.reshape(4, 4), fitness=fit.value, icp_iterations=its.value, stats=st)

    def scanmatch(self, kid, leaf_corner, leaf_surf, pose, opts=None):
        """The keyframe's clouds filtered on the device, matched against the context's resident map
        (``lslam_kfs_scanmatch``) -> (status, pose (6,), stats), as ``Context.scanmatch_scan``."""
        from .capi import Status
        p = np.array(pose, dtype=np.float32).reshape(6)
        st = LslamStats()
        rc = self._check(self.lib.lslam_kfs_scanmatch(self.h, int(kid), float(leaf_corner), float(leaf_surf), _fp(p),
                                                      C.byref(opts) if opts is not None else None, C.byref(st)))
        return Status(rc), p, st

    def edge_information(self, ref_ids, rel_T, new_id, T, leaves=(0.2, 0.4, 0.2, 0.4)):
        """``lslam_keyframe_edge_information``: the match Hessian of keyframe ``new_id`` at pose ``T`` (4x4, in ``ref_ids[0]``'s
        frame) against the local clouds of ``ref_ids`` under ``rel_T`` -> :class:`LslamEdgeInfo`.  ``leaves``: reference
        corner / surf, new corner / surf (scanMatchLocal's by default)."""
        from .capi import LslamEdgeInfo
        ids, R = self._candidates(ref_ids, rel_T)
        Tf = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        out = LslamEdgeInfo()
        self._check(self.lib.lslam_keyframe_edge_information(self.h, len(ids), ids.ctypes.data_as(c_int32_p), _fp(R), int(new_id), _fp(Tf),
                                                        float(leaves[0]), float(leaves[1]), float(leaves[2]), float(leaves[3]),
                                                        C.byref(out)))
        return out

    def add_to_fmap(self, kid, fmap, tf):
        """``FeatureMap.add_feature_cloud`` with the keyframe's clouds taken from the store."""
        T = np.ascontiguousarray(tf, dtype=np.float32).reshape(16)
        self._check(self.lib.lslam_kfs_add_to_fmap(self.h, int(kid), fmap.h, _fp(T)))

    def floor_detect(self, ids, params=None):
        """``lslam_floor_detect_keyframes``: the floor of each named keyframe's surface cloud, where it lies -- every keyframe
        through each stage in one launch, no cloud moved -> one result dict per id (:mod:`.floor`)."""
        from .capi import LslamFloorResult
        from .floor import floor_params
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        p = floor_params(params)
        res = (LslamFloorResult * max(len(ids), 1))()
        self._check(self.lib.lslam_floor_detect_keyframes(self.h, len(ids), ids.ctypes.data_as(c_int32_p), C.byref(p), res))
        return [res[i].as_dict() for i in range(len(ids))]

    # ---- 2D occupancy grid: ray-cast votes of the keyframes (lslam_occ_*, :mod:`.occupancy`) ----------------------------------
    def occ_setup(self, params=None, **kw):
        """Install the grid's parameters (``resolution``, ``origin``, ``width``, ``height``, ``up_axis``, ``min_range``,
        ``max_range``, ``obstacle_min``, ``obstacle_max``, ``ground_band``, ``sensor_height``, ``ground_clears``,
        ``hit_weight``, ``min_observations``; ``width`` and ``height`` have no default).  Other parameters than those in force
        clear the grid."""
        from . import occupancy
        occupancy.setup(self, params, **kw)

    def occ_fit_bounds(self, poses, params=None, **kw):
        """-> the parameters with ``origin``, ``width`` and ``height`` fitted to ``poses`` +- ``max_range`` (host only)."""
        from . import occupancy
        return occupancy.fit_bounds(poses, params, **kw)

    def occ_integrate(self, ids, poses, planes=None, plane_valid=None):
        """Add the votes of keyframes ``ids`` at ``poses`` (4x4 each, graph <- sensor); ``planes``: their floor planes
        ((n, 4), sensor frame) or None for the fallback, ``plane_valid``: 0 -> the fallback for that keyframe."""
        from . import occupancy
        occupancy.integrate(self, ids, poses, planes, plane_valid)

    def occ_counts(self):
        from . import occupancy
        return occupancy.counts(self)

    def occ_values(self):
        from . import occupancy
        return occupancy.values(self)

    def occ_view(self):
        from . import occupancy
        return occupancy.view(self)

    def occ_clear(self):
        from . import occupancy
        occupancy.clear(self)

    def occ_info(self):
        from . import occupancy
        return occupancy.info(self)

    # ---- visibility votes: the final map without moving objects (lslam_vis_*, :mod:`.visibility`) -----------------------------
    def vis_setup(self, params=None, **kw):
        """Install the visibility parameters (``n_row``, ``n_col``, ``fov_down_deg``, ``fov_up_deg``, ``min_range``,
        ``max_range``, ``window``, ``abs_margin``, ``rel_margin``, ``min_free_votes``, ``up_axis``; what is not named keeps its
        default).  Other parameters than those in force drop the range images held."""
        from . import visibility
        visibility.setup(self, params, **kw)

    def vis_info(self):
        from . import visibility
        return visibility.info(self)

    def vis_range_image(self, kid):
        """Keyframe ``kid``'s range image (parity tap) -> (n_row, n_col) float32, +inf where nothing was seen."""
        from . import visibility
        return visibility.range_image(self, kid)

    def vis_votes(self, ids, poses, points):
        """The votes of keyframes ``ids`` at ``poses`` (4x4 each, graph <- sensor) on ``points`` (host array, or a contiguous
        (n, 4) float32 torch tensor on the device) -> the packed words ``n_free | n_hit << 16``."""
        from . import visibility
        return visibility.votes(self, ids, poses, points)

    def vis_filter(self, ids, poses, points):
        """``points`` without the dynamic ones, in input order, compacted on the device -> (m, 4) float32."""
        from . import visibility
        return visibility.filter_points(self, ids, poses, points)

    def vis_add_to_fmap(self, kid, fmap, tf, ids, poses):
        """:meth:`add_to_fmap` with the filter in front: the keyframe's points at ``tf`` are voted on by keyframes ``ids`` at
        ``poses``; what is not dynamic is added -> (corner, surf) points left out.  No cloud crosses PCIe."""
        from . import visibility
        return visibility.add_to_fmap(self, kid, fmap, tf, ids, poses)

    def map_quality(self, ids, poses, which="surf", **params):
        """Mean map entropy and mean plane variance of keyframes ``ids``' clouds of one type put together at ``poses`` (4x4
        each, graph <- sensor): the score of a trajectory (``lslam_mapq_keyframes``; :mod:`.map_quality`) -> the stats as a
        dict.  No cloud crosses PCIe.  Keywords: ``radius``, ``min_neighbors``, ``lambda_floor``."""
        from . import map_quality
        return map_quality.keyframes_quality(self, ids, poses, which, **params)

    # ---- loop candidates by appearance: scan context (lslam_sc_*) ---------------------------------------------------------
    def sc_setup(self, **params):
        """Install the scan-context parameters (``n_ring``, ``n_sector``, ``max_range``, ``height_offset``, ``up_axis``;
        what is not named keeps its default).  Other parameters than those in force drop the descriptors held."""
        p = LslamScParams()
        self.lib.lslam_sc_default_params(C.byref(p))
        for k, v in params.items():
            if k not in SC_PARAM_FIELDS:
                raise TypeError("sc_setup: unknown parameter %r" % k)
            setattr(p, k, v)
        self._check(self.lib.lslam_sc_setup(self.h, C.byref(p)))

    def sc_info(self):
        st = LslamScStats()
        self._check(self.lib.lslam_sc_info(self.h, C.byref(st)))
        out = {k: getattr(st.params, k) for k in SC_PARAM_FIELDS}
        out.update(is_set=bool(st.is_set), n_described=st.n_described, descriptor_bytes=st.descriptor_bytes,
                   describe_launches=st.describe_launches, query_launches=st.query_launches)
        return out

    def sc_descriptor(self, kid):
        """Keyframe ``kid``'s descriptor (parity tap) -> (n_ring, n_sector) float32."""
        i = self.sc_info()
        out = np.zeros((max(i["n_ring"], 1), max(i["n_sector"], 1)), np.float32)
        self._check(self.lib.lslam_sc_descriptor(self.h, int(kid), _fp(out)))
        return out

    def sc_query(self, query_ids, max_cand_id=None, top_k=4):
        """Each query keyframe against the keyframes ``0 .. max_cand_id[q]`` (None: ``query_ids[q] - 1``) -> one
        ``(ids, shifts, dists)`` triple of arrays per query, best first (distance, then id), at most ``top_k`` long."""
        q = np.ascontiguousarray(query_ids, np.int32).reshape(-1)
        lim = None if max_cand_id is None else np.ascontiguousarray(max_cand_id, np.int32).reshape(-1)
        if lim is not None and len(lim) != len(q):
            raise ValueError("sc_query: one max_cand_id per query")
        k = max(int(top_k), 1)
        ids, sh = np.full((len(q), k), -1, np.int32), np.zeros((len(q), k), np.int32)
        d, n = np.ones((len(q), k), np.float32), np.zeros(len(q), np.int32)
        self._check(self.lib.lslam_sc_query(self.h, len(q), q.ctypes.data_as(c_int32_p),
                                                lim.ctypes.data_as(c_int32_p) if lim is not None else None, int(top_k),
                                                ids.ctypes.data_as(c_int32_p), sh.ctypes.data_as(c_int32_p), _fp(d),
                                                n.ctypes.data_as(c_int32_p)))
        return [(ids[i, :n[i]].copy(), sh[i, :n[i]].copy(), d[i, :n[i]].copy()) for i in range(len(q))]

    def sc_distances(self, query_id):
        """The query kernel's distance and shift of ``query_id`` against every keyframe (parity tap) -> (dist, shift)."""
        n = len(self)
        d, sh = np.zeros(n, np.float32), np.zeros(n, np.int32)
        self._check(self.lib.lslam_sc_distances(self.h, int(query_id), _fp(d), sh.ctypes.data_as(c_int32_p)))
        return d, sh
