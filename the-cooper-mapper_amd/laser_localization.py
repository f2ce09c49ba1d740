"""Host-side mirror of ``lidar_slam::LaserLocalization`` (/root/reference/L_SLAM/src/odometry/LaserLocalization.cpp over
util/FeatureMap.h) on the device-resident node ``lslam_loc`` (``csrc/lslam_loc.hip``, include/lslam_c.h): a prebuilt map is
loaded once (``load_map`` / ``set_map`` / ``set_map_from``), every cube's kd-tree is built once, and each sweep runs
transformMerge, the two scan filters, FeatureMap::scanMatchScan and transformUpdate behind one host wait.

Poses are row-major 4x4 float32; clouds are ``(n, 4)`` float32 ``{x, y, z, intensity}`` (or ``(n, 8)`` pcl::PointXYZI).
``dynamic_mode=True`` is LaserMatcher's ``dynamicMode`` branch: the cubes are a window over ``files_directory``
(``index2.txt`` plus ``<count>.pcd``) that follows the sensor (``lslam_pmap_open``; :mod:`.dynamic_feature_map`).
ROS plumbing, ``inputFrameSkip`` and the UKF are not mirrored.
"""
import ctypes as C

import numpy as np

from collections import namedtuple

from .capi import (LslamError, LslamLocMapStats, LslamLocSearchCounts, LslamLocWindowStats, LslamRelocMapStats, LslamRelocOpts,
                   LslamRelocResult, LslamStats, c_int32_p, c_uint8_p)
from .feature_map import _fp, _xyzi

DROPPED, HAS_VELOCITY, POSE_RESET, VELOCITY_ZEROED, SECOND_WAIT = 1, 2, 4, 8, 16  # LSLAM_LOC_* flags
HOW_SKIPPED, HOW_GRID, HOW_TREE = 0, 1, 2
RELOC_POS_TILE, RELOC_CHUNK = 32, 1024  # LSLAM_RELOC_POS_TILE / LSLAM_RELOC_CHUNK: the scoring kernel's shape

RelocCandidate = namedtuple("RelocCandidate", "hypothesis coarse_score status rounds n_rows pose")
RelocResult = namedtuple("RelocResult", "status accepted winner runner_up fraction T n_hypotheses skipped n_points n_scored "
                                        "occupied_voxels n_selected candidates ms_coarse ms_refine")


class YawSweep(np.ndarray):
    """(n, 3) float32 Twist angle triplets of a full turn; ``rot_cyclic`` tells relocalize that the indices wrap around."""
    rot_cyclic = True


def yaw_sweep(step_deg, axis, tilt=(0.0, 0.0)):
    """Angle triplets (rx, ry, rz) of a full turn about ``axis`` every ``step_deg`` degrees: axis 1 for the reference's y-up
    sensor frame, 2 for z-up (as ``synth``).  ``tilt`` fills the other two angles, in ascending axis order.  Needs no device."""
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    n = int(round(360.0 / float(step_deg)))
    if n < 1 or abs(n * float(step_deg) - 360.0) > 1e-6:
        raise ValueError("step_deg must divide 360")
    out = np.zeros((n, 3), np.float32)
    others = [a for a in range(3) if a != axis]
    out[:, others[0]], out[:, others[1]] = np.float32(tilt[0]), np.float32(tilt[1])
    out[:, axis] = (np.arange(n, dtype=np.float64) * (2.0 * np.pi / n)).astype(np.float32)
    return out.view(YawSweep)


def grid_positions(center, half_extent, step, height):
    """(n, 3) float32 positions on a square grid: center[0] + i * step, center[1] + j * step for |i|, |j| <= half_extent / step,
    first coordinate slowest, every one at ``height`` (the third coordinate).  Needs no device."""
    k = int(np.floor(float(half_extent) / float(step) + 1e-9))
    off = np.arange(-k, k + 1, dtype=np.float64) * float(step)
    xs, ys = np.meshgrid(float(center[0]) + off, float(center[1]) + off, indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, float(height))], 1).astype(np.float32)


class LaserLocalization:
    def __init__(self, ctx, cube_width=21, cube_height=11, cube_depth=21, filter_corner=None, filter_surf=None,
                 map_filter_corner=None, map_filter_surf=None, cube_size=None, world_origin=None, lidar_valid_distance=None,
                 dynamic_mode=False, files_directory=None, paged_capacity=None):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        rc = self.lib.lslam_loc_create(ctx.h, int(cube_width), int(cube_height), int(cube_depth), C.byref(h))
        if rc != 0:
            raise LslamError(rc, self.lib.lslam_last_error().decode())
        self.h = h
        if filter_corner is not None or filter_surf is not None:
            self._check(self.lib.lslam_loc_setup_scan_filter_size(self.h, float(filter_corner or 1.0), float(filter_surf or 1.0)))
        if map_filter_corner is not None or map_filter_surf is not None:
            self._check(self.lib.lslam_loc_setup_map_filter_size(self.h, float(map_filter_corner or 1.0),
                                                                 float(map_filter_surf or 1.0)))
        if cube_size is not None:
            self._check(self.lib.lslam_loc_setup_world_cube_size(self.h, float(cube_size)))
        if world_origin is not None:
            self._check(self.lib.lslam_loc_setup_world_origin(self.h, *[int(v) for v in world_origin]))
        if lidar_valid_distance is not None:
            self._check(self.lib.lslam_loc_setup_lidar_valid_distance(self.h, float(lidar_valid_distance)))
        self.dynamic_mode = bool(dynamic_mode)
        if paged_capacity is not None:
            self._check(self.lib.lslam_pmap_setup_capacity(self.h, int(paged_capacity)))
        if self.dynamic_mode and files_directory is not None:  # LaserMatcher.cpp:100-104
            self.setup_files_directory(files_directory)
        self.lidar_mapped = np.eye(4, dtype=np.float32)  # _lidarMappedNew after the last processed sweep
        self.velocity = None                             # None until a sweep has one
        self.last_stats = None
        self.last_flags = 0
        self.last_status = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.lslam_loc_destroy(self.h)
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

    # ---- the map, built once ------------------------------------------------------------------------------------------
    def load_map(self, directory):
        """loadCloudFromFiles: every listed cube through its type's VoxelGrid (the map filters), then every tree."""
        self._check(self.lib.lslam_loc_load(self.h, str(directory).encode()))

    def set_map(self, corner, surf, filter=False):
        c, s = _xyzi(corner), _xyzi(surf)
        if c.shape[1] != s.shape[1]:
            raise ValueError("corner and surf clouds must share a point layout")
        self._check(self.lib.lslam_loc_set_map(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p), len(s),
                                               c.shape[1] * 4, 1 if filter else 0))

    def set_map_from(self, feature_map):
        """Adopt the map of a :class:`~.feature_map.FeatureMap` on the same context, device to device."""
        self._check(self.lib.lslam_loc_set_map_from_fmap(self.h, feature_map.h))

    # ---- the dynamic mode: a window of cubes paged in from files ------------------------------------------------------
    def setup_files_directory(self, directory):
        """setupFilesDirectory: index2.txt is read; no PCD is touched before the first sweep."""
        self._check(self.lib.lslam_pmap_open(self.h, str(directory).encode()))
        self.dynamic_mode = True

    def setup_paged_capacity(self, max_points_per_type):
        self._check(self.lib.lslam_pmap_setup_capacity(self.h, int(max_points_per_type)))

    def update(self, position):
        """DynamicFeatureMap::update at a sensor position (the window follows it, then the active area)."""
        p = np.ascontiguousarray(position, dtype=np.float32).reshape(3)
        self._check(self.lib.lslam_pmap_update(self.h, _fp(p)))

    def stage(self, position):
        """Read, filter and build the cubes a window around ``position`` would need, ahead of the step that takes them."""
        p = np.ascontiguousarray(position, dtype=np.float32).reshape(3)
        self._check(self.lib.lslam_pmap_stage(self.h, _fp(p)))

    def get_window_surround(self):
        """getSurroundFeature of the window as the last update left it -> (corner (n, 4), surf (m, 4))."""
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_pmap_get_surround(self.h, None, 0, C.byref(nc), None, 0, C.byref(ns)))
        c, s = np.zeros((nc.value, 4), np.float32), np.zeros((ns.value, 4), np.float32)
        self._check(self.lib.lslam_pmap_get_surround(self.h, _fp(c), len(c), C.byref(nc), _fp(s), len(s), C.byref(ns)))
        return c, s

    def window_info(self):
        o = LslamLocWindowStats()
        self._check(self.lib.lslam_pmap_window_info(self.h, C.byref(o)))
        out = {}
        for f, ty in LslamLocWindowStats._fields_:
            v = getattr(o, f)
            out[f] = tuple(int(x) for x in v) if hasattr(v, "__len__") else int(v)
        return out

    def set_search(self, use_grid):
        self._check(self.lib.lslam_loc_setup_search(self.h, 1 if use_grid else 0))

    def info(self):
        o = LslamLocMapStats()
        self._check(self.lib.lslam_loc_info(self.h, C.byref(o)))
        return dict(cubes_loaded=tuple(o.cubes_loaded), cubes_with_tree=tuple(o.cubes_with_tree), n_points=tuple(o.n_points),
                    structure_builds=o.structure_builds, grid_builds=o.grid_builds, grid_cube=tuple(o.grid_cube),
                    grid_reach=o.grid_reach, grid_on=tuple(o.grid_on), tree_depth=o.tree_depth)

    # ---- the sweep ----------------------------------------------------------------------------------------------------
    def handle_initial_pose(self, T):
        T = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        self._check(self.lib.lslam_loc_set_initial_pose(self.h, _fp(T)))

    def process(self, corner_last, surf_last, lidar_odom_new, stamp_ns):
        """One sweep -> the 4x4 ``_lidarMappedNew``, or None when the sweep was dropped (no initial pose yet).  Two torch
        tensors on the context's device ((n, 4) float32, contiguous) are taken where they are."""
        odom = np.ascontiguousarray(lidar_odom_new, dtype=np.float32).reshape(16)
        T = np.zeros(16, np.float32)
        v = np.zeros(3, np.float32)
        flags = C.c_int32()
        st = LslamStats()
        if hasattr(corner_last, "data_ptr") and hasattr(surf_last, "data_ptr"):
            for x in (corner_last, surf_last):
                if not (x.is_cuda and x.is_contiguous() and x.dim() == 2 and x.shape[1] == 4 and x.element_size() == 4):
                    raise ValueError("device clouds must be contiguous (n, 4) float32 tensors on the GPU")
            rc = self.lib.lslam_loc_process_device(self.h, C.c_void_p(corner_last.data_ptr()), corner_last.shape[0],
                                                   C.c_void_p(surf_last.data_ptr()), surf_last.shape[0], _fp(odom), int(stamp_ns),
                                                   _fp(T), _fp(v), C.byref(flags), C.byref(st))
        else:
            c, s = _xyzi(corner_last), _xyzi(surf_last)
            if c.shape[1] != s.shape[1]:
                raise ValueError("corner and surf clouds must share a point layout")
            rc = self.lib.lslam_loc_process(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p), len(s),
                                            c.shape[1] * 4, _fp(odom), int(stamp_ns), _fp(T), _fp(v), C.byref(flags), C.byref(st))
        self._check(rc)
        self.last_status, self.last_flags = rc, flags.value
        if flags.value & DROPPED:
            return None
        self.last_stats = st
        self.lidar_mapped = T.reshape(4, 4).copy()
        self.velocity = v.copy() if flags.value & HAS_VELOCITY else None
        return self.lidar_mapped.copy()

    process_device = process

    def match(self, corner, surf, pose):
        """prepareFeatureFrame + optimizeTransform from a Twist, the node's pose state untouched -> (status, pose, stats)."""
        c, s = _xyzi(corner), _xyzi(surf)
        p = np.array(pose, dtype=np.float32).reshape(6)
        st = LslamStats()
        rc = self._check(self.lib.lslam_loc_match(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p), len(s),
                                                  c.shape[1] * 4, _fp(p), C.byref(st)))
        return rc, p, st

    def get_surround(self):
        """prepareFeatureSurround on request -> (corner (n, 4), surf (m, 4))."""
        nc, ns = C.c_size_t(), C.c_size_t()
        self._check(self.lib.lslam_loc_get_surround(self.h, None, 0, C.byref(nc), None, 0, C.byref(ns)))
        c, s = np.zeros((nc.value, 4), np.float32), np.zeros((ns.value, 4), np.float32)
        self._check(self.lib.lslam_loc_get_surround(self.h, _fp(c), len(c), C.byref(nc), _fp(s), len(s), C.byref(ns)))
        return c, s

    def search_stats(self):
        o = LslamLocSearchCounts()
        self._check(self.lib.lslam_loc_search_stats(self.h, C.byref(o)))
        return {f: (int(getattr(o, f)[0]), int(getattr(o, f)[1])) for f, _ in LslamLocSearchCounts._fields_}

    def debug_knn5(self, which, queries):
        """The search's parity tap -> (xyz (nq, 5, 3), d2 (nq, 5), how (nq,))."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        nq = len(q)
        xyz, d2, how = np.zeros((nq, 5, 3), np.float32), np.zeros((nq, 5), np.float32), np.zeros(nq, np.uint8)
        self._check(self.lib.lslam_loc_debug_knn5(self.h, int(which), q.ctypes.data_as(C.c_void_p), nq, q.shape[1] * 4, _fp(xyz), _fp(d2),
                                                  how.ctypes.data_as(c_uint8_p)))
        return xyz, d2, how

    # ---- global re-localisation (lslam_reloc_*) -------------------------------------------------------------------------
    @staticmethod
    def _reloc_opts(rotations, opts):
        o = LslamRelocOpts()
        names = {f for f, _ in LslamRelocOpts._fields_}
        for k, v in opts.items():
            if k not in names:
                raise TypeError("unknown relocalisation option %r" % k)
            setattr(o, k, v)
        if "rot_cyclic" not in opts and getattr(rotations, "rot_cyclic", False):
            o.rot_cyclic = 1
        return o

    @staticmethod
    def _reloc_inputs(corner, surf, rotations, positions):
        c, s = _xyzi(corner), _xyzi(surf)
        if c.shape[1] != s.shape[1]:
            raise ValueError("corner and surf clouds must share a point layout")
        r = np.ascontiguousarray(np.asarray(rotations), dtype=np.float32).reshape(-1, 3)
        p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        return c, s, r, p

    @staticmethod
    def _reloc_result(rc, res):
        cands = [RelocCandidate(int(c.hypothesis), int(c.coarse_score), int(c.status), int(c.rounds), int(c.n_rows),
                                np.array(c.pose, np.float32)) for c in res.candidates[:res.n_candidates]]
        return RelocResult(rc, bool(res.accepted), int(res.winner), int(res.runner_up), float(res.fraction),
                           np.array(res.T, np.float32).reshape(4, 4), int(res.n_hypotheses), int(res.skipped), tuple(res.n_points),
                           tuple(res.n_scored), tuple(res.occupied_voxels), int(res.n_selected), cands, float(res.ms_coarse),
                           float(res.ms_refine))

    def relocalize(self, corner, surf, rotations, positions, **opts):
        """A pose from one sweep and the map alone: every (rotation, position) hypothesis scored on the device, the best few
        refined with the node's matcher -> :class:`RelocResult` (``status``: 0 accepted, NOT_CONVERGED, TOO_FEW_MATCHES).
        ``apply=1`` hands an accepted pose to the node as ``handle_initial_pose`` would.  Options: lslam_reloc_opts."""
        c, s, r, p = self._reloc_inputs(corner, surf, rotations, positions)
        o = self._reloc_opts(rotations, opts)
        res = LslamRelocResult()
        rc = self._check(self.lib.lslam_reloc_relocalize(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p),
                                                         len(s), c.shape[1] * 4, _fp(r), len(r), _fp(p), len(p), C.byref(o),
                                                         C.byref(res)))
        return self._reloc_result(rc, res)

    def reloc_scores(self, corner, surf, rotations, positions, **opts):
        """The coarse stage alone (the same kernels) -> (scores (n_rot, n_pos) int32, top_idx, top_score, RelocResult)."""
        c, s, r, p = self._reloc_inputs(corner, surf, rotations, positions)
        o = self._reloc_opts(rotations, opts)
        res = LslamRelocResult()
        scores = np.zeros(len(r) * len(p), np.int32)
        ti, ts = np.zeros(1024, np.int32), np.zeros(1024, np.int32)
        nt = C.c_int32()
        rc = self._check(self.lib.lslam_reloc_scores(self.h, c.ctypes.data_as(C.c_void_p), len(c), s.ctypes.data_as(C.c_void_p), len(s),
                                                     c.shape[1] * 4, _fp(r), len(r), _fp(p), len(p), C.byref(o),
                                                     scores.ctypes.data_as(c_int32_p), ti.ctypes.data_as(c_int32_p),
                                                     ts.ctypes.data_as(c_int32_p), C.byref(nt), C.byref(res)))
        return scores.reshape(len(r), len(p)), ti[:nt.value].copy(), ts[:nt.value].copy(), self._reloc_result(rc, res)

    def reloc_nms(self, top_idx, rotations, positions, **opts):
        """The host half of the selection: positions in ``top_idx`` of the NMS survivors (no device work)."""
        r = np.asarray(rotations, dtype=np.float32).reshape(-1, 3)
        p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        ti = np.ascontiguousarray(top_idx, dtype=np.int32)
        o = self._reloc_opts(rotations, opts)
        keep = np.zeros(64, np.int32)
        n = self._check(self.lib.lslam_reloc_nms(ti.ctypes.data_as(c_int32_p), len(ti), _fp(p), len(r), len(p), C.byref(o),
                                                 keep.ctypes.data_as(c_int32_p)))
        return keep[:n].copy()

    def reloc_occupied(self, which, queries, voxel=0.0):
        """Tap of the occupancy sets: 1 where the query point's voxel holds a map point of type ``which``."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        out = np.zeros(len(q), np.uint8)
        self._check(self.lib.lslam_reloc_occupied(self.h, int(which), float(voxel), q.ctypes.data_as(C.c_void_p), len(q), q.shape[1] * 4,
                                                  out.ctypes.data_as(c_uint8_p)))
        return out

    def reloc_info(self):
        o = LslamRelocMapStats()
        self._check(self.lib.lslam_reloc_info(self.h, C.byref(o)))
        return dict(occupied_voxels=tuple(o.occupied_voxels), table_slots=int(o.table_slots), builds=int(o.builds),
                    voxel=float(o.voxel), valid=int(o.valid))
