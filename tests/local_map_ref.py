"""The reference's sliding-window local mapper restated with oracle calls and numpy only (a helper of
tests/test_local_map_abi.py and tests/test_gpu_local_map.py, not a conftest):

* ``LocalFeatureMap`` (io_module/LocalFeatureMap.h) with ``FrameUpdater`` (io_module/FrameUpdater.hpp): the path length
  and ``clean()`` in float64 -- including the reference's erase of ``n + 1`` frames when ``n`` have fallen behind;
* ``featureMapUpdate`` (odometry/LaserMappingLocal.cpp:68-83): ``p' = R p + t`` in float32 in the device kernel's operation
  order (numpy's elementwise operations do not fuse, so this is exact);
* ``getSurroundFeature``: the frames concatenated in queue order, ``Oracle.voxel_grid`` with the corner / surf leaf;
* ``LaserMappingLocal::process`` over ``Oracle.scanmatch_scan`` (thresholds 0.1 / 0.1, score gate off).
"""
import numpy as np

EMPTY = np.zeros((0, 4), np.float32)


def transform_cloud(T, cloud):
    """pcl::transformPointCloud with an Isometry3f (transform_utils.h:601-614): ((r0 x + r1 y) + r2 z) + t, intensity kept."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    c = np.ascontiguousarray(cloud, np.float32)
    out = c.copy()
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def delta_translation_norm(prev, pose):
    """``(prev.inverse() * pose).translation().norm()`` of two Isometry3d: the inverse is (R^T, -(R^T t)), the product's
    translation R^T t_pose + t_inv, every 3-term sum taken left to right -- float64 throughout."""
    prev, pose = np.asarray(prev, np.float64), np.asarray(pose, np.float64)
    d = np.zeros(3, np.float64)
    for k in range(3):
        a = (prev[0, k] * pose[0, 3] + prev[1, k] * pose[1, 3]) + prev[2, k] * pose[2, 3]
        b = (prev[0, k] * prev[0, 3] + prev[1, k] * prev[1, 3]) + prev[2, k] * prev[2, 3]
        d[k] = a + (-b)
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def frames_to_erase(accums, current, threshold):
    """``LocalFeatureMap::clean`` on the queue's accum values (the frame just pushed included, at the back): the frames at the
    front with ``accum <= current - threshold`` are counted; if there are n > 0 of them, n + 1 frames are erased."""
    n = 0
    for a in accums:
        if a > current - threshold:
            break
        n += 1
    return n + 1 if n > 0 else 0


class RefLocalFeatureMap:
    def __init__(self, oracle, queue_distance=30.0, leaf_corner=0.2, leaf_surf=0.4):
        self.o = oracle
        self.queue_distance = float(queue_distance)
        self.leaf = (float(leaf_corner), float(leaf_surf))
        self.clear()

    def clear(self):
        self.queue = []          # (corner, surf, accum)
        self.accum = 0.0
        self.prev = None
        self.evicted = 0

    def add_data_frame(self, corner_ds, surf_ds, T_map):
        T_map = np.asarray(T_map, np.float32).reshape(4, 4)
        P = T_map.astype(np.float64)  # frame->odom = pose.cast<double>()
        if self.prev is not None:     # FrameUpdater::update: the first frame only stores the pose
            self.accum += delta_translation_norm(self.prev, P)
        self.prev = P
        self.queue.append((transform_cloud(T_map, corner_ds), transform_cloud(T_map, surf_ds), self.accum))
        n = frames_to_erase([f[2] for f in self.queue], self.accum, self.queue_distance)
        assert n <= len(self.queue)
        del self.queue[:n]
        self.evicted += n

    def concatenated(self):
        c = np.concatenate([f[0] for f in self.queue]) if self.queue else EMPTY
        s = np.concatenate([f[1] for f in self.queue]) if self.queue else EMPTY
        return c, s

    def get_surround_feature(self):
        c, s = self.concatenated()
        if len(c):
            c = self.o.voxel_grid(c, self.leaf[0])
        if len(s):
            s = self.o.voxel_grid(s, self.leaf[1])
        return c, s


class RefLaserMappingLocal:
    """``LaserMappingLocal::process`` with oracle calls; Twist <-> Isometry conversions are the ABI's host helpers (``cv``)."""

    def __init__(self, oracle, cv, queue_distance=30.0, leaf_corner=0.2, leaf_surf=0.4):
        self.o, self.cv = oracle, cv
        self.fm = RefLocalFeatureMap(oracle, queue_distance, leaf_corner, leaf_surf)
        self.odom_last = np.eye(4, dtype=np.float32)
        self.mapped_last = np.eye(4, dtype=np.float32)
        self.last_surround = (EMPTY, EMPTY)
        self.last_stats = None  # None: no match on this sweep (empty window)

    def match(self, corner_last, surf_last, odom_new):
        """Everything up to the new map pose; nothing of the chain's state changes.  -> (pose 4x4, corner_ds, surf_ds)"""
        odom_new = np.asarray(odom_new, np.float32).reshape(4, 4)
        new = (self.mapped_last @ np.linalg.inv(self.odom_last) @ odom_new).astype(np.float32)
        cds, sds = self.o.voxel_grid(corner_last, 1.0), self.o.voxel_grid(surf_last, 1.0)
        mc, ms = self.fm.get_surround_feature()
        self.last_surround, self.last_stats = (mc, ms), None
        if len(mc) or len(ms):
            opts = self.o.default_opts()
            opts.delta_t_abort = opts.delta_r_abort = 0.1
            opts.use_score = 0
            ok, pose, st = self.o.scanmatch_scan(mc, ms, cds, sds, self.cv.isometry_to_pose(new), opts)
            self.last_stats = st
            if st.status != 1:
                new = self.cv.pose_to_isometry(pose)
        return new, cds, sds

    def commit(self, new, cds, sds, odom_new):
        """transformUpdate + featureMapUpdate at the pose ``new`` (the chain's own, or the device's to keep both on one input)."""
        self.mapped_last, self.odom_last = np.array(new, np.float32), np.array(odom_new, np.float32).reshape(4, 4)
        self.fm.add_data_frame(cds, sds, new)

    def process(self, corner_last, surf_last, odom_new):
        new, cds, sds = self.match(corner_last, surf_last, odom_new)
        self.commit(new, cds, sds, odom_new)
        return new
