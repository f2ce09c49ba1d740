"""Host-side mirror of the feature-extraction front end: ``ScanRegistration::extractFeatures``
(/root/reference/L_SLAM/src/odometry/ScanRegistration.cpp:190-425) over the C ABI
(``lslam_extract_features``, kernels in ``csrc/lslam_features.hip``)."""
import ctypes as C

import numpy as np

from .capi import LslamError, LslamOregStats, LslamRegParams, LslamSregStats, c_double_p, c_float_p, c_int32_p

LISTS = ("sharp", "less_sharp", "flat", "less_flat")


class FeatureSet:
    """A sweep's four feature clouds in HBM (``lslam_fset``): what the registration node hands the odometry node
    without a trip through the host.  Filled by :func:`extract_features_dev` or :meth:`upload`; complete when that call
    returns, free for the next fill once the ``DeviceLaserOdometry.process`` that consumed it has returned."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        rc = ctx.lib.lslam_fset_create(ctx.h, C.byref(h))
        if rc < 0:
            raise LslamError(rc, ctx.lib.lslam_last_error().decode())
        self.h = h

    def counts(self):
        c = (C.c_size_t * 4)()
        self.ctx.lib.lslam_fset_counts(self.h, c)
        return dict(zip(LISTS, (int(v) for v in c)))

    def upload(self, sharp, less_sharp, flat, less_flat, ctx=None):
        ctx = ctx or self.ctx
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (sharp, less_sharp, flat, less_flat)]
        args = []
        for a in arrs:
            args += [a.ctypes.data_as(C.c_void_p), len(a)]
        rc = ctx.lib.lslam_fset_upload(ctx.h, self.h, *args, 16)
        if rc < 0:
            raise LslamError(rc, ctx.lib.lslam_last_error().decode())
        return self

    def download(self, which, ctx=None):
        ctx = ctx or self.ctx
        k = LISTS.index(which) if isinstance(which, str) else int(which)
        n = list(self.counts().values())[k]
        out = np.zeros((n, 4), np.float32)
        m = C.c_size_t()
        rc = ctx.lib.lslam_fset_download(ctx.h, self.h, k, out.ctypes.data_as(c_float_p), n, C.byref(m))
        if rc < 0:
            raise LslamError(rc, ctx.lib.lslam_last_error().decode())
        return out

    def close(self):
        if self.h:
            self.ctx.lib.lslam_fset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def extract_features_dev(ctx, cloud, scan_ranges, fset, params=None, intensity_field=3):
    """:func:`extract_features` with the four lists left in HBM (``fset``); returns their sizes."""
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 4:
        raise ValueError("cloud must be (n, >=4) float32")
    r = np.ascontiguousarray(scan_ranges, dtype=np.int32).reshape(-1, 2)
    counts = (C.c_size_t * 4)()
    rc = ctx.lib.lslam_extract_features_dev(ctx.h, a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4, int(intensity_field) * 4,
                                            r.ctypes.data_as(c_int32_p), len(r), C.byref(params) if params is not None else None,
                                            fset.h, counts)
    if rc < 0:
        raise LslamError(rc, ctx.lib.lslam_last_error().decode())
    return dict(zip(LISTS, (int(v) for v in counts)))


def default_params(ctx):
    p = LslamRegParams()
    ctx.lib.lslam_reg_default_params(C.byref(p))
    return p


def extract_features(ctx, cloud, scan_ranges, params=None, intensity_field=3, taps=False):
    """cloud: (n, >=4) float32, xyz first, ``intensity_field`` = column copied to the outputs'
    intensity; scan_ranges: (rings, 2) inclusive [first, last].  Returns a dict with the four feature
    clouds ``sharp``, ``less_sharp``, ``flat``, ``less_flat`` ((m, 4) each) and, with ``taps``, the
    per-point ``curvature``, ``picked`` (marks after setScanBuffersFor) and ``label``."""
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 4:
        raise ValueError("cloud must be (n, >=4) float32")
    r = np.ascontiguousarray(scan_ranges, dtype=np.int32).reshape(-1, 2)
    n = len(a)
    outs = [ctx.scratch("features%d" % k, n, 4) for k in range(4)]
    counts = (C.c_size_t * 4)()
    curv = np.zeros(n, np.float32) if taps else None
    picked = np.zeros(n, np.int8) if taps else None
    label = np.zeros(n, np.int8) if taps else None
    fp = lambda x: x.ctypes.data_as(c_float_p) if x is not None else None
    bp = lambda x: x.ctypes.data_as(C.POINTER(C.c_int8)) if x is not None else None
    rc = ctx.lib.lslam_extract_features(ctx.h, a.ctypes.data_as(C.c_void_p), n, a.shape[1] * 4,
                                        int(intensity_field) * 4, r.ctypes.data_as(c_int32_p), len(r),
                                        C.byref(params) if params is not None else None, fp(outs[0]), fp(outs[1]),
                                        fp(outs[2]), fp(outs[3]), counts, fp(curv), bp(picked), bp(label))
    if rc < 0:
        raise LslamError(rc, ctx.lib.lslam_last_error().decode())
    res = dict(sharp=outs[0][:counts[0]].copy(), less_sharp=outs[1][:counts[1]].copy(),
               flat=outs[2][:counts[2]].copy(), less_flat=outs[3][:counts[3]].copy())
    if taps:
        res.update(curvature=curv, picked=picked, label=label)
    return res


def multiscan_register(ctx, cloud, lower_deg, upper_deg, n_rings, scan_period=0.1):
    """MultiScanRegistration::process (no IMU): raw driver cloud (n, >=3) -> (ring-sorted (m, 4)
    {x', y', z', ring + relTime}, ranges (n_rings, 2)) -- the inputs of :func:`extract_features`."""
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    out = ctx.scratch("multiscan", len(a), 4)
    ranges = np.zeros((int(n_rings), 2), np.int32)
    n = C.c_size_t()
    rc = ctx.lib.lslam_multiscan_register(ctx.h, a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4,
                                          float(lower_deg), float(upper_deg), int(n_rings), float(scan_period),
                                          out.ctypes.data_as(c_float_p), len(a), C.byref(n),
                                          ranges.ctypes.data_as(c_int32_p))
    if rc < 0:
        raise LslamError(rc, ctx.lib.lslam_last_error().decode())
    return out[:n.value].copy(), ranges


def rpy_from_quaternion(x, y, z, w):
    """tf::Matrix3x3(q).getRPY(roll, pitch, yaw) (solution_number 1, the default): of the two Euler triples of a rotation the
    one with pitch in [-pi/2, pi/2]; at the gimbal lock (|m20| >= 1) yaw is 0."""
    import math
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    m00, m10, m20 = 1.0 - s * (y * y + z * z), s * (x * y + w * z), s * (x * z - w * y)
    m21, m22 = s * (y * z + w * x), 1.0 - s * (x * x + y * y)
    if abs(m20) >= 1.0:  # gimbal lock: yaw = 0, roll = atan2(m21, m22) as tf forms it
        return math.atan2(m21, m22), (math.pi / 2.0 if m20 < 0 else -math.pi / 2.0), 0.0
    pitch = -math.asin(m20)
    c = math.cos(pitch)
    return math.atan2(m21 / c, m22 / c), pitch, math.atan2(m10 / c, m00 / c)


class MultiScanRegistration:
    """``lidar_slam::MultiScanRegistration`` as a node on the device (``lslam_sreg_*``): raw driver cloud in, the sweep's four
    feature lists in a :class:`FeatureSet` out -- ring and relTime, the IMU de-skew (whenever :meth:`handle_imu_message` has
    been called), the grouping by ring, the ranges and the extraction without a trip through the host, one wait per sweep."""
    SYSTEM_DELAY = 2  # ScanRegistration.h: the first clouds of a session are skipped

    def __init__(self, ctx, lower_deg=-15.0, upper_deg=15.0, n_rings=16, scan_period=0.1, params=None, imu_history_size=200):
        self.ctx = ctx
        self.n_rings = int(n_rings)
        h = C.c_void_p()
        rc = ctx.lib.lslam_sreg_create(ctx.h, C.byref(params) if params is not None else None, float(lower_deg), float(upper_deg),
                                       self.n_rings, float(scan_period), int(imu_history_size), C.byref(h))
        if rc < 0:
            raise LslamError(rc, ctx.lib.lslam_last_error().decode())
        self.h = h
        self.system_delay = self.SYSTEM_DELAY
        self.cloud_receive_count = 0
        self.imu_trans = np.zeros((4, 3), np.float32)
        self.last_stats = LslamSregStats()
        self.fset = None

    def _check(self, rc):
        if rc < 0:
            raise LslamError(rc, self.ctx.lib.lslam_last_error().decode())

    def handle_imu_message(self, stamp_ns, rpy, linear_acceleration):
        """handleIMUMessage after getRPY: ``rpy`` in radians, ``linear_acceleration`` {x, y, z} in the IMU's axes."""
        la = (C.c_double * 3)(*[float(v) for v in linear_acceleration])
        self._check(self.ctx.lib.lslam_sreg_imu_push(self.h, int(stamp_ns), float(rpy[0]), float(rpy[1]), float(rpy[2]), la))

    def handle_imu_quaternion(self, stamp_ns, orientation_xyzw, linear_acceleration):
        self.handle_imu_message(stamp_ns, rpy_from_quaternion(*[float(v) for v in orientation_xyzw]), linear_acceleration)

    def has_imu_data(self):
        return self.imu_info()[0] > 0

    def imu_info(self):
        n = C.c_int32()
        pos, vel = (C.c_double * 3)(), (C.c_double * 3)()
        self._check(self.ctx.lib.lslam_sreg_imu_info(self.h, C.byref(n), pos, vel))
        return n.value, np.array(pos), np.array(vel)

    def imu_clear(self):
        self._check(self.ctx.lib.lslam_sreg_imu_clear(self.h))

    def process(self, cloud, stamp_ns, fset):
        """MultiScanRegistration::process: cloud (n, >=3) float32 in arrival order; returns the four lists' sizes."""
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("cloud must be (n, >=3) float32")
        counts = (C.c_size_t * 4)()
        trans = np.zeros((4, 3), np.float32)
        rc = self.ctx.lib.lslam_sreg_process(self.h, a.ctypes.data_as(C.c_void_p), len(a), a.shape[1] * 4, int(stamp_ns), fset.h, counts,
                                             trans.ctypes.data_as(c_float_p), C.byref(self.last_stats))
        self._check(rc)
        self.imu_trans = trans
        return dict(zip(LISTS, (int(v) for v in counts)))

    def handle_cloud_message(self, cloud, stamp_ns, fset=None):
        """handleCloudMessage: the first SYSTEM_DELAY clouds are dropped (returns None), the others processed into ``fset`` (or a
        feature set of the node's own, ``self.fset``)."""
        self.cloud_receive_count += 1
        if self.system_delay > 0:
            self.system_delay -= 1
            return None
        if fset is None:
            if self.fset is None:
                self.fset = FeatureSet(self.ctx)
            fset = self.fset
        return self.process(cloud, stamp_ns, fset)

    def cloud(self):
        """The last sweep's registered cloud (m, 4) {x', y', z', ring + relTime} and its (n_rings, 2) ranges."""
        n = C.c_size_t()
        ranges = np.zeros((self.n_rings, 2), np.int32)
        self._check(self.ctx.lib.lslam_sreg_cloud(self.h, None, 0, C.byref(n), ranges.ctypes.data_as(c_int32_p)))
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            self._check(self.ctx.lib.lslam_sreg_cloud(self.h, out.ctypes.data_as(c_float_p), len(out), C.byref(n), None))
        return out, ranges

    def close(self):
        if self.h:
            self.ctx.lib.lslam_sreg_destroy(self.h)
            self.h = None
        if self.fset is not None:
            self.fset.close()
            self.fset = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_organised(xyz, ring):
    """An (H, W, >=3) float32 image and its (H, W) uint16 rings as the node's device format: (H, W) cells of 16 bytes,
    {x, y, z, word} with the ring in the low 16 bits of word."""
    xyz = np.asarray(xyz, np.float32)
    ring = np.asarray(ring)
    if xyz.ndim != 3 or xyz.shape[2] < 3 or ring.shape != xyz.shape[:2]:
        raise ValueError("image must be (H, W, >=3) float32 with an (H, W) ring array")
    cells = np.zeros(xyz.shape[:2] + (4,), np.float32)
    cells[..., :3] = xyz[..., :3]
    cells[..., 3] = ring.astype(np.uint16).astype(np.uint32).view(np.float32)
    return cells


class OrganisedScanRegistration:
    """``lidar_slam::OrganisedScanRegistration`` as a node on the device (``lslam_oreg_*``): a height x width cloud whose points
    carry their ring in, the sweep's four feature lists in a :class:`FeatureSet` out -- validity, relTime from the column, the
    rows concatenated (a stable compaction), the ranges and the extraction without a trip through the host, one wait per sweep.
    As in the reference an IMU that has been heard changes ``imu_trans`` only: the points are not de-skewed."""
    SYSTEM_DELAY = 2  # OrganisedScanRegistration.h: the first clouds of a session are skipped

    def __init__(self, ctx, scan_period=0.1, blind_radius=2.5, params=None, imu_history_size=200):
        self.ctx = ctx
        h = C.c_void_p()
        rc = ctx.lib.lslam_oreg_create(ctx.h, C.byref(params) if params is not None else None, float(scan_period), float(blind_radius),
                                       int(imu_history_size), C.byref(h))
        if rc < 0:
            raise LslamError(rc, ctx.lib.lslam_last_error().decode())
        self.h = h
        self.system_delay = self.SYSTEM_DELAY
        self.cloud_receive_count = 0
        self.imu_trans = np.zeros((4, 3), np.float32)
        self.last_stats = LslamOregStats()
        self.height = 0  # of the last sweep that succeeded: the rows of cloud()'s ranges
        self.fset = None

    def _check(self, rc):
        if rc < 0:
            raise LslamError(rc, self.ctx.lib.lslam_last_error().decode())

    def handle_imu_message(self, stamp_ns, rpy, linear_acceleration):
        """handleIMUMessage after getRPY: ``rpy`` in radians, ``linear_acceleration`` {x, y, z} in the IMU's axes."""
        la = (C.c_double * 3)(*[float(v) for v in linear_acceleration])
        self._check(self.ctx.lib.lslam_oreg_imu_push(self.h, int(stamp_ns), float(rpy[0]), float(rpy[1]), float(rpy[2]), la))

    def handle_imu_quaternion(self, stamp_ns, orientation_xyzw, linear_acceleration):
        self.handle_imu_message(stamp_ns, rpy_from_quaternion(*[float(v) for v in orientation_xyzw]), linear_acceleration)

    def has_imu_data(self):
        return self.imu_info()[0] > 0

    def imu_info(self):
        n = C.c_int32()
        pos, vel = (C.c_double * 3)(), (C.c_double * 3)()
        self._check(self.ctx.lib.lslam_oreg_imu_info(self.h, C.byref(n), pos, vel))
        return n.value, np.array(pos), np.array(vel)

    def imu_clear(self):
        self._check(self.ctx.lib.lslam_oreg_imu_clear(self.h))

    def process(self, cloud, stamp_ns, fset, ring=None, ring_offset=None):
        """OrganisedScanRegistration::process.  ``cloud``: with ``ring`` an (H, W, >=3) float32 image and ``ring`` its (H, W)
        uint16 rings (packed into the 16-byte form here); without, an (H, W) structured array with float32 fields ``x``, ``y``,
        ``z`` first and a uint16 field ``ring`` (any itemsize that is a multiple of 4: the reference's PointXYZIT has 32, ring at
        26), or an (H, W, k) float32 array whose points are read as raw bytes with the ring at byte ``ring_offset`` (default 12).
        Returns the four lists' sizes."""
        if ring is not None:
            a = pack_organised(cloud, ring)
            stride, off = 16, 12
        else:
            a = np.ascontiguousarray(cloud)
            if a.dtype.names:
                if a.ndim != 2 or a.dtype.names[:3] != ("x", "y", "z") or a.dtype.fields["x"][1] != 0 or "ring" not in a.dtype.names:
                    raise ValueError("structured cloud must be (H, W) with x, y, z first and a ring field")
                stride, off = a.dtype.itemsize, a.dtype.fields["ring"][1] if ring_offset is None else int(ring_offset)
            else:
                if a.ndim != 3 or a.dtype != np.float32 or a.shape[2] < 3:
                    raise ValueError("cloud must be (H, W, >=3) float32, or structured, or come with ring=")
                stride, off = a.shape[2] * 4, 12 if ring_offset is None else int(ring_offset)
        height, width = a.shape[:2]
        counts = (C.c_size_t * 4)()
        trans = np.zeros((4, 3), np.float32)
        rc = self.ctx.lib.lslam_oreg_process(self.h, a.ctypes.data_as(C.c_void_p), height, width, stride, off, int(stamp_ns), fset.h, counts,
                                             trans.ctypes.data_as(c_float_p), C.byref(self.last_stats))
        self._check(rc)
        self.imu_trans = trans
        self.height = height
        return dict(zip(LISTS, (int(v) for v in counts)))

    def handle_cloud_message(self, cloud, stamp_ns, fset=None, ring=None):
        """handleCloudMessage: the first SYSTEM_DELAY clouds are dropped (returns None), the others processed into ``fset`` (or a
        feature set of the node's own, ``self.fset``)."""
        self.cloud_receive_count += 1
        if self.system_delay > 0:
            self.system_delay -= 1
            return None
        if fset is None:
            if self.fset is None:
                self.fset = FeatureSet(self.ctx)
            fset = self.fset
        return self.process(cloud, stamp_ns, fset, ring=ring)

    def cloud(self):
        """The last sweep's registered cloud (m, 4) {x, y, z, ring + relTime} and its (height, 2) ranges."""
        n = C.c_size_t()
        ranges = np.zeros((self.height, 2), np.int32)
        self._check(self.ctx.lib.lslam_oreg_cloud(self.h, None, 0, C.byref(n), ranges.ctypes.data_as(c_int32_p)))
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            self._check(self.ctx.lib.lslam_oreg_cloud(self.h, out.ctypes.data_as(c_float_p), len(out), C.byref(n), None))
        return out, ranges

    def close(self):
        if self.h:
            self.ctx.lib.lslam_oreg_destroy(self.h)
            self.h = None
        if self.fset is not None:
            self.fset.close()
            self.fset = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
