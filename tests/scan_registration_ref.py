"""The registration node's IMU branch restated on the CPU (a helper of tests/test_scan_registration_ref.py and
tests/test_gpu_scan_registration.py, not a conftest), written from the reference's arithmetic:

* ``ImuHistory``: ``ScanRegistration::handleIMUMessage`` (odometry/ScanRegistration.cpp:89-120) -- gravity removed in double,
  the acceleration rotated with ``rotateZXY``, position and velocity integrated in float with a float ``timeDiff`` -- into the
  ring buffer of util/CircularBuffer.h (the oldest state overwritten when full);
* ``walk_indices``: ``interpolateIMUStateFor`` 's index exactly as the reference moves it -- one index, walked forward while the
  points are visited in arrival order, never back; ``closed_form_indices`` (prefix maximum + search) and ``per_point_indices``
  (a search per point that forgets the points before it: NOT what the reference does) beside it;
* ``states_for``: the three cases of ``interpolateIMUStateFor`` and ``IMUState::interpolate`` with its yaw wrap;
* ``deskew``: ``setIMUTransformFor`` + ``transformToStartIMU`` (:150-169, util/math_utils.h:115-236);
* ``register_points``: ring and relTime of ``MultiScanRegistration::process`` (:95-168) in arrival order;
* ``process``: the whole of ``MultiScanRegistration::process`` up to the ring-sorted cloud and its ranges, and ``_imuTrans``
  (ScanRegistration.cpp:684-707).

Number formats: every float of the reference is a numpy float32 here, every double a float64; numpy's elementwise operations
round once per operation and do not fuse.  sin / cos of an interpolated angle are ``float32(sin(float64(x)))``, the correctly
rounded value (numpy's float32 sin / cos are not; glibc's sinf / cosf, which the reference's ``Angle`` calls, differ from it by
one ulp for about 1.3 % of angles -- which is why the de-skewed coordinates are held to a bound and not to bits).  A state that
is pushed caches the C library's ``sinf`` / ``cosf`` of its angles, as ``Angle(float)`` does on the host: the rotation of the
acceleration in ``handleIMUMessage`` and the states used as they are carry those values.
"""
import ctypes
import ctypes.util
import math

import numpy as np

F = np.float32
PI = math.pi


def sin32(x):
    return np.sin(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def cos32(x):
    return np.cos(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = ctypes.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [ctypes.c_float]


def angle_cache(ang):
    """What three Angle(float) cache on the host: (sin roll, cos roll, sin pitch, cos pitch, sin yaw, cos yaw) of libm."""
    return np.array([f(float(a)) for a in np.asarray(ang, np.float32) for f in (_libm.sinf, _libm.cosf)], np.float32)


def to_sec(d_ns):
    """ros::Duration::toSec() of an exact nanosecond difference: sec + 1e-9 * nsec, 0 <= nsec < 1e9."""
    sec, nsec = divmod(int(d_ns), 10 ** 9)
    return float(sec) + 1e-9 * float(nsec)


def rot(c, s, u, v):
    """(c u - s v, s u + c v) in float32: rotZ on (x, y), rotX on (y, z), rotY on (z, x)."""
    return c * u - s * v, s * u + c * v


def rotate_zxy(p, trig):
    """rotateZXY(p, roll, pitch, yaw); trig = (sin roll, cos roll, sin pitch, cos pitch, sin yaw, cos yaw)."""
    x, y, z = p
    sr, cr, sp, cp, sy, cy = trig
    x, y = rot(cr, sr, x, y)
    y, z = rot(cp, sp, y, z)
    z, x = rot(cy, sy, z, x)
    return x, y, z


def rotate_yxz_neg(p, trig):
    """rotateYXZ(p, -yaw, -pitch, -roll): Angle::operator- negates the sine and keeps the cosine."""
    x, y, z = p
    sr, cr, sp, cp, sy, cy = trig
    z, x = rot(cy, -sy, z, x)
    y, z = rot(cp, -sp, y, z)
    x, y = rot(cr, -sr, x, y)
    return x, y, z


class ImuHistory:
    """_imuHistory: states as rows {roll, pitch, yaw, position[3], velocity[3], the six cached sin / cos} (float32) with int
    stamps (ns)."""

    def __init__(self, capacity=200):
        self.capacity = int(capacity)
        self.stamps = []
        self.rows = []

    def __len__(self):
        return len(self.stamps)

    def push(self, stamp_ns, roll, pitch, yaw, la):
        acc = np.array([F(la[1] - math.sin(roll) * math.cos(pitch) * 9.81),
                        F(la[2] - math.cos(roll) * math.cos(pitch) * 9.81),
                        F(la[0] + math.sin(pitch) * 9.81)], np.float32)
        ang = np.array([roll, pitch, yaw], np.float32)
        pos, vel = np.zeros(3, np.float32), np.zeros(3, np.float32)
        trig = angle_cache(ang)
        if self.stamps:
            acc = np.array(rotate_zxy(tuple(acc), tuple(trig)), np.float32)
            prev = self.rows[-1]
            dt = F(to_sec(stamp_ns - self.stamps[-1]))
            pos = (prev[3:6] + prev[6:9] * dt) + ((F(0.5) * acc) * dt) * dt
            vel = prev[6:9] + acc * dt
        self.stamps.append(int(stamp_ns))
        self.rows.append(np.concatenate([ang, pos, vel, trig]).astype(np.float32))
        if len(self.stamps) > self.capacity:  # CircularBuffer::push on a full buffer
            self.stamps.pop(0)
            self.rows.pop(0)

    def arrays(self, scan_time_ns):
        """(tsec[k] = (scanTime - stamp).toSec(), dt_prev[k], rows (k, 15))."""
        tsec = np.array([to_sec(scan_time_ns - s) for s in self.stamps], np.float64)
        dt = np.array([0.0] + [to_sec(b - a) for a, b in zip(self.stamps[:-1], self.stamps[1:])], np.float64)
        return tsec, dt, np.stack(self.rows).astype(np.float32)


def walk_indices(tsec, rel, start=0):
    """The reference's loop, literally: for every kept point in arrival order
    ``while idx < size - 1 and tsec[idx] + relTime > 0: idx += 1``.  Returns (index per point, the index it ends on)."""
    idx, last = int(start), len(tsec) - 1
    ts = [float(t) for t in tsec]
    out = np.empty(len(rel), np.int64)
    for i, r in enumerate(np.asarray(rel, np.float32).astype(np.float64).tolist()):
        while idx < last and ts[idx] + r > 0:
            idx += 1
        out[i] = idx
    return out, idx


def first_index(tsec, t):
    """f(t): the first index with tsec + t <= 0, or the last index."""
    hit = np.nonzero(np.asarray(tsec, np.float64) + float(t) <= 0)[0]
    return int(hit[0]) if len(hit) else len(tsec) - 1


def closed_form_indices(tsec, rel, keep=None):
    """f(max(0, the largest relTime among the kept points so far)): what the device computes with a prefix maximum and a binary
    search.  keep (optional): rel holds EVERY point of the cloud and keep says which are kept -- a dropped point contributes the
    identity of the maximum, whatever its relTime; the indices of the kept points are returned."""
    rel = np.asarray(rel, np.float32)
    keep = np.ones(len(rel), bool) if keep is None else np.asarray(keep, bool)
    pm = np.maximum.accumulate(np.where(keep, np.maximum(rel, F(0)), F(0))) if len(rel) else rel
    return np.array([first_index(tsec, t) for t in pm[keep].astype(np.float64)], np.int64)


def per_point_indices(tsec, rel):
    """A search per point that does not remember the points before it -- differs from the reference when relTime goes back."""
    return np.array([first_index(tsec, max(0.0, float(t))) for t in np.asarray(rel, np.float32)], np.int64)


def states_for(tsec, dt_prev, rows, idx, rel):
    """interpolateIMUStateFor for points with the given history index: -> (angles (n, 3), trig (n, 6), pos (n, 3), vel (n, 3))."""
    idx = np.asarray(idx, np.int64)
    rel = np.asarray(rel, np.float32)
    time_diff = tsec[idx] + rel.astype(np.float64)
    raw = (idx == 0) | (time_diff > 0)
    S, E = rows[idx], rows[np.maximum(idx - 1, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (-time_diff / dt_prev[idx]).astype(np.float32)
    ratio = np.where(raw, F(0), ratio).astype(np.float32)
    inv = F(1) - ratio
    ang = np.empty((len(idx), 3), np.float32)
    ang[:, 0] = S[:, 0] * inv + E[:, 0] * ratio
    ang[:, 1] = S[:, 1] * inv + E[:, 1] * ratio
    dyaw = (S[:, 2] - E[:, 2]).astype(np.float64)
    head = (S[:, 2] * inv).astype(np.float64)
    up = (head + (E[:, 2].astype(np.float64) + 2 * PI) * ratio.astype(np.float64)).astype(np.float32)
    down = (head + (E[:, 2].astype(np.float64) - 2 * PI) * ratio.astype(np.float64)).astype(np.float32)
    plain = S[:, 2] * inv + E[:, 2] * ratio
    ang[:, 2] = np.where(dyaw > PI, up, np.where(dyaw < -PI, down, plain))
    vel = S[:, 6:9] * inv[:, None] + E[:, 6:9] * ratio[:, None]
    pos = S[:, 3:6] * inv[:, None] + E[:, 3:6] * ratio[:, None]
    ang[raw], pos[raw], vel[raw] = S[raw, 0:3], S[raw, 3:6], S[raw, 6:9]
    s, c = sin32(ang), cos32(ang)
    trig = np.stack([s[:, 0], c[:, 0], s[:, 1], c[:, 1], s[:, 2], c[:, 2]], 1)
    trig[raw] = S[raw, 9:15]  # a state used as it is keeps what it cached when it was pushed
    return ang, trig, pos.astype(np.float32), vel.astype(np.float32)


def deskew(xyz, rel, cur, start):
    """setIMUTransformFor + transformToStartIMU; cur = states_for(...) per point, start = the same for the single start state.
    Returns (de-skewed xyz (n, 3), the shifts (n, 3))."""
    _, trig, pos, _ = cur
    _, trig0, pos0, vel0 = start
    rel = np.asarray(rel, np.float32)
    shift = (pos - pos0[0]) - vel0[0] * rel[:, None]
    p = rotate_zxy((xyz[:, 0], xyz[:, 1], xyz[:, 2]), tuple(trig[:, k] for k in range(6)))
    p = tuple(p[d] + shift[:, d] for d in range(3))
    p = rotate_yxz_neg(p, tuple(trig0[0, k] for k in range(6)))
    return np.stack(p, 1).astype(np.float32), shift.astype(np.float32)


def register_points(raw, lower_deg, upper_deg, n_rings, scan_period=0.1):
    """Ring and relTime of every point in arrival order (MultiScanRegistration.cpp:95-168): -> (xyz' (n, 3) in the swapped axes,
    ring (n,) with -1 for dropped points, relTime (n,) float32)."""
    raw = np.ascontiguousarray(raw, np.float32)
    n = len(raw)
    with np.errstate(all="ignore"):
        start_ori = F(-F(math.atan2(float(raw[0, 1]), float(raw[0, 0]))))
        end_ori = F(F(-F(math.atan2(float(raw[-1, 1]), float(raw[-1, 0])))) + F(2) * F(PI))
        if float(F(end_ori - start_ori)) > 3 * PI:
            end_ori = F(float(end_ori) - 2 * PI)
        elif float(F(end_ori - start_ori)) < PI:
            end_ori = F(float(end_ori) + 2 * PI)
        x, y, z = raw[:, 1], raw[:, 2], raw[:, 0]
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d2 = (x * x + y * y) + z * z
        ok &= ~(d2.astype(np.float64) < 0.0001)
        angle = np.arctan((y / np.sqrt(x * x + z * z)).astype(np.float64)).astype(np.float32)
        factor = F(F(n_rings - 1) / (F(upper_deg) - F(lower_deg)))
        idf = ((angle * F(180)).astype(np.float64) / PI - float(F(lower_deg))) * float(factor) + 0.5
        ring = np.where(ok & np.isfinite(idf), np.trunc(np.where(np.isfinite(idf), idf, 0.0)), -1).astype(np.int64)
        ok &= (ring >= 0) & (ring < n_rings)
        ring = np.where(ok, ring, -1)
        ori0 = (-np.arctan2(x.astype(np.float64), z.astype(np.float64)).astype(np.float32)).astype(np.float32)
        so, eo = float(start_ori), float(end_ori)
        o64 = ori0.astype(np.float64)
        mode_a = np.where(o64 < so - PI / 2, (o64 + 2 * PI).astype(np.float32),
                          np.where(o64 > so + PI * 3 / 2, (o64 - 2 * PI).astype(np.float32), ori0)).astype(np.float32)
        flips = np.nonzero(ok & ((mode_a - start_ori).astype(np.float64) > PI))[0]
        first_half = int(flips[0]) if len(flips) else n  # the point that flips halfPassed is itself still "not passed"
        b = (o64 + 2 * PI).astype(np.float32)
        b64 = b.astype(np.float64)
        mode_b = np.where(b64 < eo - PI * 3 / 2, (b64 + 2 * PI).astype(np.float32),
                          np.where(b64 > eo + PI / 2, (b64 - 2 * PI).astype(np.float32), b)).astype(np.float32)
        ori = np.where(np.arange(n) <= first_half, mode_a, mode_b).astype(np.float32)
        rel = (F(scan_period) * (ori - start_ori)) / F(end_ori - start_ori)
    return np.stack([x, y, z], 1), ring, rel.astype(np.float32)


class Registration:
    """MultiScanRegistration with its members that live across sweeps: the history, _imuStart, _imuCur, _imuPositionShift."""

    def __init__(self, lower_deg=-15.0, upper_deg=15.0, n_rings=16, scan_period=0.1, imu_history_size=200, index_rule="walk"):
        self.lower, self.upper, self.n_rings, self.scan_period = lower_deg, upper_deg, int(n_rings), scan_period
        self.history = ImuHistory(imu_history_size)
        self.index_rule = index_rule
        self.start_ang, self.start_trig = np.zeros(3, np.float32), np.array([0, 1, 0, 1, 0, 1], np.float32)
        self.start_vel = np.zeros(3, np.float32)
        self.cur_ang, self.cur_vel, self.shift = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)

    def process(self, raw, scan_time_ns):
        """-> dict(cloud (m, 4) ring-sorted, ranges (n_rings, 2), imu_trans (4, 3), plus the arrival-order arrays
        xyz_raw / xyz / ring / rel / index / shift of the kept points)."""
        xyz, ring, rel = register_points(raw, self.lower, self.upper, self.n_rings, self.scan_period)
        keep = ring >= 0
        xyz_k, ring_k, rel_k = xyz[keep], ring[keep], rel[keep]
        out_xyz, idx, shifts = xyz_k, np.zeros(len(rel_k), np.int64), np.zeros((len(rel_k), 3), np.float32)
        if len(self.history):
            tsec, dt_prev, rows = self.history.arrays(scan_time_ns)
            i0, _ = walk_indices(tsec, np.zeros(1, np.float32))  # reset(): _imuIdx = 0, interpolateIMUStateFor(0, _imuStart)
            start = states_for(tsec, dt_prev, rows, i0, np.zeros(1, np.float32))
            self.start_ang, self.start_trig, self.start_vel = start[0][0], start[1][0], start[3][0]
            if self.index_rule == "walk":
                idx, _ = walk_indices(tsec, rel_k, start=i0[0])
            elif self.index_rule == "closed":
                idx = closed_form_indices(tsec, rel_k)
            else:
                idx = per_point_indices(tsec, rel_k)
            if len(rel_k):
                cur = states_for(tsec, dt_prev, rows, idx, rel_k)
                out_xyz, shifts = deskew(xyz_k, rel_k, cur, start)
                self.cur_ang, self.cur_vel, self.shift = cur[0][-1], cur[3][-1], shifts[-1]
        order = np.argsort(ring_k, kind="stable")
        cloud = np.concatenate([out_xyz, (ring_k.astype(np.float32) + rel_k)[:, None]], 1).astype(np.float32)[order]
        ranges = np.zeros((self.n_rings, 2), np.int32)
        total = 0
        for r in range(self.n_rings):  # IndexRange(first, last), MultiScanRegistration.cpp:184-189
            ranges[r, 0] = total
            total += int((ring_k == r).sum())
            ranges[r, 1] = total - 1 if total > 0 else 0
        return dict(cloud=cloud, ranges=ranges, imu_trans=self.imu_trans(), xyz_raw=xyz_k, xyz=out_xyz, ring=ring_k, rel=rel_k,
                    index=idx, order=order, shift=shifts)

    def imu_trans(self):
        """_imuTrans: {start pitch, yaw, roll}, {cur pitch, yaw, roll}, shift and velocity change in the start frame."""
        t = np.zeros((4, 3), np.float32)
        t[0] = self.start_ang[[1, 2, 0]]
        t[1] = self.cur_ang[[1, 2, 0]]
        t[2] = rotate_yxz_neg(tuple(self.shift), tuple(self.start_trig))
        t[3] = rotate_yxz_neg(tuple(self.cur_vel - self.start_vel), tuple(self.start_trig))
        return t
