"""The registration node for organised clouds restated on the CPU (a helper of tests/test_organised_registration_ref.py and
tests/test_gpu_organised_registration.py, not a conftest), written from the reference's arithmetic
(odometry/OrganizedScanRegistration.cpp:82-150):

* ``process``: the whole of ``OrganisedScanRegistration::process`` up to the registered cloud and its ranges, vectorised --
  validity (finite coordinates, then ``x*x + y*y + z*z < blind*blind`` drops the point, all float, left to right), ``relTime =
  float(double(scanPeriod) * double(col) / width)``, the 4th channel ``float(ring) + relTime`` with the point's own ring (not
  its row), the per-row clouds concatenated in row order, ``IndexRange(first, size > 0 ? size - 1 : 0)`` per row;
* ``process_literal``: the double loop transcribed, Python floats for the double part and ``np.float32`` for the float part;
* ``imu_trans``: what ``publishResult`` sends for this class, which inherits the IMU subscription but never calls
  ``setIMUTransformFor`` / ``transformToStartIMU``: ``_imuCur`` and ``_imuPositionShift`` stay zero, so the rows are {start
  pitch, yaw, roll}, zeros, the rotated zero shift, ``rotateYXZ(0 - _imuStart.velocity, -yaw, -pitch, -roll)``.  ``_imuStart`` is
  ``interpolateIMUStateFor(0)`` on ``scan_registration_ref.ImuHistory``; an interpolated start state caches the C library's
  ``sinf`` / ``cosf`` of its angles, as ``Angle(float)`` does on the host.

Every float of the reference is a numpy float32 here, every double a float64; numpy rounds once per operation and does not fuse.
"""
import numpy as np

import scan_registration_ref as R

F = np.float32


def rel_times(width, scan_period=0.1):
    """relTime of every column: (double)scanPeriod * (double)col / width, rounded once to float."""
    return (np.float64(F(scan_period)) * np.arange(width, dtype=np.float64) / np.float64(width)).astype(np.float32)


def keep_mask(xyz, blind_radius=2.5):
    xyz = np.asarray(xyz, np.float32)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    with np.errstate(all="ignore"):
        d2 = (x * x + y * y) + z * z
        return np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(d2 < F(blind_radius) * F(blind_radius))


def process(xyz, ring, scan_period=0.1, blind_radius=2.5):
    """xyz (H, W, >=3) float32, ring (H, W) uint16 -> dict(cloud (m, 4), ranges (H, 2) int32, keep (H, W) bool)."""
    xyz = np.asarray(xyz, np.float32)
    ring = np.asarray(ring, np.uint16)
    H, W = ring.shape
    keep = keep_mask(xyz, blind_radius)
    curv = ring.astype(np.int32).astype(np.float32) + rel_times(W, scan_period)[None, :]
    cloud = np.concatenate([xyz[..., :3], curv[..., None]], -1).astype(np.float32)[keep]  # row-major: the rows concatenated
    size = np.cumsum(keep.sum(1))
    ranges = np.stack([np.concatenate([[0], size[:-1]]), np.where(size > 0, size - 1, 0)], 1).astype(np.int32)
    return dict(cloud=cloud, ranges=ranges, keep=keep)


def process_literal(xyz, ring, scan_period=0.1, blind_radius=2.5):
    """The reference's loops as they stand (:99-140)."""
    H, W = np.asarray(ring).shape
    period, blind = F(scan_period), F(blind_radius)
    scans = [[] for _ in range(H)]
    for row in range(H):
        for col in range(W):
            x, y, z = F(xyz[row][col][0]), F(xyz[row][col][1]), F(xyz[row][col][2])
            rel_time = F(float(period) * float(col) / W)
            curvature = F(F(int(ring[row][col])) + rel_time)
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                continue
            with np.errstate(all="ignore"):
                if F(F(x * x) + F(y * y)) + F(z * z) < blind * blind:
                    continue
            scans[row].append((x, y, z, curvature))
    cloud, ranges, size = [], [], 0
    for row in range(H):
        cloud += scans[row]
        first = size
        size += len(scans[row])
        ranges.append((first, size - 1 if size > 0 else 0))
    return dict(cloud=np.array(cloud, np.float32).reshape(-1, 4), ranges=np.array(ranges, np.int32).reshape(H, 2))


def start_state(history, scan_time_ns):
    """_imuStart = interpolateIMUStateFor(0) on the host: -> (angles (3,), trig (6,), velocity (3,))."""
    tsec, dt_prev, rows = history.arrays(scan_time_ns)
    zero = np.zeros(1, np.float32)
    i0, _ = R.walk_indices(tsec, zero)
    ang, trig, _, vel = R.states_for(tsec, dt_prev, rows, i0, zero)
    raw = i0[0] == 0 or tsec[i0[0]] > 0
    return ang[0], (trig[0] if raw else R.angle_cache(ang[0])), vel[0]


def imu_trans(history, scan_time_ns):
    t = np.zeros((4, 3), np.float32)
    if not len(history):
        return t
    ang, trig, vel = start_state(history, scan_time_ns)
    t[0] = ang[[1, 2, 0]]
    zero = (F(0), F(0), F(0))
    t[2] = R.rotate_yxz_neg(zero, tuple(trig))
    t[3] = R.rotate_yxz_neg(tuple(F(0) - v for v in vel), tuple(trig))
    return t


class Registration:
    """OrganisedScanRegistration with the one member that lives across sweeps: the IMU history."""

    def __init__(self, scan_period=0.1, blind_radius=2.5, imu_history_size=200):
        self.scan_period, self.blind_radius = scan_period, blind_radius
        self.history = R.ImuHistory(imu_history_size)

    def process(self, xyz, ring, scan_time_ns):
        out = process(xyz, ring, self.scan_period, self.blind_radius)
        out["imu_trans"] = imu_trans(self.history, scan_time_ns)
        return out


def image_from_scan(cloud, rings, steps, scan_period=0.1):
    """The organised image of a ``synth.make_scan(..., full=True)`` cloud: cell (ring, column) from the 4th channel (ring +
    column / steps * scan_period), cells without a return NaN.  -> (xyz (rings, steps, 3) float32, ring (rings, steps) uint16)."""
    w = cloud[:, 3].astype(np.float64)
    r = np.floor(w).astype(np.int64)
    col = np.rint((w - r) / scan_period * steps).astype(np.int64)
    ok = (col >= 0) & (col < steps)
    assert ok.all() and len(np.unique(r * steps + col)) == len(cloud)
    img = np.full((rings, steps, 3), np.nan, np.float32)
    img[r, col] = cloud[:, :3]
    return img, np.repeat(np.arange(rings, dtype=np.uint16)[:, None], steps, 1)


def as_point_xyzit(xyz, ring, fill=0):
    """The image as the reference's PointXYZIT records: (H, W) structured, 32 bytes a point, x / y / z at 0 and the ring at 26;
    every other byte holds ``fill``."""
    dt = np.dtype(dict(names=["x", "y", "z", "ring"], formats=[np.float32, np.float32, np.float32, np.uint16], offsets=[0, 4, 8, 26],
                       itemsize=32))
    H, W = np.asarray(ring).shape
    raw = np.full((H, W, 32), fill, np.uint8)
    out = raw.view(dt).reshape(H, W)
    out["x"], out["y"], out["z"], out["ring"] = xyz[..., 0], xyz[..., 1], xyz[..., 2], ring
    return out
