"""Restatement of the localisation node (odometry/LaserLocalization.cpp:140-188 over LaserMatcher.cpp:289-340 and
util/FeatureMap.h:415-462,490-691), composed only from tests/oracle_lib.py: the map loaded with a per-cube VoxelGrid,
transformMerge, the two scan filters, ``oracle.scanmatch_cubes``, the reset-after-match rule of transformUpdate and the
velocity rule.  It is what tests/test_gpu_localization.py holds the device node against."""
import os

import numpy as np

DROPPED, HAS_VELOCITY, POSE_RESET, VELOCITY_ZEROED = 1, 2, 4, 8  # include/lslam_c.h LSLAM_LOC_*

F = np.float32


def transform_associate(Lold, Lnew, Wold):
    """transformAssociate (util/transform_utils.h:502-507): Wnew = Wold * Lold^-1 * Lnew for rigid float32 4x4 matrices, with
    the operation order of lslam_transform_associate (a row times a column accumulated left to right)."""
    Lold, Lnew, Wold = (np.asarray(a, F).reshape(4, 4) for a in (Lold, Lnew, Wold))

    def mul(A, B):
        C = np.zeros((4, 4), F)
        for r in range(3):
            for c in range(3):
                C[r, c] = F(F(A[r, 0] * B[0, c]) + F(A[r, 1] * B[1, c])) + F(A[r, 2] * B[2, c])
            C[r, 3] = F(F(F(A[r, 0] * B[0, 3]) + F(A[r, 1] * B[1, 3])) + F(A[r, 2] * B[2, 3])) + A[r, 3]
        C[3, 3] = 1
        return C
    Linv = np.zeros((4, 4), F)
    for r in range(3):
        for c in range(3):
            Linv[r, c] = Lold[c, r]
        Linv[r, 3] = -(F(F(Lold[0, r] * Lold[0, 3]) + F(Lold[1, r] * Lold[1, 3])) + F(Lold[2, r] * Lold[2, 3]))
    Linv[3, 3] = 1
    return mul(mul(Wold, Linv), Lnew)


NO_CUBE = -(2 ** 31)  # what the reference's (int) cast makes of a value that is not a number or does not fit: no valid index


def round_half_away(q):
    """std::round of float32 values -> int64.  The half is added in float64, where q + 0.5 is exact for every float32 q below
    2^24 (a float32 sum rounds the predecessor of 0.5 up to 1.0: one float per cube wall went to the wrong cube).  A value that
    is not finite, or beyond the int range, gives NO_CUBE."""
    q = np.asarray(q, F).astype(np.float64)
    fits = np.isfinite(q) & (np.abs(q) < 2.0 ** 31 - 1.0)
    r = np.trunc(np.where(fits, q, 0.0) + np.copysign(0.5, q))
    return np.where(fits, r, float(NO_CUBE)).astype(np.int64)


def cube_index(p, cube_size, origin):
    """worldToCube (FeatureMap.h:475-487): (int)(std::round(p / size) + origin), the quotient a float32, the rounding half away
    from zero.  A coordinate that is not finite (or absurdly large) gives NO_CUBE on its axis: isIndexValid fails."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = round_half_away(np.asarray(p, F)[..., :3] / F(cube_size))
    return np.where(r == NO_CUBE, NO_CUBE, r + np.asarray(origin, np.int64))


def read_pcd_xyzi(path):
    """A binary PCD with the fields x y z intensity, 16 bytes per point (what saveCloudToFiles writes)."""
    raw = open(path, "rb").read()
    head, _, body = raw.partition(b"DATA binary\n")
    n = [int(l.split()[1]) for l in head.decode().splitlines() if l.startswith("POINTS")][0]
    assert b"FIELDS x y z intensity" in head
    return np.frombuffer(body, F, n * 4).reshape(n, 4).copy()


class RefLocalization:
    def __init__(self, oracle, dims, cube_size=50.0, origin=None, filter_corner=1.0, filter_surf=1.0,
                 map_filter_corner=1.0, map_filter_surf=1.0):
        self.o = oracle
        self.dims = tuple(int(v) for v in dims)
        self.cube_size = float(cube_size)
        self.origin = tuple(int(round((d - 1) / 2.0)) for d in self.dims) if origin is None else tuple(origin)
        self.scan_leaf = (float(filter_corner), float(filter_surf))
        self.map_leaf = (float(map_filter_corner), float(map_filter_surf))
        self.map = [np.zeros((0, 4), F), np.zeros((0, 4), F)]
        self.cubes = [{}, {}]  # per type: cube index -> its cloud
        self.initialized = False
        self.reset_pending = False
        self.reset_pose = np.eye(4, dtype=F)
        self.mapped_last = np.eye(4, dtype=F)
        self.odom_last = np.eye(4, dtype=F)
        self.pose_last = np.eye(4, dtype=F)
        self.stamp_last = 0
        self.velocity = None
        self.last = None  # (ok, stats) of the last match

    # ---- the map ----------------------------------------------------------------------------------------------------------
    def _to_index(self, ijk):
        return ijk[0] + ijk[1] * self.dims[0] + ijk[2] * self.dims[0] * self.dims[1]

    def _commit(self):
        for t in range(2):
            keys = sorted(self.cubes[t])
            self.map[t] = (np.concatenate([self.cubes[t][k] for k in keys], 0) if keys else np.zeros((0, 4), F)).astype(F)

    def set_map(self, corner, surf, filter=False):
        """Points pushed into their cubes in input order (pushCornerPoint / pushSurfPoint); filter: every cube through its
        type's VoxelGrid as loadCloudFromFiles does."""
        for t, cloud in enumerate((corner, surf)):
            cloud = np.ascontiguousarray(cloud, F)[:, :4]
            self.cubes[t] = {}
            if len(cloud) == 0:
                continue
            ijk = cube_index(cloud, self.cube_size, self.origin)
            ok = np.all((ijk >= 0) & (ijk < np.asarray(self.dims)), axis=1)
            idx = ijk[:, 0] + ijk[:, 1] * self.dims[0] + ijk[:, 2] * self.dims[0] * self.dims[1]
            for c in np.unique(idx[ok]):
                pts = cloud[ok & (idx == c)]
                self.cubes[t][int(c)] = self.o.voxel_grid(pts, self.map_leaf[t]) if filter else pts
        self._commit()

    def load_map(self, directory, filter=True):
        """loadCloudFromFiles (FeatureMap.h:415-462) into an empty map: lines "count type i j k size"; a later entry for a cube
        replaces the earlier one, a missing PCD is skipped, each cube goes through its type's VoxelGrid."""
        self.cubes = [{}, {}]
        for line in open(os.path.join(directory, "index.txt")):
            w = line.split()
            if len(w) < 6:
                continue
            count, t, i, j, k = (int(v) for v in w[:5])
            if t not in (0, 1) or not all(0 <= v < d for v, d in zip((i, j, k), self.dims)):
                continue
            path = os.path.join(directory, "%d.pcd" % count)
            if not os.path.exists(path):
                continue
            pts = read_pcd_xyzi(path)
            self.cubes[t][self._to_index((i, j, k))] = self.o.voxel_grid(pts, self.map_leaf[t]) if filter and len(pts) else pts
        self._commit()

    # ---- the sweep --------------------------------------------------------------------------------------------------------
    def handle_initial_pose(self, T):
        self.reset_pose = np.asarray(T, F).reshape(4, 4).copy()
        self.reset_pending = True
        self.initialized = True

    def prepare_frame(self, corner, surf):
        c = np.ascontiguousarray(corner, F)[:, :4]
        s = np.ascontiguousarray(surf, F)[:, :4]
        return (self.o.voxel_grid(c, self.scan_leaf[0]) if len(c) else c, self.o.voxel_grid(s, self.scan_leaf[1]) if len(s) else s)

    def match(self, corner, surf, pose):
        """prepareFeatureFrame + optimizeTransform -> (ok, pose, stats)."""
        c, s = self.prepare_frame(corner, surf)
        return self.o.scanmatch_cubes(self.map[0], self.map[1], c, s, pose, self.cube_size, self.origin, self.dims)

    def isometry_to_pose(self, T):
        T = np.asarray(T, F).reshape(4, 4)
        return self.o.Rt_to_pose(np.ascontiguousarray(T[:3, :3]), np.ascontiguousarray(T[:3, 3]))

    def pose_to_isometry(self, pose):
        R, t = self.o.pose_to_Rt(np.asarray(pose, F))
        T = np.eye(4, dtype=F)
        T[:3, :3], T[:3, 3] = R, t
        return T

    def process(self, corner, surf, odom, stamp_ns):
        """LaserLocalization::process -> (T or None when dropped, flags)."""
        if not self.initialized:
            return None, DROPPED
        odom = np.asarray(odom, F).reshape(4, 4)
        Wnew = transform_associate(self.odom_last, odom, self.mapped_last)            # transformMerge
        ok, pose, st = self.match(corner, surf, self.isometry_to_pose(Wnew))           # prepareFeatureFrame, optimizeTransform
        self.last = (ok, st)
        T = self.pose_to_isometry(pose)
        flags = 0
        if self.reset_pending:                                                         # transformUpdate: AFTER the match
            T = self.reset_pose.copy()
            self.reset_pending = False
            flags |= POSE_RESET
        self.mapped_last = T.copy()
        self.odom_last = odom.copy()
        self.velocity = None
        if self.stamp_last != 0:
            dt = F(float(stamp_ns - self.stamp_last) * 1e-9)
            v = ((T[:3, 3] - self.pose_last[:3, 3]) / dt).astype(F)
            if F(np.sqrt(F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2])))) > 30:
                v = np.zeros(3, F)
                flags |= VELOCITY_ZEROED
            self.velocity = v
            flags |= HAS_VELOCITY
        self.pose_last = T.copy()
        self.stamp_last = int(stamp_ns)
        return T.copy(), flags


# ---- the test scene (ISSUE: synth.World(half_extent=60, wall_half=55), make_map(world, 0.2, 0.4, seed=77), four 16 x 900 sweeps) ----
DIMS = (121, 121, 11)
ORIGIN = (60, 60, 5)
CUBE = 50.0


def scene_pose(k):
    return (0.01, -0.015, 0.3 + 0.05 * k, 3.0 + 4.0 * k, -2.0 + 1.5 * k, 1.8)


def make_scene(synth, n_sweeps=4, extra_poses=()):
    world = synth.World(half_extent=60, wall_half=55)
    map_c, map_s = synth.make_map(world, 0.2, 0.4, seed=77)
    poses = [scene_pose(k) for k in range(n_sweeps)] + [tuple(p) for p in extra_poses]
    sweeps = []
    for k, gt in enumerate(poses):
        c, s, _ = synth.make_scan(world, 16, 900, gt_pose=gt, seed=1234 + k)
        sweeps.append((c, s))
    start = synth.perturb_pose(poses[0], dt=0.2, dr_deg=1.0)
    return dict(world=world, map_corner=map_c, map_surf=map_s, poses=poses, sweeps=sweeps, start=start)


def run_trajectory(node, scene, pose_to_isometry, stamp0=1_000_000_000, step_ns=200_000_000):
    """Drive a node (the restatement or the device mirror: handle_initial_pose / process) over the scene: the odometry input is
    the ground-truth pose of every sweep, the initial pose the perturbed start.  -> list of (T, velocity or None, flags)."""
    node.handle_initial_pose(pose_to_isometry(scene["start"]))
    out = []
    for k, (c, s) in enumerate(scene["sweeps"]):
        odom = pose_to_isometry(np.asarray(scene["poses"][k], F))
        r = node.process(c, s, odom, stamp0 + k * step_ns)
        if isinstance(r, tuple):
            T, flags = r
        else:
            T, flags = r, node.last_flags
        out.append((None if T is None else np.asarray(T, F).copy(), None if node.velocity is None else np.asarray(node.velocity, F).copy(), flags))
    return out
