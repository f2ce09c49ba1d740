"""Restatement of the paged cube window (util/DynamicFeatureMap.h: setupPCDFileName :129-161, update :504-677,
getSurroundFeature :681-692, computeActiveAera / InVerticalFov :748-804, scanMatchScan :807-1017), composed only from
tests/oracle_lib.py.  The window is a set of GLOBAL cube indices; a cube that enters is read from its PCD and goes through
``oracle.voxel_grid`` with its type's leaf; the match is ``oracle.scanmatch_cubes`` on the resident cubes' filtered clouds
concatenated in ascending window-cell order, with ``origin = half - sensorGloIdx`` and ``dims = window``.  That call rests on two
preconditions, asserted here on the CPU: every filtered point re-bins into its file's cube, and every query stays inside the
window (the reference indexes out of range there; the device skips such a query).  tests/test_gpu_paged_localization.py holds
the device node against this."""
import os

import numpy as np

import localization_ref as lr

F = np.float32


round_half_away = lr.round_half_away  # std::round of a float32 without a second rounding; not finite -> lr.NO_CUBE


def glo_idx(p, cube_size):
    """Glo2GloIdx: (int) round(x / cube_size) per axis, a float quotient."""
    with np.errstate(invalid="ignore", over="ignore"):
        return round_half_away(np.asarray(p, F)[..., :3] / F(cube_size))


def parse_index(path):
    """setupPCDFileName: lines ``count type i j k size``; type 0 is corner, anything else surf; a later line for the same
    (type, cube) replaces the earlier one.  -> [corner, surf] dicts (i, j, k) -> count.  Every line is taken once."""
    index = [{}, {}]
    for line in open(path):
        w = line.split()
        if len(w) < 6:
            continue
        count, t, i, j, k = (int(v) for v in w[:5])
        index[0 if t == 0 else 1][(i, j, k)] = count
    return index


def write_pcd(path, pts):
    pts = np.ascontiguousarray(pts, F).reshape(-1, 4)
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
                 "COUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (len(pts), len(pts))).encode())
        f.write(pts.tobytes())


def write_paged_map(directory, map_corner, map_surf, cube_size, index_name="index2.txt", offset=(0, 0, 0)):
    """The map binned by round(p / cube_size) into one PCD per (type, cube), input order kept inside a cube, with the index
    beside them (cube indices + offset).  -> [corner, surf] dicts (i, j, k) -> count."""
    os.makedirs(directory, exist_ok=True)
    index = [{}, {}]
    lines = []
    count = 0
    keys = {}
    for t, cloud in enumerate((map_corner, map_surf)):
        cloud = np.ascontiguousarray(cloud, F)[:, :4]
        g = glo_idx(cloud, cube_size)
        keys[t] = (g, np.unique(g, axis=0))
    for key in sorted(set(map(tuple, keys[0][1])) | set(map(tuple, keys[1][1]))):
        for t, cloud in enumerate((map_corner, map_surf)):
            g = keys[t][0]
            sel = np.all(g == np.asarray(key), axis=1)
            if not sel.any():
                continue
            pts = np.ascontiguousarray(cloud, F)[sel, :4]
            write_pcd(os.path.join(directory, "%d.pcd" % count), pts)
            index[t][tuple(int(v) for v in key)] = count
            lines.append("%d %d %d %d %d %d\n" % (count, t, key[0] + offset[0], key[1] + offset[1], key[2] + offset[2], len(pts)))
            count += 1
    with open(os.path.join(directory, index_name), "w") as f:
        f.writelines(lines)
    return index


def active_area(index, pos, cube_size, valid):
    """computeActiveAera + InVerticalFov, transcribed: ws = ceil(valid / cube); loops i, j, k over [-ws, ws]; an offset is
    skipped unless a corner or surf entry is listed there; the centre is taken; any other offset is taken iff the smallest of its
    eight corner distances from the sensor's fractional position is <= valid (doubles, as written; the fractional position is a
    float).  -> list of global indices in loop order."""
    pos = np.asarray(pos, F)
    cs, valid = F(cube_size), F(valid)
    c = glo_idx(pos, cs)
    real = (pos[:3] / cs - c.astype(F)).astype(F).astype(np.float64)
    ws = int(np.ceil(valid / cs))
    d = (-0.5, 0.5)
    out = []
    for i in range(-ws, ws + 1):
        for j in range(-ws, ws + 1):
            for k in range(-ws, ws + 1):
                g = (int(c[0]) + i, int(c[1]) + j, int(c[2]) + k)
                if g not in index[0] and g not in index[1]:
                    continue
                take = i == 0 and j == 0 and k == 0
                if not take:
                    min_dis = -1.0
                    for dx in d:
                        for dy in d:
                            for dz in d:
                                x, y, z = i + dx - real[0], j + dy - real[1], k + dz - real[2]
                                dis = np.sqrt((x * float(cs)) ** 2 + (y * float(cs)) ** 2 + (z * float(cs)) ** 2)
                                min_dis = dis if min_dis == -1.0 else min(min_dis, dis)
                    take = not (min_dis > float(valid))
                if take:
                    out.append(g)
    return out


class RefPagedMap:
    def __init__(self, oracle, directory, dims, cube_size=50.0, valid=100.0, leaf_corner=0.2, leaf_surf=0.4):
        assert all(d % 2 == 1 for d in dims), "an even window dimension has no centre cube"
        self.o = oracle
        self.dir = str(directory)
        self.dims = tuple(int(d) for d in dims)
        self.half = tuple(d // 2 for d in self.dims)
        self.cube_size, self.valid = float(cube_size), float(valid)
        assert int(np.ceil(F(valid) / F(cube_size))) <= min(self.dims) // 2
        self.leaf = (float(leaf_corner), float(leaf_surf))
        self.index = parse_index(os.path.join(self.dir, "index2.txt"))
        self.centre = None
        self.cubes = [{}, {}]     # per type: global index -> filtered cloud (an unreadable file: an empty cloud)
        self.active = []
        self.files_read = 0       # by the last update
        self.files_missing = 0
        self.entered = [[], []]   # listed cubes the last update brought in
        self.steps = 0

    def in_window(self, g, c=None):
        c = self.centre if c is None else c
        return all(abs(int(g[d]) - int(c[d])) <= self.half[d] for d in range(3))

    def window_cells(self):
        """Global indices of the window in ascending cell order (i fastest)."""
        W, H, D = self.dims
        for k in range(D):
            for j in range(H):
                for i in range(W):
                    yield (self.centre[0] + i - self.half[0], self.centre[1] + j - self.half[1], self.centre[2] + k - self.half[2])

    def _load(self, t, g):
        path = os.path.join(self.dir, "%d.pcd" % self.index[t][g])
        if not os.path.exists(path):
            self.files_missing += 1
            return np.zeros((0, 4), F)
        self.files_read += 1
        pts = lr.read_pcd_xyzi(path)
        out = self.o.voxel_grid(pts, self.leaf[t]) if len(pts) else pts
        # precondition of the oracle call: a filtered point belongs to the cube its file was cut for
        assert np.all(glo_idx(out, self.cube_size) == np.asarray(g)), ("a filtered point left its cube", t, g)
        return out

    def update(self, pos):
        c = tuple(int(v) for v in glo_idx(np.asarray(pos, F), self.cube_size))
        self.files_read = self.files_missing = 0
        self.entered = [[], []]
        if self.centre is None or c != self.centre:
            old = self.centre
            self.centre = c
            for t in range(2):
                self.cubes[t] = {g: v for g, v in self.cubes[t].items() if self.in_window(g)}
                for g in self.window_cells():
                    if g in self.index[t] and g not in self.cubes[t]:
                        assert old is None or not self.in_window(g, old)
                        self.cubes[t][g] = self._load(t, g)
                        self.entered[t].append(g)
            self.steps += 1
        self.active = active_area(self.index, pos, self.cube_size, self.valid)

    def surround(self):
        """getSurroundFeature: the active cubes' filtered clouds in active-area order."""
        out = []
        for t in range(2):
            parts = [self.cubes[t][g] for g in self.active if g in self.cubes[t]]
            out.append(np.concatenate(parts, 0).astype(F) if parts else np.zeros((0, 4), F))
        return out

    def window_map(self):
        out = []
        for t in range(2):
            parts = [self.cubes[t][g] for g in self.window_cells() if g in self.cubes[t]]
            out.append(np.concatenate(parts, 0).astype(F) if parts else np.zeros((0, 4), F))
        return out

    def origin(self):
        return tuple(self.half[d] - self.centre[d] for d in range(3))

    def queries_in_window(self, cloud, pose):
        R, t = self.o.pose_to_Rt(np.asarray(pose, F))
        q = (np.asarray(cloud, F)[:, :3] @ R.T + t).astype(F)
        g = glo_idx(q, self.cube_size)
        return bool(np.all(np.abs(g - np.asarray(self.centre)) <= np.asarray(self.half)))

    def match(self, corner, surf, pose):
        """scanMatchScan on filtered scan clouds from a Twist, after update at its translation -> (ok, pose, stats)."""
        pose = np.asarray(pose, F)
        self.update(pose[3:6])
        mc, ms = self.window_map()
        assert self.queries_in_window(corner, pose) and self.queries_in_window(surf, pose), "a query leaves the window at the prior"
        ok, p, st = self.o.scanmatch_cubes(mc, ms, corner, surf, pose, self.cube_size, self.origin(), self.dims)
        assert self.queries_in_window(corner, p) and self.queries_in_window(surf, p), "a query leaves the window at the result"
        return ok, p, st


class RefPagedLocalization(lr.RefLocalization):
    """LaserLocalization::process with the dynamic branches: update(translation of the merged prior) before the match."""

    def __init__(self, oracle, paged, filter_corner=1.0, filter_surf=1.0):
        super().__init__(oracle, paged.dims, paged.cube_size, (0, 0, 0), filter_corner, filter_surf)
        self.paged = paged

    def match(self, corner, surf, pose):
        c, s = self.prepare_frame(corner, surf)
        return self.paged.match(c, s, pose)


# ---- the test scene: localization_ref's world and sweeps, 10 m cubes, a 9 x 9 x 5 window, every sweep cut to 30 m ----
CUBE = 10.0
WINDOW = (9, 9, 5)
VALID = 20.0
LEAVES = (1.0, 1.0)
RANGE_CUT = 30.0
STATIC_DIMS = (21, 21, 11)
STATIC_ORIGIN = (10, 10, 5)


def make_scene(synth, n_sweeps=4):
    scene = lr.make_scene(synth, n_sweeps=n_sweeps)
    cut = []
    for c, s in scene["sweeps"]:
        c, s = np.ascontiguousarray(c, F), np.ascontiguousarray(s, F)
        cut.append((c[np.linalg.norm(c[:, :3], axis=1) <= RANGE_CUT], s[np.linalg.norm(s[:, :3], axis=1) <= RANGE_CUT]))
    scene["sweeps"] = cut
    return scene
