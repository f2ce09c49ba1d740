"""The x-subdivided cell table (csrc/lslam_grid.hpp, CellGrid::xsub, knn5_grid<.., FINE>) as a statement about point sets, checked
on the CPU by brute force, in the style of tests/test_grid_proof_property.py, whose numpy restatement of the cubic probe this
one extends with the kernel's sub-cell rule:

  x index of a point or a query  floor(fl(fl(v - org[0]) * inv_cx)), inv_cx = S / c; coarse x cell = that index div S
                                 (the kernel: floor((index + 0.5) * fl(1 / S)); position in the cell clamp(u * fl(1 / S) - cell))
  interior, wall, rg, y / z clip on coarse coordinates, as in the cubic probe
  x-extent of the nine runs      max(S (fxc - 1), floor(u - rbc S)) .. min(S (fxc + 1) + S - 1, floor(u + rbc S))   [sub-cells]

Claims, for S = 1 .. 4, bounds from the exact fifth distance up to the acceptance gate:
  * PROVEN => the five returned are the five nearest by the reference's fp32 distance, in order, with nanoflann's margin;
  * every map point the probe did not scan is farther than min(cl, rg): cl = rb - GRID_U_SLACK c keeps its claim;
  * the candidates for S are a subset of those for S = 1 (the cubic table) and hold every point within that radius;
  * unclipped, the candidate sets are equal -- a loop's first sweep sees what it saw.

The last two compare two TABLES, and hold exactly where the two agree on everybody's coarse cell.  For S = 2 and 4 they
always do: fl(S / c) = S fl(1 / c) (a power of two commutes with rounding), so the sub-cell coordinate is S times the
cubic one, bit for bit, and index div S is the cubic cell -- asserted below for every point and query.  For S = 3,
fl(3 / c) and 3 fl(1 / c) differ in the last place, and a point or a query within that rounding of a cell wall (the queries
here are PUT there) lies in the neighbouring coarse cell of the subdivided table: by the table's own definition, so nothing
the proof needs changes (the first two claims are checked for every query), but the set comparison leaves such points out and
skips such queries."""
import numpy as np

import test_grid_proof_property as gp

F = np.float32
FLT_MAX = gp.FLT_MAX


class XGrid(gp.Grid):
    def __init__(self, pts, S, c=gp.CELL):
        self.S = int(S)
        super().__init__(pts, c)
        self.inv_cx = self.inv_c if self.S == 1 else F(F(self.S) / self.c)
        self.inv_s = F(F(1.0) / F(self.S))
        self.nx = int(self.dims[0]) * self.S
        ux = self.ux(self.pts[:, 0])
        u = self.u(self.pts)
        fine = np.floor(ux).astype(int)
        # the coarse cell of a map point, by definition fine div S: never more than a rounding away from where the cubic table puts it
        assert np.abs(fine // self.S - np.floor(u[:, 0]).astype(int)).max() <= 1
        self.moved = set(np.nonzero(fine // self.S != np.floor(u[:, 0]).astype(int))[0].tolist())
        assert not self.moved or self.S == 3
        self.by_cell = {}
        for i, k in enumerate(zip(fine, np.floor(u[:, 1]).astype(int), np.floor(u[:, 2]).astype(int))):
            self.by_cell.setdefault(tuple(int(v) for v in k), []).append(i)

    def ux(self, x):
        return ((np.asarray(x, F) - self.org[0]).astype(F) * self.inv_cx).astype(F)

    def probe_x(self, q, bound=FLT_MAX):
        """-> (verdict, five, distances, candidates (set of map indices), radius every unscanned point is beyond [m])"""
        q = q.astype(F)
        S, sx = self.S, F(self.S)
        u = self.u(q)
        ux = F(self.ux(q[0]))
        n = self.dims
        interior = ux >= sx and ux < F(F(self.nx) - sx) and all(u[a] >= 1.0 and u[a] < F(n[a] - 1) for a in (1, 2))
        if not interior:
            return ("far" if np.isfinite(u).all() and np.isfinite(ux) else "unproven"), None, None, set(), 0.0
        fine = np.floor(ux)
        fxc = np.floor(F(F(fine + F(0.5)) * self.inv_s))
        assert int(fxc) == int(fine) // S        # the kernel's float form of `div`
        f0 = np.array([fxc, np.floor(u[1]), np.floor(u[2])], F)
        ex = min(max(F(F(ux * self.inv_s) - fxc), F(0.0)), F(1.0))
        e = np.array([ex, u[1] - f0[1], u[2] - f0[2]], F)
        wall = min(min(e[a], F(1.0) - e[a]) for a in range(3))
        rg = self.c * ((F(1.0) - gp.U_SLACK) + wall)
        rg2 = F((rg * rg) * (F(1.0) - (F(1.0e-5) + gp.NF_SLACK)))
        lo, hi = f0 - 1, f0 + 1
        xlo, xhi = F(sx * (fxc - 1)), F(sx * (fxc + 1) + (sx - 1))
        clip_lo2, beyond = FLT_MAX, float(rg)
        if bound < 1e30:
            rb = F(np.sqrt(F(bound)) * (F(1.0) + F(1.0e-5)) + gp.CLIP_MARGIN)
            rbc = F(rb * self.inv_c)
            rbx = F(rbc * sx)
            xlo, xhi = max(xlo, np.floor(F(ux - rbx))), min(xhi, np.floor(F(ux + rbx)))
            lo = np.maximum(lo, np.floor((np.array([0, u[1], u[2]], F) - rbc).astype(F)))
            hi = np.minimum(hi, np.floor((np.array([0, u[1], u[2]], F) + rbc).astype(F)))
            cl = F(rb - gp.U_SLACK * self.c)
            clip_lo2 = F((cl * cl) * (F(1.0) - F(1.0e-5)))
            beyond = min(beyond, float(cl))
        cand = []
        for jz in range(int(f0[2]) - 1, int(f0[2]) + 2):
            for jy in range(int(f0[1]) - 1, int(f0[1]) + 2):
                if not (lo[1] <= jy <= hi[1] and lo[2] <= jz <= hi[2]):
                    continue
                row = []
                for jx in range(int(xlo), int(xhi) + 1):
                    row += self.by_cell.get((jx, jy, jz), [])
                if len(row) > 64:   # GRID_ROW_MAX + 1: the lane sits the loop out, unproven whatever it would find
                    return "unproven", None, None, None, beyond
                cand += row
        cset = set(cand)
        cand = np.array(cand, int)
        d = gp.dist2(q, self.pts[cand]) if len(cand) else np.zeros(0, F)
        dk = gp.key_dist2(q, self.pts[cand]) if len(cand) else np.zeros(0, F)
        keys = (dk.view(np.uint32) & np.uint32(~((1 << gp.ID_BITS) - 1) & 0xFFFFFFFF)).astype(np.uint64) * 1024 + np.arange(len(cand), dtype=np.uint64)
        order = np.argsort(keys, kind="stable")[:6]
        surv, e6 = cand[order], d[order]
        if len(surv) < 5:
            return "unproven", None, None, cset, beyond
        t6 = FLT_MAX if len(surv) < 6 else F(F(np.uint32(keys[order[5]] // 1024).view(F)) * (F(1.0) - gp.KEY_SLACK))
        idx5, d5 = list(surv[:5]), list(e6[:5])
        lb = e6[5] if len(surv) == 6 else FLT_MAX
        if not all(e6[i] <= e6[i + 1] for i in range(len(e6) - 1)):
            o2 = np.argsort(e6[:5], kind="stable")
            idx5, d5 = [surv[i] for i in o2], [e6[i] for i in o2]
            if len(surv) == 6:
                lb = max(e6[5], d5[4])
                if e6[5] < d5[4]:
                    pos = int(np.searchsorted(np.array(d5, F), e6[5], side="right"))
                    d5 = d5[:pos] + [e6[5]] + d5[pos:4]
                    idx5 = idx5[:pos] + [surv[5]] + idx5[pos:4]
        if lb < 1e30:
            lb = F(lb * (F(1.0) - gp.NF_SLACK))
        lb6 = min(F(lb), t6, rg2, clip_lo2)
        distinct = all(d5[i] < d5[i + 1] for i in range(4))
        return ("proven" if distinct and d5[4] < lb6 else "unproven"), np.array(idx5), np.array(d5, F), cset, beyond


def lattice_map(rng, jitter_ulps):
    """~2 000 points on a 0.4 m lattice (a ground sheet and a wall); jittered by a few ulps, or exact (ties everywhere)."""
    g = np.arange(-8.0, 8.0, 0.4)
    gx, gy = np.meshgrid(g, g)
    hz = np.arange(0.4, 4.0, 0.4)
    wx, wz = np.meshgrid(g, hz)
    pts = np.concatenate([np.c_[gx.ravel(), gy.ravel(), np.zeros(gx.size)], np.c_[wx.ravel(), np.full(wx.size, 2.0), wz.ravel()]]).astype(F)
    if jitter_ulps:
        k = rng.integers(-jitter_ulps, jitter_ulps + 1, pts.shape)
        pts = np.where(pts != 0, (pts.view(np.int32) + k.astype(np.int32)).view(F), pts)   # (an exact 0.0 stays)
    return pts


def random_map(rng):
    """~2 000 points: a ground sheet and a wall near a 0.4 m voxel pitch with jitter, poles, clutter."""
    g = np.arange(-7.0, 7.0, 0.4)
    gx, gy = np.meshgrid(g, g)
    ground = np.c_[gx.ravel(), gy.ravel(), np.zeros(gx.size)] + rng.uniform(-0.12, 0.12, (gx.size, 3)) * [1, 1, 0.1]
    h = np.arange(0, 5, 0.4)
    wx, wz = np.meshgrid(g, h)
    wall = np.c_[wx.ravel(), np.full(wx.size, 3.1), wz.ravel()] + rng.uniform(-0.1, 0.1, (wx.size, 3)) * [1, 0.1, 1]
    poles = np.concatenate([np.c_[np.full(len(h), x), np.full(len(h), y), h] for x, y in rng.uniform(-6, 6, (12, 2))])
    return np.concatenate([ground, wall, poles, rng.uniform(-7, 7, (150, 3))]).astype(F)


def queries(rng, G1, pts, n):
    """Near map points; a third of them put on (and an ulp either side of) a sub-cell wall of S = 2, 3 or 4 -- among them the
    first and the last sub-cell of a coarse cell."""
    out = []
    for i in range(n):
        q = (pts[rng.integers(len(pts))] + rng.normal(0, rng.choice([0.02, 0.15, 0.4]), 3)).astype(F)
        if i % 3 == 0:
            S = int(rng.choice([2, 3, 4]))
            cx = np.floor(G1.u(q)[0])
            k = int(rng.choice([0, 1, S - 1, S]))   # walls of the first and the last sub-cell of the coarse cell
            x = F(G1.org[0] + F(F(cx + F(k) / F(S)) * G1.c))
            x = np.nextafter(x, F([-np.inf, 0, np.inf][int(rng.integers(3))] + x), dtype=F) if rng.integers(2) else x
            q[0] = x
        out.append(q)
    return out


def check_map(pts, rng, n_q, counts):
    grids = {S: XGrid(pts, S) for S in (1, 2, 3, 4)}
    G1 = gp.Grid(pts)
    p64 = pts.astype(np.float64)
    for q in queries(rng, grids[1], pts, n_q):
        d_all = gp.dist2(q, pts)
        order = np.argsort(d_all, kind="stable")
        truth, d_true, d6 = order[:5], d_all[order[:5]], d_all[order[5]]
        true_dist = np.sqrt(((p64 - q.astype(np.float64)) ** 2).sum(1))
        # bounds: none; the exact fifth distance; between it and the gate; the gate
        gate = F(5.0) * (F(1.0) + F(1e-5))
        mid = F(min(float(gate), float(d_true[4]) * float(rng.choice([1.02, 1.5, 4.0]))))
        for bound in (FLT_MAX, min(gate, F(d_true[4])), mid, gate):
            if bound < 1e30 and not bound >= d_true[4]:
                continue   # (beyond the gate: not a bound of the fifth distance, nothing is looked up there)
            ref = None
            for S in (1, 2, 3, 4):
                verdict, idx5, d5, cset, beyond = grids[S].probe_x(q, bound)
                if S == 1:   # the restated probe with S = 1 IS the cubic probe of tests/test_grid_proof_property.py
                    v0, i0, e0 = G1.probe(q, bound)
                    assert v0 == verdict and (i0 is None or (np.array_equal(i0, idx5) and np.array_equal(e0, d5)))
                    ref = cset
                if verdict == "far":
                    assert d_true[0] > 5.0
                    continue
                if verdict == "proven":
                    counts["proven", S] = counts.get(("proven", S), 0) + 1
                    assert np.array_equal(idx5, truth), (S, q, idx5, truth)
                    assert np.array_equal(d5.view(np.uint32), d_true.view(np.uint32))
                    assert F(d6 * (F(1.0) - gp.NF_SLACK)) >= d5[4] or d6 * (1.0 - 1.1e-5) > d5[4]
                if cset is None:   # a row longer than 64 candidates: unproven, nothing else claimed
                    counts["overflow"] = counts.get("overflow", 0) + 1
                    continue
                unscanned = np.ones(len(pts), bool)
                unscanned[list(cset)] = False
                assert not unscanned.any() or true_dist[unscanned].min() > beyond, (S, q, bound, true_dist[unscanned].min(), beyond)
                q_moved = int(np.floor(grids[S].ux(q[0]))) // S != int(np.floor(grids[1].u(q)[0]))
                assert not q_moved or S == 3
                if ref is not None and not q_moved:
                    moved = grids[S].moved
                    assert cset - moved <= ref, (S, q, bound)
                    if bound > 1e30:
                        assert cset - moved == ref - moved, (S, q)
                    elif S > 1:
                        counts["fewer"] = counts.get("fewer", 0) + (len(cset) < len(ref))
                        counts["clipped"] = counts.get("clipped", 0) + 1


def test_subdivided_probe_random_map():
    rng = np.random.default_rng(16)
    counts = {}
    check_map(random_map(rng), rng, 700, counts)
    assert all(counts.get(("proven", S), 0) > 300 for S in (1, 2, 3, 4)), counts   # (not vacuous)
    assert counts["fewer"] > 0.1 * counts["clipped"], counts   # the finer clip does cut candidates


def test_subdivided_probe_lattice_exact():
    rng = np.random.default_rng(17)
    counts = {}
    check_map(lattice_map(rng, 0), rng, 650, counts)
    assert all(counts.get(("proven", S), 0) > 100 for S in (1, 2, 3, 4)), counts


def test_subdivided_probe_lattice_jittered():
    rng = np.random.default_rng(18)
    counts = {}
    check_map(lattice_map(rng, 3), rng, 650, counts)
    assert all(counts.get(("proven", S), 0) > 100 for S in (1, 2, 3, 4)), counts


def test_row_longer_than_64_is_unproven_not_wrong():
    rng = np.random.default_rng(19)
    pts = np.concatenate([random_map(rng), (np.array([0.1, 0.1, 1.0]) + rng.uniform(0, 0.05, (80, 3))).astype(F)]).astype(F)
    for S in (1, 2, 3, 4):
        G = XGrid(pts, S)
        verdict, _, _, cset, _ = G.probe_x(np.array([0.12, 0.12, 1.02], F))
        assert verdict == "unproven" and cset is None
