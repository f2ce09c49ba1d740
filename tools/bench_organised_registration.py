#!/usr/bin/env python3
"""The registration front end of an organised sensor per sweep, three ways, taken in turn in one process on the same sweeps:

  A  the composed path: OrganisedScanRegistration::process restated on the host (numpy, every buffer made once: validity,
     relTime per column, ring + relTime, the rows concatenated, the ranges), then lslam_extract_features_dev through the C ABI.
     Its two parts are clocked separately: "restate" is host arithmetic in numpy (the Python side's share of A), "extract" the
     library call (upload of the registered cloud, three launches, one wait)
  B  the yardstick: the multi-scan node (lslam_sreg_process, no IMU heard) on the same returns in arrival order
  C  the organised node (lslam_oreg_process) on the packed 16-byte cells

on seeded 16 x 1800 and 64 x 1800 sweeps (--shapes adds others, e.g. 128x2048).  B and C are called through the C ABI with
buffers made once, as A's library part is.  Every call ends in its own wait, so the host clock around it is the time per sweep.
Medians over --sweeps sweeps per variant, --repeats repeats of the whole measurement (the spread of the medians is the noise a
difference has to beat).  A and C must agree in every bit of the lists, the cloud and the ranges or the script exits non-zero.
Bytes over PCIe: counted from the shapes for A, reported by the nodes for B and C.  Prints a table and one JSON line."""
import argparse
import ctypes as C
import gc
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T0 = 1_700_000_000 * 10 ** 9
BLIND = 2.5


def sweeps_of(synth, rings, steps, n):
    """-> [(xyz (rings, steps, 3) with NaN where no return, ring (rings, steps) uint16, the returns in arrival order (m, 4))]."""
    world = synth.World(half_extent=175.0)
    out = []
    for k in range(n):
        gt = (0.0, 0.0, 0.3 + 0.01 * k, 3.0 + 0.4 * k, -2.0 + 0.15 * k, synth.SENSOR_HEIGHT)
        cloud = synth.make_scan(world, rings, steps, gt_pose=gt, seed=300 + k, full=True)[3]
        w = cloud[:, 3].astype(np.float64)
        r = np.floor(w).astype(np.int64)
        col = np.clip(np.rint((w - r) / 0.1 * steps).astype(np.int64), 0, steps - 1)
        xyz = np.full((rings, steps, 3), np.nan, np.float32)
        xyz[r, col] = cloud[:, :3]
        ring = np.repeat(np.arange(rings, dtype=np.uint16)[:, None], steps, 1)
        raw = np.ascontiguousarray(cloud[np.lexsort((r, -(cloud[:, 3] - r)))], np.float32)
        out.append((xyz, ring, raw))
    return out


class Restatement:
    """OrganisedScanRegistration::process in numpy with its buffers made once (tests/organised_registration_ref.py is the
    statement the tests hold the node to; this is the same arithmetic written for speed)."""

    def __init__(self, h, w, scan_period=0.1, blind=BLIND):
        self.h, self.w = h, w
        self.rel = (np.float64(np.float32(scan_period)) * np.arange(w, dtype=np.float64) / np.float64(w)).astype(np.float32)
        self.blind2 = np.float32(blind) * np.float32(blind)
        self.t = [np.zeros((h, w), np.float32) for _ in range(3)]
        self.keep = np.zeros((h, w), bool)
        self.fin = np.zeros((h, w), bool)
        self.full = np.zeros((h, w, 4), np.float32)
        self.cloud = np.zeros((h * w, 4), np.float32)
        self.ranges = np.zeros((h, 2), np.int32)
        self.n = 0

    def __call__(self, xyz, ring):
        a, b, c = self.t
        with np.errstate(all="ignore"):
            np.multiply(xyz[..., 0], xyz[..., 0], out=a)
            np.multiply(xyz[..., 1], xyz[..., 1], out=b)
            np.add(a, b, out=a)
            np.multiply(xyz[..., 2], xyz[..., 2], out=c)
            np.add(a, c, out=a)
            np.less(a, self.blind2, out=self.keep)
        np.logical_not(self.keep, out=self.keep)
        for d in range(3):
            np.isfinite(xyz[..., d], out=self.fin)
            np.logical_and(self.keep, self.fin, out=self.keep)
        self.full[..., :3] = xyz
        np.add(ring.astype(np.float32), self.rel[None, :], out=self.full[..., 3])
        flat = np.flatnonzero(self.keep.reshape(-1))
        self.n = len(flat)
        np.take(self.full.reshape(-1, 4), flat, axis=0, out=self.cloud[:self.n])
        size = np.cumsum(self.keep.sum(1))
        self.ranges[0, 0] = 0
        self.ranges[1:, 0] = size[:-1]
        self.ranges[:, 1] = np.where(size > 0, size - 1, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=["16x1800", "64x1800"])
    args = ap.parse_args()
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    capi = importlib.import_module("the-cooper-mapper_amd.capi")
    sr = pkg.scan_registration
    ctx = pkg.Context(0)
    lib = ctx.lib
    result = {}
    for shape in args.shapes:
        rings, steps = (int(v) for v in shape.split("x"))
        lo, hi = (-24.9, 2.0) if rings == 64 else (-15.0, 15.0)
        data = sweeps_of(synth, rings, steps, 8)
        cells = [sr.pack_organised(xyz, ring) for xyz, ring, _ in data]
        fs = sr.FeatureSet(ctx)
        node_b = pkg.MultiScanRegistration(ctx, lo, hi, rings)
        node_c = pkg.OrganisedScanRegistration(ctx, blind_radius=BLIND)
        st_b, st_c = capi.LslamSregStats(), capi.LslamOregStats()
        counts = (C.c_size_t * 4)()
        restate = Restatement(rings, steps)
        rr_p = restate.ranges.ctypes.data_as(capi.c_int32_p)
        clock = {"restate": 0.0}

        def check(rc):
            if rc < 0:
                raise pkg.LslamError(rc, lib.lslam_last_error().decode())

        def run_a(i):
            t = time.perf_counter()
            restate(data[i][0], data[i][1])
            clock["restate"] = time.perf_counter() - t
            if restate.n:
                check(lib.lslam_extract_features_dev(ctx.h, restate.cloud.ctypes.data_as(C.c_void_p), restate.n, 16, 12, rr_p, rings, None, fs.h, counts))

        def run_b(i):
            raw = data[i][2]
            check(lib.lslam_sreg_process(node_b.h, raw.ctypes.data_as(C.c_void_p), len(raw), 16, T0, fs.h, counts, None, C.byref(st_b)))

        def run_c(i):
            check(lib.lslam_oreg_process(node_c.h, cells[i].ctypes.data_as(C.c_void_p), rings, steps, 16, 12, T0, fs.h, counts, None, C.byref(st_c)))
        variants = {"A": run_a, "B": run_b, "C": run_c}
        # C is A in every bit: lists, cloud, ranges
        for i in range(len(data)):
            run_a(i)
            want = [fs.download(k) for k in sr.LISTS]
            run_c(i)
            node_c.height = rings  # (the call above went past the mirror, which remembers the rows for cloud())
            cloud, ranges = node_c.cloud()
            same = len(cloud) == restate.n and np.array_equal(cloud.view(np.uint32), restate.cloud[:restate.n].view(np.uint32)) and \
                np.array_equal(ranges, restate.ranges)
            for k, w in zip(sr.LISTS, want):
                got = fs.download(k)
                same = same and got.shape == w.shape and np.array_equal(got.view(np.uint32), w.view(np.uint32))
            if not same:
                print("FAIL: the organised node differs from the composed path on sweep %d of %s" % (i, shape))
                return 1
        n_cells = rings * steps
        for i in range(args.warmup):
            for f in variants.values():
                f(i % len(data))
        gc.collect(); gc.freeze(); gc.disable()
        med = {v: [] for v in variants}
        med_restate = []
        for _ in range(args.repeats):
            host = {v: [] for v in variants}
            part = []
            for i in range(args.sweeps):
                for v, f in variants.items():
                    t = time.perf_counter()
                    f(i % len(data))
                    host[v].append(time.perf_counter() - t)
                    if v == "A":
                        part.append(clock["restate"])
            for v in variants:
                med[v].append(float(np.median(host[v]) * 1e3))
            med_restate.append(float(np.median(part) * 1e3))
        gc.enable()
        gc.unfreeze()
        m = int(st_c.n_points)
        rows = {
            "A": dict(up=m * 16 + rings * 8, down=32, waits=1, launches="3 (after the host's loop)"),
            "B": dict(up=int(st_b.bytes_up), down=int(st_b.bytes_down), waits=1, launches="%d + grouping" % st_b.launches),
            "C": dict(up=int(st_c.bytes_up), down=int(st_c.bytes_down), waits=1, launches="%d" % st_c.launches),
        }
        print("%s (%d cells, %d kept; B: %d returns in, %d kept), medians of %d sweeps, %d repeats (min .. max of the medians)" %
              (shape, n_cells, m, len(data[-1][2]), int(st_b.n_points), args.sweeps, args.repeats))
        for v in variants:
            h = med[v]
            rows[v].update(host_ms=float(np.median(h)), host_ms_min=min(h), host_ms_max=max(h))
            extra = "   of which restate (numpy, host) %.3f ms" % float(np.median(med_restate)) if v == "A" else ""
            print("  %-2s host %.3f ms (%.3f .. %.3f)   up %8d B  down %8d B  waits %d  launches %s%s" %
                  (v, rows[v]["host_ms"], min(h), max(h), rows[v]["up"], rows[v]["down"], rows[v]["waits"], rows[v]["launches"], extra))
        rows["A"]["restate_ms"] = float(np.median(med_restate))
        spread_b = max(med["B"]) - min(med["B"])
        diff = rows["C"]["host_ms"] - rows["B"]["host_ms"]
        print("  C - B = %+.3f ms (spread of B's repeats %.3f ms, %.1f %% of B): %s;  A - C = %.3f ms" %
              (diff, spread_b, 100 * spread_b / rows["B"]["host_ms"], "C is at or below B" if diff <= spread_b else "C IS SLOWER THAN B",
               rows["A"]["host_ms"] - rows["C"]["host_ms"]))
        result[shape] = dict(cells=n_cells, kept=m, variants=rows, c_minus_b_ms=diff, b_spread_ms=spread_b)
        node_b.close(); node_c.close(); fs.close()
    print(json.dumps(dict(tool="bench_organised_registration", sweeps=args.sweeps, repeats=args.repeats, result=result)))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
