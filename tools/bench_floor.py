#!/usr/bin/env python3
"""Cost of floor detection over a keyframe store: CLOUDS surface clouds of synth.make_scan(rings=16, azimuth_steps=1800), timed
with HIP events on the library's own stream (lslam_stream).  Two figures, each the median of REPS after 20 warm-up calls:
  detect  one lslam_floor_detect_keyframes call over all the clouds with the default parameters (512 hypotheses, one refit):
          every kernel of every stage, the small downloads and the host's fits -- the call as a caller sees it
  score   the scoring kernel alone (lslam_debug_floor_score: 10 launches per sample, the time per launch), the H x K point-plane
          tests of all the clouds in one launch
and beside them the scoring kernel's lower bound by VALU issue, from its disassembled inner loop: one iteration tests 4
hypotheses against the lane's 4 points with LOOP_VALU = 126 vector instructions (48 v_mul_f32, 48 v_add_f32, 16 v_cmp_le_f32 --
7 per test -- and 14 that keep each hypothesis's count in its lane), i.e. 7.875 per test; one wavefront instruction covers 64
lanes and occupies a SIMD for 4 cycles at the device's maximum clock (2400 MHz), over 4 SIMDs x the compute units.  The
arithmetic alone (7 per test) is printed beside it.  Prints one JSON line."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "100"))
CLOUDS = int(os.environ.get("CLOUDS", "16"))
LOOP_VALU, LOOP_TESTS = 126, 16   # the inner loop's vector instructions and lane-tests per iteration (disassembly, profiles/)
ARITHMETIC_VALU_PER_TEST = 7
SCORE_LAUNCHES = 10


def main():
    import torch
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ctx = pkg.Context(0)
    store = pkg.KeyframeStore(ctx)
    world = synth.World(half_extent=60.0, wall_half=55.0)
    ids, n_points = [], 0
    for k in range(CLOUDS):
        gt = (0.0, 0.0, 0.3 + 0.05 * k, 3.0 + 0.5 * k, -2.0 + 0.2 * k, synth.SENSOR_HEIGHT)
        corner, surf, _ = synth.make_scan(world, 16, 1800, gt_pose=gt, seed=500 + k)
        ids.append(store.add(corner, surf))
        n_points += len(surf)
    stream = C.c_void_p(ctx.lib.lslam_stream(ctx.h))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    params = pkg.floor.floor_params()
    res = store.floor_detect(ids, params)
    cand = sum(r["n_candidates"] for r in res)

    def timed(call, per=1):
        ms = []
        for _ in range(REPS + 20):
            assert hip.hipEventRecord(ev[0], stream) == 0
            call()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
            ms.append(t.value / per)
        ms = ms[20:]
        return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "p90_us": 1e3 * sorted(ms)[int(0.9 * len(ms))]}

    before = store.info()
    out = {"clouds": CLOUDS, "surface_points": n_points, "candidates": cand, "hypotheses": int(params.n_hypotheses), "reps": REPS,
           "status_ok": sum(r["status"] == 0 for r in res)}
    out["detect"] = timed(lambda: store.floor_detect(ids, params))
    out["score"] = timed(lambda: store._check(ctx.lib.lslam_debug_floor_score(store.h, SCORE_LAUNCHES)), per=SCORE_LAUNCHES)
    after = store.info()
    out["cloud_bytes_moved"] = (after["cloud_bytes_uploaded"] - before["cloud_bytes_uploaded"]) + (after["cloud_bytes_downloaded"] - before["cloud_bytes_downloaded"])
    prop = torch.cuda.get_device_properties(0)
    cus, mhz = prop.multi_processor_count, 2400.0  # the device's MAXIMUM clock: a bound whatever clock the chip holds under load
    tests = float(cand) * float(params.n_hypotheses)
    bound = lambda per_test: tests * per_test / 64.0 * 4.0 / (4.0 * cus) / mhz
    out["valu_bound"] = {"valu_per_test": LOOP_VALU / float(LOOP_TESTS), "compute_units": cus, "clock_mhz": mhz,
                         "us": bound(LOOP_VALU / float(LOOP_TESTS)), "arithmetic_only_valu_per_test": ARITHMETIC_VALU_PER_TEST,
                         "arithmetic_only_us": bound(ARITHMETIC_VALU_PER_TEST)}
    out["score"]["over_valu_bound"] = out["score"]["median_us"] / out["valu_bound"]["us"]
    out["score"]["over_arithmetic_only_bound"] = out["score"]["median_us"] / out["valu_bound"]["arithmetic_only_us"]
    for e in ev:
        hip.hipEventDestroy(e)
    store.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
