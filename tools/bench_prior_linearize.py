#!/usr/bin/env python3
"""What a unary constraint costs: one linearisation of the 5 000-keyframe / 25 000-edge bench graph (synth.make_pose_graph)
with no priors and with one XYZ prior per keyframe, timed with HIP events on the library's own stream (lslam_pg_stream): median
of REPS launches of lslam_pg_linearize without read-back -- the edge kernel, (the prior kernel,) the two assemble kernels and
the chi2 sum.  The trial chi2 of an LM iteration has no entry point of its own; it is timed inside one LM iteration
(lslam_pg_optimize(1) from the same start, lslam_pg_stats.gpu_ms_total: linearisation, damped solve, update, trial chi2),
median of LM_REPS fresh graphs.  The "no_priors" figures are the ones to compare with the parent commit's
tools/bench_robust_linearize.py "plain" on the same machine: that path launches nothing new.  Prints one JSON line."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "200"))
LM_REPS = int(os.environ.get("LM_REPS", "5"))


def main():
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    g = synth.make_pose_graph()
    n = len(g["init"])
    rng = np.random.default_rng(0)
    sigma = np.array([0.3, 0.3, 0.6])
    meas = np.zeros((n, 7))
    meas[:, 6] = 1.0
    meas[:, :3] = g["gt"][:, :3] + rng.normal(size=(n, 3)) * sigma  # a fix per keyframe: ground truth + (0.3, 0.3, 0.6) m
    info = np.zeros((n, 6, 6))
    info[:, :3, :3] = np.diag(1.0 / sigma ** 2)
    priors = dict(vertex=np.arange(n, dtype=np.int32), type=np.zeros(n, np.int32), meas=meas, info=info)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def graph(pr):
        pg = pkg.PoseGraph(0)
        pg.set_graph(g["init"], g["ij"], g["meas"], g["info"], priors=pr)
        pg.build()
        return pg

    def timed(pg):
        stream = C.c_void_p(pg.lib.lslam_pg_stream(pg.h))
        ms = []
        for _ in range(REPS + 20):
            assert hip.hipEventRecord(ev[0], stream) == 0
            assert pg.lib.lslam_pg_linearize(pg.h, None, None, None, None, None) == 0  # waits for the stream itself
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]) == 0
            ms.append(t.value)
        ms = ms[20:]  # warm-up launches dropped
        return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "p90_us": 1e3 * sorted(ms)[int(0.9 * len(ms))]}

    def one_lm_iteration(pr):
        ms, trials = [], []
        for _ in range(LM_REPS):
            pg = graph(pr)
            pg.optimize(1)
            ms.append(pg.last_stats.gpu_ms_total)
            trials.append(pg.last_stats.lm_trials)
            pg.close()
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "trials": trials}

    out = {"tool": "bench_prior_linearize", "keyframes": n, "edges": len(g["ij"]), "reps": REPS}
    pg = graph(None)
    out["no_priors"] = timed(pg)
    pg.set_priors(priors)
    out["xyz_prior_per_keyframe"] = timed(pg)
    pg.set_priors(None)
    out["no_priors_again"] = timed(pg)
    pg.close()
    out["xyz_prior_per_keyframe"]["over_no_priors"] = out["xyz_prior_per_keyframe"]["median_us"] / out["no_priors"]["median_us"]
    out["lm_iteration_no_priors"] = one_lm_iteration(None)
    out["lm_iteration_xyz_prior_per_keyframe"] = one_lm_iteration(priors)
    for e in ev:
        hip.hipEventDestroy(e)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
