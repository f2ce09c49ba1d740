#!/usr/bin/env python3
"""Cost of one robust linearisation against a plain one on the 5 000-keyframe bench graph (synth.make_pose_graph), timed with
HIP events on the library's own stream (lslam_pg_stream): median of REPS launches of lslam_pg_linearize without read-back --
the edge kernel, the two assemble kernels and the chi2 sum.  Configurations: no kernels; DCS 1 on the loop edges (what
Graph(loop_robust_kernel="DCS") sets); Cauchy 0.1 on every edge (fp64 log and a division per edge: the dearest kernel
everywhere).  Prints one JSON line."""
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


def main():
    pkg = importlib.import_module("the-cooper-mapper_amd")
    synth = importlib.import_module("the-cooper-mapper_amd.synth")
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    g = synth.make_pose_graph()
    ne, n_odo = len(g["ij"]), len(g["init"]) - 1
    pg = pkg.PoseGraph(0)
    pg.set_graph(g["init"], g["ij"], g["meas"], g["info"])
    pg.build()
    stream = C.c_void_p(pg.lib.lslam_pg_stream(pg.h))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed():
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

    out = {"keyframes": len(g["init"]), "edges": ne, "reps": REPS}
    out["plain"] = timed()
    kinds = np.zeros(ne, np.int32)
    kinds[n_odo:] = 3
    pg.set_robust_kernels(kinds, 1.0)
    out["dcs_on_loop_edges"] = timed()
    pg.set_robust_kernels(np.full(ne, 2, np.int32), 0.1)
    out["cauchy_on_every_edge"] = timed()
    pg.clear_robust_kernels()
    out["plain_again"] = timed()
    for k in ("dcs_on_loop_edges", "cauchy_on_every_edge"):
        out[k]["over_plain"] = out[k]["median_us"] / out["plain"]["median_us"]
    for e in ev:
        hip.hipEventDestroy(e)
    pg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
