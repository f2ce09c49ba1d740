#!/usr/bin/env python3
"""What a covariance costs: lslam_pg_relative_covariances on the bench graph (tests/golden/posegraph_bench.g2o.gz) at its stored
optimum (tests/golden/posegraph_bench_optimum.npz), for n_q = 1, 8 and 32 queries against the newest keyframe, with the
block-Jacobi preconditioner alone (coarse 0) and with the second level (coarse 1): PCG iterations, wall ms per call (median of
REPS calls, each ends with its own read-back) and ms per solved column.  Beside them the parent's one-vector solve: one
lslam_pg_solve at lambda = 1e-12 on the same system -- its tolerance is 1e-10, so the covariance calls run at rel_tol = 1e-10
as well -- on a graph created with the same preconditioner (LSLAM_PG_COARSE, read when a graph is created).  A full panel is
60 columns: n_q = 8 solves 54 columns in one panel, n_q = 32 solves 198 in four.  Prints one line per figure, then one JSON line."""
import gzip
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "5"))
TOL = 1e-10


def main():
    pkg = importlib.import_module("the-cooper-mapper_amd")
    gold = os.path.join(ROOT, "tests", "golden")
    opt = np.load(os.path.join(gold, "posegraph_bench_optimum.npz"))["poses"]
    out = dict(rel_tol=TOL, reps=REPS, rows=[])
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "posegraph_bench.g2o")
        with gzip.open(os.path.join(gold, "posegraph_bench.g2o.gz"), "rb") as src, open(f, "wb") as dst:
            shutil.copyfileobj(src, dst)
        g = pkg.PoseGraph.read_g2o(f)
    n = len(opt)
    ref = n - 1
    rng = np.random.default_rng(0)
    pool = rng.permutation(n - 1)
    for coarse in (0, 1):
        os.environ["LSLAM_PG_COARSE"] = str(coarse)
        pg = pkg.PoseGraph(0)
        pg.set_graph(opt, g["ij"], g["meas"], g["info"], fixed=g["fixed"])
        pg.linearize()
        ts, its = [], 0
        for _ in range(REPS):
            t0 = time.perf_counter()
            _, its = pg.solve(1e-12)
            ts.append((time.perf_counter() - t0) * 1e3)
        row = dict(what="lslam_pg_solve", coarse=coarse, columns=1, iters=its, ms_per_call=statistics.median(ts),
                   ms_per_column=statistics.median(ts))
        out["rows"].append(row)
        print("coarse %d  lslam_pg_solve(1e-12)           : %5d iterations  %9.3f ms" % (coarse, its, row["ms_per_call"]))
        for nq in (1, 8, 32):
            vs = [int(v) for v in pool[:nq]]
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                pg.relative_covariances(ref, vs, rel_tol=TOL, max_iters=20000, coarse=coarse)
                ts.append((time.perf_counter() - t0) * 1e3)
            st = pg.marginal_stats
            ms = statistics.median(ts)
            row = dict(what="relative_covariances", coarse=coarse, n_q=nq, columns=st.columns, panels=st.panels, iters_max=st.iters_max,
                       iters_mean=st.iters_sum / st.columns, ms_per_call=ms, ms_per_column=ms / st.columns,
                       ms_per_panel_iteration=ms / (st.panels * max(st.iters_max, 1)))
            out["rows"].append(row)
            print("coarse %d  relative_covariances n_q %2d     : %5d iterations (max), %3d columns in %d panels  %9.3f ms  "
                  "%8.3f ms per column" % (coarse, nq, st.iters_max, st.columns, st.panels, ms, row["ms_per_column"]))
        pg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
