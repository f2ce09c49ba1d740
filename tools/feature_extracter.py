#!/usr/bin/env python3
"""The reference's featureExtracter executable (io_module/feature_extracter.cpp, scripts/map_convert_for_localization.sh) on this
backend: a dense survey cloud IN.pcd becomes the corner / surf cube map OUT_DIR (index.txt plus <count>.pcd) that
LaserLocalization.load_map opens.

    python tools/feature_extracter.py IN.pcd OUT_DIR [--paged] [--partition-leaf 50 --partition-min-points 1000 ...]

IN.pcd is read by the library's PCD reader (DATA ascii or binary; binary_compressed is refused with a message).  --paged also
writes index2.txt (lslam_index_convert) for the dynamic mode of the localisation node.  Every field of lslam_survey_params can
be given as --field-name VALUE; the defaults are the reference's literals."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALARS = {"boundary_angle": float, "partition_leaf": float, "partition_min_points": int, "filter_leaf": float,
           "filter_min_points": int, "normal_radius": float, "knn_k": int, "smoothness_angle": float, "cluster_min": int,
           "cluster_max": int, "boundary_radius": float, "feature_leaf": float, "feature_min_points": int, "cube_size": float,
           "knn_cell": float}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pcd")
    ap.add_argument("out_dir")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--paged", action="store_true", help="also write index2.txt for the paged localisation node")
    ap.add_argument("--cube-dims", type=int, nargs=3)
    ap.add_argument("--cube-origin", type=int, nargs=3)
    for name, ty in SCALARS.items():
        ap.add_argument("--" + name.replace("_", "-"), type=ty)
    a = ap.parse_args(argv)
    if not os.path.isfile(a.pcd):
        print("feature_extracter: %s: no such file" % a.pcd, file=sys.stderr)
        return 2
    os.makedirs(a.out_dir, exist_ok=True)
    pkg = importlib.import_module("the-cooper-mapper_amd")
    kw = {k: getattr(a, k) for k in list(SCALARS) + ["cube_dims", "cube_origin"] if getattr(a, k) is not None}
    try:
        ctx = pkg.Context(a.device)
        m = pkg.survey_map.extract_file(ctx, a.pcd, **kw)
        m.save(a.out_dir)
        st = m.info()
        if a.paged:
            rc = ctx.lib.lslam_index_convert(os.path.join(a.out_dir, "index.txt").encode(), *[int(v) for v in m.params.cube_origin],
                                             os.path.join(a.out_dir, "index2.txt").encode())
            if rc != 0:
                raise pkg.LslamError(rc, ctx.lib.lslam_last_error().decode())
        m.close()
        ctx.close()
    except pkg.LslamError as e:
        print("feature_extracter: %s" % e, file=sys.stderr)
        return 1
    print("Input points size :%d" % (st["points_in"] + st["points_nonfinite"]))
    print("blocks %d (+%d below the minimum), filtered points %d (%d without a normal), regions kept %d / dropped %d, label sweeps %d"
          % (st["blocks_kept"], st["blocks_dropped"], st["filtered_points"], st["undefined_normals"], st["clusters_kept"],
             st["clusters_dropped"], st["label_sweeps"]))
    print("corner points %d, surf points %d -> %s" % (st["n_corner"], st["n_surf"], a.out_dir))
    return 0


if __name__ == "__main__":
    sys.exit(main())
