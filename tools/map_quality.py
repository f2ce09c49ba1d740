#!/usr/bin/env python3
"""Score a saved map: python3 tools/map_quality.py DIR [--radius R] [--min-neighbors K] [--lambda-floor F] [--device N]

DIR is a map directory as lslam_fmap_save / FeatureMap.save_cloud_to_files / Graph.save write it (index.txt and one PCD per
cube and feature type).  The cubes are loaded into a device FeatureMap large enough for every cube the index names, and the mean
map entropy (MME) and mean plane variance (MPV) of each feature type are evaluated where the points lie (FeatureMap.quality).
Prints one line of JSON per feature type.  Lower is crisper; compare two maps of the same drive at the same parameters."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cube_dims(directory):
    """The smallest cube array that holds every cube of DIR/index.txt (lines: file, type, i, j, k, points)."""
    dims = [1, 1, 1]
    with open(os.path.join(directory, "index.txt")) as f:
        for line in f:
            w = line.split()
            if len(w) >= 6:
                for d in range(3):
                    dims[d] = max(dims[d], int(w[2 + d]) + 1)
    return dims


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--min-neighbors", type=int, default=5)
    ap.add_argument("--lambda-floor", type=float, default=1e-8)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(args.directory, "index.txt")):
        sys.exit("%s: no index.txt (not a saved map directory)" % args.directory)
    pkg = importlib.import_module("the-cooper-mapper_amd")
    ctx = pkg.Context(args.device)
    fm = pkg.FeatureMap(ctx, *cube_dims(args.directory))
    fm.load_cloud_from_files(args.directory)
    for which in ("corner", "surf"):
        st = fm.quality(which, radius=args.radius, min_neighbors=args.min_neighbors, lambda_floor=args.lambda_floor)
        print(json.dumps(dict(feature=which, directory=args.directory, radius=args.radius, min_neighbors=args.min_neighbors,
                              lambda_floor=args.lambda_floor, **st)))
    fm.close()
    ctx.close()


if __name__ == "__main__":
    main()
