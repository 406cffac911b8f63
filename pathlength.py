#!/usr/bin/env python3
"""Path length from the stem base of point cloud files on the GPU - the reference's ``utils/pathlength-batch.py``.

``python pathlength.py FILE.ply [FILE.ply ...]`` (one argument holding several paths separated by whitespace works as in the
reference) ``[--downsample 0.05] [--kpairs 3] [--knn 100] [--nbrs-threshold 0.15] [--nbrs-threshold-step 0.05]``

Defaults of ``pathlength-batch.py:29-64``; the base is the first point of least z of the downsampled cloud (:67).  The reference's
``downsample_cloud`` / ``upsample_cloud`` are not part of its tree, so the downsampling is this project's own
(``pointstowood_amd.pathlength.downsample``): the ``p2w_voxel_sample`` grid of cell ``--downsample``, each occupied cell represented by
its largest point index, the representatives in ascending index order, and every input point given its representative's path
length; ``--downsample 0`` runs on every point.  The output ``<dir>/<base>_pathlength.ply`` next to the input holds every input column
plus a float64 ``pathlength``; points whose representative was never reached are left out, as the reference's upsampling of the
graph's nodes leaves them out.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description="Path length from the stem base over a kNN graph, per point cloud file.")
    p.add_argument("files", nargs="+", help="PLY files (an argument may hold several paths separated by whitespace)")
    p.add_argument("--downsample", type=float, default=0.05, help="downsampling cell in metres (0: every point)")
    p.add_argument("--kpairs", type=int, default=3, help="points linked per point and step")
    p.add_argument("--knn", type=int, default=100, help="neighbours searched per point (at most 100)")
    p.add_argument("--nbrs-threshold", type=float, default=0.15, help="largest gap bridged before the threshold is raised")
    p.add_argument("--nbrs-threshold-step", type=float, default=0.05, help="threshold increment when no point can be added")
    return p


def file_list(args):
    return [f for a in args.files for f in a.split()]


def process(path, args):
    from pointstowood_amd import io
    from pointstowood_amd.pathlength import downsample, path_length

    cols, xyz = io.read_ply_points(path)
    if args.downsample > 0:
        reps, owner = downsample(xyz, args.downsample)
        sub = xyz[reps].contiguous()
    else:
        owner = None
        sub = xyz
    dist, _ = path_length(sub, None, args.kpairs, args.knn, args.nbrs_threshold, args.nbrs_threshold_step)
    d = (dist[owner] if owner is not None else dist).cpu().numpy()
    keep = ~np.isnan(d)
    out = {k: np.asarray(v)[keep] for k, v in cols.items()}
    out["pathlength"] = d[keep]
    opath = os.path.join(os.path.dirname(path), os.path.splitext(os.path.basename(path))[0] + "_pathlength.ply")
    io.write_ply(opath, out)
    print(f"{path}: {int(keep.sum())} of {len(d)} points reached, {sub.shape[0]} graph nodes -> {opath}")
    return opath


def main(argv=None):
    args = build_parser().parse_args(argv)
    files = file_list(args)
    for f in files:
        if os.path.splitext(f)[1].lower() != ".ply":
            raise SystemExit(f"{f}: only .ply input is built")
    if not 1 <= args.knn <= 100:
        raise SystemExit(f"--knn must be in 1 .. 100, got {args.knn}")
    for f in files:
        print(f"Processing {os.path.splitext(os.path.basename(f))[0]}")
        process(f, args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
