#!/usr/bin/env python3
"""Euclidean clustering of a point cloud file on the GPU - the reference's ``euclidean_clustering`` CLI.

``python euclidean_clustering.py FILE.ply [--cluster_tolerance 0.1] [--min_cluster_size 10] [--max_cluster_size 10000]``

Arguments and defaults of ``pointstowood/src/euclidean_clustering.py:49-55``; the two printed counts of :69-70; the output of
``pointstowood/utils/euclidean_clustering_optim.py:86-93``: ``<dir>/<base>_clustered.ply`` next to the input with every input
column plus ``cluster_id`` (-1 = noise).  The clusters are ``pointstowood_amd.cluster.EuclideanCluster``'s: the reference's
``src/`` semantics (components numbered by their smallest point index), not the multiprocessing variant's racy numbering.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser(description="Perform Euclidean Clustering on a point cloud file.")
    p.add_argument("input_file", help="Path to the input point cloud file")
    p.add_argument("--cluster_tolerance", type=float, default=0.1, help="Cluster tolerance (epsilon)")
    p.add_argument("--min_cluster_size", type=int, default=10, help="Minimum cluster size")
    p.add_argument("--max_cluster_size", type=int, default=10000, help="Maximum cluster size")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    path = args.input_file
    if os.path.splitext(path)[1].lower() != ".ply":
        raise SystemExit(f"{path}: only .ply input is built (the reference also reads .las / .pcd through laspy / its own parser)")
    from pointstowood_amd import io
    from pointstowood_amd.cluster import euclidean_cluster

    cols, xyz = io.read_ply_points(path)
    labels, n_clusters = euclidean_cluster(xyz, args.cluster_tolerance, args.min_cluster_size, args.max_cluster_size)
    labels = labels.cpu().numpy()
    print(f"Number of clusters: {n_clusters}")
    print(f"Number of noise points: {int(np.sum(labels == -1))}")
    out = dict(cols)
    out["cluster_id"] = labels                   # (an input cluster_id column is replaced in place, like the reference's)
    opath = os.path.join(os.path.dirname(path), os.path.splitext(os.path.basename(path))[0] + "_clustered.ply")
    io.write_ply(opath, out)
    print(f"Clustered point cloud saved to: {opath}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
