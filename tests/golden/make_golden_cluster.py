#!/usr/bin/env python3
"""Generate the Euclidean-clustering golden fixtures in tests/golden/cluster/ FROM THE REFERENCE ITSELF.

Companion of make_golden_host.py: this script imports the reference's unmodified ``EuclideanCluster``
(``pointstowood/src/euclidean_clustering.py``) and its ``src/io.py`` from ``/root/reference/pointstowood`` in the authoring
container (scipy and pandas installed, no stubs), runs them on the cases below and records inputs and outputs:

  <case>.npz         xyz [n, 3] float64, tolerance, min_size, max_size (may be inf), labels [n] int64 = the reference's
                     ``EuclideanCluster(tolerance, min_size, max_size).cluster(xyz)``
  cli_input.ply      a small cloud with extra columns; cli_input_clustered.ply = what the reference's CLI flow writes for it
                     (load_file -> EuclideanCluster with the CLI defaults -> ``cluster_id`` column -> save_file, the output
                     convention of utils/euclidean_clustering_optim.py:86-93), cli.json = the counts it prints
  manifest.json      sha256 of every file above

Cases (each small enough for the reference's per-point Python BFS): blobs + sparse noise; a cubic lattice with spacing equal to
the tolerance (ties at d == r, decided by fp64 rounding) with a third of its points removed; the same lattice at a large easting;
exact duplicates with tolerance 0; a size filter where max_size drops the largest component and min_size the singletons; one
point; no points.  The reference's source never enters this repo; only these data vectors do.

    python tests/golden/make_golden_cluster.py
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cluster")
sys.path.insert(0, "/root/reference/pointstowood")

import src.io as ref_io  # noqa: E402
from src.euclidean_clustering import EuclideanCluster  # noqa: E402


def blobs(seed=0, n_blob=24, per=900, n_noise=2500):
    g = np.random.default_rng(seed)
    centres = g.uniform([0, 0, 0], [40, 40, 12], (n_blob, 3))
    sig = g.uniform(0.05, 0.25, n_blob)
    pts = [c + g.standard_normal((int(per * g.uniform(0.2, 1.5)), 3)) * s for c, s in zip(centres, sig)]
    pts.append(g.uniform([0, 0, 0], [40, 40, 12], (n_noise, 3)))
    p = np.concatenate(pts)
    return p[g.permutation(len(p))]


def lattice(seed=1, side=30, spacing=0.1, keep=0.66, offset=(0.0, 0.0, 0.0)):
    g = np.random.default_rng(seed)
    idx = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    idx = idx[g.random(len(idx)) < keep]
    idx = idx[g.permutation(len(idx))]
    return idx * spacing + np.asarray(offset)


def duplicates(seed=2, n_unique=6000):
    g = np.random.default_rng(seed)
    u = np.round(g.uniform(0, 20, (n_unique, 3)), 3)
    rep = g.integers(1, 5, n_unique)
    p = np.repeat(u, rep, axis=0)
    return p[g.permutation(len(p))]


def filtered(seed=3):
    g = np.random.default_rng(seed)
    sizes = [3000, 1200, 800, 400, 50, 2]
    pts = [np.array([12.0 * i, 0.0, 0.0]) + g.uniform(-1, 1, (s, 3)) * (0.2 * s ** (1 / 3)) for i, s in enumerate(sizes)]
    pts.append(g.uniform([0, 30, 0], [80, 60, 20], (600, 3)))          # singletons
    p = np.concatenate(pts)
    return p[g.permutation(len(p))]


def cases():
    big = filtered()
    lab = EuclideanCluster(0.6, 1).cluster(big)
    largest = np.bincount(lab).max()
    return {
        "blobs_noise": (blobs(), 0.1, 10, 10000),
        "lattice_tie": (lattice(), 0.1, 1, np.inf),
        "lattice_easting": (lattice(offset=(512345.0, 6012345.0, 123.0)), 0.1, 1, np.inf),
        "duplicates_tol0": (duplicates(), 0.0, 2, np.inf),
        "filter_minmax": (big, 0.6, 2, float(largest - 1)),
        "single_point": (np.array([[1.5, -2.25, 3.0]]), 0.1, 1, np.inf),
        "empty": (np.zeros((0, 3)), 0.1, 1, np.inf),
    }


def cli_case(tmp):
    g = np.random.default_rng(4)
    xyz = blobs(seed=5, n_blob=8, per=600, n_noise=800) * 0.5 + np.array([300000.0, 5000000.0, 50.0])
    import pandas as pd
    df = pd.DataFrame({"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "reflectance": g.uniform(-25, 5, len(xyz)),
                       "pwood": g.random(len(xyz))})
    inp = os.path.join(tmp, "cli_input.ply")
    ref_io.write_ply(inp, df)
    # the reference CLI's flow with its defaults (src/euclidean_clustering.py:49-70, utils/euclidean_clustering_optim.py:86-93)
    pc_data, headers = ref_io.load_file(filename=inp, additional_headers=True)
    labels = EuclideanCluster(cluster_tolerance=0.1, min_cluster_size=10, max_cluster_size=10000).cluster(pc_data[["x", "y", "z"]].values)
    counts = {"n_clusters": int(len(np.unique(labels[labels != -1]))), "n_noise": int(np.sum(labels == -1))}
    pc_data["cluster_id"] = labels
    headers = list(dict.fromkeys(headers + ["cluster_id"]))
    outp = os.path.join(tmp, "cli_input_clustered.ply")
    ref_io.save_file(outp, pc_data.copy(), additional_fields=headers)
    shutil.copy(inp, os.path.join(OUT, "cli_input.ply"))
    shutil.copy(outp, os.path.join(OUT, "cli_input_clustered.ply"))
    with open(os.path.join(OUT, "cli.json"), "w") as f:
        json.dump({"args": {"cluster_tolerance": 0.1, "min_cluster_size": 10, "max_cluster_size": 10000}, **counts}, f, indent=1)
    return counts


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (xyz, tol, mn, mx) in cases().items():
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        labels = np.asarray(EuclideanCluster(tol, mn, mx).cluster(xyz), dtype=np.int64)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), xyz=xyz, tolerance=np.float64(tol), min_size=np.float64(mn),
                            max_size=np.float64(mx), labels=labels)
        k = labels.max() + 1 if len(labels) else 0
        print(f"{name}: {len(xyz)} points, {k} clusters, {int((labels == -1).sum())} noise")
    with tempfile.TemporaryDirectory() as tmp:
        print("cli:", cli_case(tmp))
    man = {}
    for f in sorted(os.listdir(OUT)):
        if f != "manifest.json":
            man[f] = hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
