#!/usr/bin/env python3
"""Path length (pointstowood_amd.pathlength.path_length) on synthetic trees: GPU time per stage (kNN, growth, SSSP), growth steps,
edges and edges per second, against a CPU baseline on the same tree.

    python tools/pathlength_bench.py [--n 100000 1000000] [--knn 100] [--repeat 3] [--cpu-n 100000] [--out FILE.json]

Trees: a stem of 12 m (radius 0.25 m) with 40 branches (radius 3-6 cm), points uniform on the surfaces with 3 mm noise, the point
density set to give n points.  The reference defaults (kpairs 3, knn 100, nbrs_threshold 0.15, step 0.05), base = the first point of
least z; one warm-up run per size, then ``--repeat`` runs; medians are reported.  CPU baseline (one process) on trees of at most
``--cpu-n`` points: scipy ``cKDTree.query(k=knn)`` plus ``scipy.sparse.csgraph.dijkstra`` over the graph the GPU built - a lower
bound of the reference, whose growth loop is Python.  The reference's own time is recorded as measured on a workstation CPU core
(REFERENCE_CPU below); it needs sklearn and networkx, which the GPU machines do not carry.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import pathlength as PL  # noqa: E402

# array_to_graph + extract_path_info of the reference on tests/golden/pathlength/tree_defaults (5 043 points, script defaults),
# one CPU core: 0.30 s for the graph, 119 steps, 19 995 edges
REFERENCE_CPU = {"n": 5043, "graph_s": 0.30, "steps": 119, "edges": 19995}


def _cylinder(g, a, b, r, m):
    axis = b - a
    L = np.linalg.norm(axis)
    u = axis / L
    t = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, t)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    s, phi = g.uniform(0, L, m), g.uniform(0, 2 * np.pi, m)
    p = a + s[:, None] * u + r * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return p + g.normal(0, 0.003, p.shape)


def tree(n, seed=0):
    g = np.random.default_rng(seed)
    cyl = [(np.zeros(3), np.array([0.1, 0.05, 12.0]), 0.25)]
    for i, h in enumerate(np.linspace(3.0, 11.5, 40)):
        ang = i * 2.4
        d = np.array([np.cos(ang), np.sin(ang), 0.5])
        a = np.array([0.0, 0.0, h]) + 0.24 * np.array([np.cos(ang), np.sin(ang), 0.0])
        cyl.append((a, a + (3.5 - 0.2 * h) * d / np.linalg.norm(d), 0.06 - 0.002 * h))
    area = np.array([2 * np.pi * r * np.linalg.norm(b - a) for a, b, r in cyl])
    m = np.maximum(1, np.round(n * area / area.sum()).astype(int))
    m[0] += n - m.sum()
    p = np.concatenate([_cylinder(g, a, b, r, k) for (a, b, r), k in zip(cyl, m)])
    return p[g.permutation(len(p))]


def gpu_runs(x, knn, repeat):
    PL.path_length(x, knn=knn)
    runs = []
    for _ in range(repeat):
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        PL.path_length(x, knn=knn, stats=st)
        torch.cuda.synchronize()
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        runs.append(st)
    return runs


def cpu_baseline(xyz, knn, edges):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    cKDTree(xyz).query(xyz, k=knn)
    t1 = time.perf_counter()
    e = edges[edges[:, 0] != edges[:, 1]]
    w = np.sqrt(((xyz[e[:, 0], 0] - xyz[e[:, 1], 0]) ** 2 + (xyz[e[:, 0], 1] - xyz[e[:, 1], 1]) ** 2) + (xyz[e[:, 0], 2] - xyz[e[:, 1], 2]) ** 2)
    A = coo_matrix((w, (e[:, 0], e[:, 1])), shape=(len(xyz), len(xyz))).tocsr()
    dijkstra(A, directed=False, indices=int(np.argmin(xyz[:, 2])))
    t2 = time.perf_counter()
    return {"knn_ms": (t1 - t0) * 1e3, "dijkstra_ms": (t2 - t1) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--knn", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pathlength_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "knn": a.knn, "kpairs": 3, "nbrs_threshold": 0.15, "nbrs_threshold_step": 0.05,
           "reference_cpu": REFERENCE_CPU, "sizes": []}
    for n in a.n:
        xyz = tree(n)
        x = torch.from_numpy(xyz).cuda()
        runs = gpu_runs(x, a.knn, a.repeat)
        med = {k: statistics.median([r[k] for r in runs]) for k in ("knn_ms", "grow_ms", "sssp_ms", "wall_ms")}
        last = runs[-1]
        row = {"n": n, **med, "steps": last["steps"], "edges": last["edges"], "gap_steps": last["gap_steps"],
               "threshold_raises": last["threshold_raises"], "grow_launches": last["grow_launches"],
               "sssp_rounds": last["sssp_rounds"], "sssp_launches": last["sssp_launches"], "knn_cell": last["knn_cell"],
               "edges_per_s": last["edges"] / ((med["grow_ms"] + med["sssp_ms"]) * 1e-3),
               "points_per_s": n / (med["wall_ms"] * 1e-3), "unreached": bool(last["stopped_unreached"])}
        if n <= a.cpu_n:
            nbr = PL.knn_rows(x, a.knn)
            _, edges, _ = PL._grow(x, nbr, int(torch.argmin(x[:, 2]).item()), 3, 0.15, 0.05, float("inf"))
            row["cpu_baseline"] = cpu_baseline(xyz, a.knn, edges.cpu().numpy().astype(np.int64))
        print(json.dumps(row), flush=True)
        res["sizes"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
