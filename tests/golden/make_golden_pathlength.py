#!/usr/bin/env python3
"""Generate the path-length golden fixtures in tests/golden/pathlength/ FROM THE REFERENCE ITSELF.

Companion of make_golden_cluster.py: this script imports the reference's unmodified ``array_to_graph`` and ``extract_path_info``
(``pointstowood/utils/shortest_path.py``: sklearn NearestNeighbors + networkx) from the reference checkout given by
``P2W_REFERENCE`` (default ``/root/reference``), runs them on the cases below and records inputs and outputs:

  <case>.npz      xyz [n, 3] float64, kpairs, knn, nbrs_threshold, nbrs_threshold_step, graph_threshold, base_id;
                  edges [E, 2] int32 = the graph's undirected edges as (min, max), ascending, self-loops kept; weights [E] float64;
                  step [n] int32 = the step register (-1 for NaN); node_ids / distance = extract_path_info's Dijkstra result sorted
                  by node id (empty when the base has no edge: networkx then raises NodeNotFound, recorded as no_source = 1)
  manifest.json   sha256 of every file above

Every case is checked by brute force to have no two equal distances among the first knn + 1 entries of any row, where the
order of sklearn's KD-tree is not defined.  (knn_equals_n: sklearn's "auto" takes its brute-force search at knn >= n / 2, whose
distances come from a dot-product expansion and differ from the exact ones by a few ulps; the graph is still the exact one's.)  The reference's source never enters this repo; only these data vectors do.

    python tests/golden/make_golden_pathlength.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pathlength")
sys.path.insert(0, os.path.join(os.environ.get("P2W_REFERENCE", "/root/reference"), "pointstowood", "utils"))

import networkx as nx  # noqa: E402
from shortest_path import array_to_graph, extract_path_info  # noqa: E402

DEFAULTS = dict(kpairs=3, knn=100, nbrs_threshold=0.15, nbrs_threshold_step=0.05, graph_threshold=np.inf)


def _cylinder(g, a, b, r, density):
    """Points on the side of the cylinder of radius r from a to b, uniformly at `density` points per m^2, with 3 mm noise."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    axis = b - a
    L = np.linalg.norm(axis)
    u = axis / L
    t = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(u, t)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    m = int(2 * np.pi * r * L * density)
    s, phi = g.uniform(0, L, m), g.uniform(0, 2 * np.pi, m)
    p = a + s[:, None] * u + r * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return p + g.normal(0, 0.003, p.shape)


def tree(seed=0, density=650.0):
    """A stem of 6 m and radius 0.15 m with six branches of radius 4 cm: about 5 000 points."""
    g = np.random.default_rng(seed)
    parts = [_cylinder(g, (0, 0, 0), (0.05, 0.02, 6.0), 0.15, density)]
    for i, h in enumerate(np.linspace(2.0, 5.2, 6)):
        ang = i * 2.4
        d = np.array([np.cos(ang), np.sin(ang), 0.6])
        a = np.array([0.0, 0.0, h]) + 0.14 * np.array([np.cos(ang), np.sin(ang), 0.0])
        parts.append(_cylinder(g, a, a + 1.4 * d / np.linalg.norm(d), 0.04, density))
    p = np.concatenate(parts)
    return p[g.permutation(len(p))]


def tree_with_clumps(seed=0):
    """The tree with three detached clumps of 30 points each, 0.3 / 0.42 / 0.55 m off the stem: crossing them needs the gap step
    with several threshold raises (each clump is smaller than knn, so its rows reach back to the tree)."""
    g = np.random.default_rng(seed + 100)
    t = tree(seed)
    clumps = []
    for h, gap, ang in ((1.0, 0.30, 0.3), (3.3, 0.42, 2.0), (5.6, 0.55, 4.1)):
        c = np.array([np.cos(ang), np.sin(ang), 0.0]) * (0.15 + gap + 0.03) + np.array([0, 0, h])
        clumps.append(c + g.normal(0, 0.012, (30, 3)))
    p = np.concatenate([t] + clumps)
    return p[g.permutation(len(p))]


def _check_no_ties(xyz, knn):
    n = len(xyz)
    k = min(knn + 1, n)
    for s in range(0, n, 1024):
        q = xyz[s:s + 1024]
        d = ((q[:, None, 0] - xyz[None, :, 0]) ** 2 + (q[:, None, 1] - xyz[None, :, 1]) ** 2) + (q[:, None, 2] - xyz[None, :, 2]) ** 2
        d = np.sort(np.sqrt(d), axis=1)[:, :k]
        assert np.all(np.diff(d, axis=1) > 0), "equal distances inside a kNN row"


def cases():
    t = tree()
    g = np.random.default_rng(7)
    small = g.uniform(0, 1, (40, 3))
    return {
        "tree_defaults": (t, {}),
        "tree_gaps": (tree_with_clumps(), {}),
        "tree_k16": (tree(seed=1, density=1200.0)[:4000], dict(kpairs=1, knn=16)),
        "tree_graph_threshold": (t, dict(graph_threshold=0.07)),
        "tree_easting": (t + np.array([512345.0, 6012345.0, 123.0]), {}),
        "single_point": (np.array([[1.5, -2.25, 3.0]]), dict(knn=1)),
        "knn_equals_n": (small, dict(knn=40, nbrs_threshold=0.1)),
    }


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (xyz, over) in cases().items():
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        prm = {**DEFAULTS, **over}
        _check_no_ties(xyz, prm["knn"])
        base = int(np.argmin(xyz[:, 2]))
        t0 = time.perf_counter()
        G, steps = array_to_graph(xyz, base, prm["kpairs"], prm["knn"], prm["nbrs_threshold"], prm["nbrs_threshold_step"],
                                  prm["graph_threshold"], return_step=True)
        t_graph = time.perf_counter() - t0
        e = np.array([(min(a, b), max(a, b)) for a, b in G.edges()], dtype=np.int64).reshape(-1, 2)
        w = np.array([G[a][b]["weight"] for a, b in e], dtype=np.float64)
        o = np.lexsort((e[:, 1], e[:, 0])) if len(e) else np.zeros(0, dtype=np.int64)
        e, w = e[o], w[o]
        try:
            ids, dist = extract_path_info(G, base, return_path=False)
            no_source = 0
        except nx.NodeNotFound:
            ids, dist, no_source = [], [], 1
        ids, dist = np.asarray(ids, dtype=np.int64), np.asarray(dist, dtype=np.float64)
        o = np.argsort(ids)
        step = np.where(np.isnan(steps), -1, steps).astype(np.int32)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), xyz=xyz, base_id=np.int64(base), no_source=np.int64(no_source),
                            **{k: (np.int64(v) if k in ("kpairs", "knn") else np.float64(v)) for k, v in prm.items()},
                            edges=e.astype(np.int32), weights=w, step=step, node_ids=ids[o], distance=dist[o])
        loops = int(np.sum(e[:, 0] == e[:, 1])) if len(e) else 0
        print(f"{name}: {len(xyz)} points, {len(e)} edges ({loops} self-loops), {int(step.max())} steps, "
              f"{len(ids)} reached, {int((step < 0).sum())} unprocessed; graph {t_graph:.2f} s")
    man = {}
    for f in sorted(os.listdir(OUT)):
        if f != "manifest.json":
            man[f] = hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
