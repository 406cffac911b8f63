#!/usr/bin/env python3
"""Euclidean clustering (pointstowood_amd.cluster) on the synthetic forest plot: GPU time per stage, points/s, pairs measured and
components found at several tolerances, against a CPU baseline on a stated subset.

    python tools/cluster_bench.py [--n 10000000] [--tol 0.05 0.1 0.2] [--cpu-n 1000000] [--repeat 3] [--out FILE.json]

GPU: ``synthetic_voxels.forest_plot(n)`` (float32 coordinates), every component kept (min_size 1), one warm-up run per tolerance,
then ``--repeat`` runs with the stages launched one at a time between events (grid = local coordinates + sort + cell table, link,
compress, number); medians are reported.  The same on the first ``--cpu-n`` points of the plot (an i.i.d. thinning: the plot's
points are generated independently), where the CPU baseline runs: scipy ``cKDTree.query_pairs(r)`` +
``scipy.sparse.csgraph.connected_components`` (one process; a lower bound of the reference's per-point BFS, which was not run).
For the kernel shares run it under ``rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py ...``.
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
from pointstowood_amd import synthetic_voxels as synth  # noqa: E402
from pointstowood_amd.cluster import euclidean_cluster  # noqa: E402

STAGES = ("grid_ms", "link_ms", "compress_ms", "number_ms")


def gpu_runs(xyz, tol, repeat):
    euclidean_cluster(xyz, tol, 1)                     # warm-up (first launches, allocator)
    runs = []
    for _ in range(repeat):
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, k = euclidean_cluster(xyz, tol, 1, stats=st)
        torch.cuda.synchronize()
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        st["components"] = k
        runs.append(st)
    out = {s: statistics.median(r[s] for r in runs) for s in STAGES + ("wall_ms",)}
    out["gpu_ms"] = sum(out[s] for s in STAGES)
    out["points_per_s"] = xyz.shape[0] / (out["gpu_ms"] * 1e-3)
    for key in ("pairs", "components", "cell", "n_cells", "table"):
        out[key] = runs[-1][key]
    assert len({r["components"] for r in runs}) == 1 and len({r["pairs"] for r in runs}) == 1
    return out


def cpu_baseline(xyz, tol):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = xyz.shape[0]
    t0 = time.perf_counter()
    pr = cKDTree(xyz).query_pairs(tol, output_type="ndarray")
    k, _ = connected_components(coo_matrix((np.ones(len(pr), dtype=np.int8), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
    dt = time.perf_counter() - t0
    return {"s": dt, "points_per_s": n / dt, "edges": int(len(pr)), "components": int(k)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--tol", type=float, nargs="+", default=[0.05, 0.1, 0.2])
    ap.add_argument("--cpu-n", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    plot = synth.forest_plot(a.n, seed=0)[:, :3].contiguous()
    dev = torch.device("cuda", 0)
    xyz = plot.to(dev)
    sub = xyz[:a.cpu_n].contiguous()
    res = {"device": torch.cuda.get_device_name(0), "n": a.n, "cpu_subset_n": a.cpu_n, "workload": "synthetic_voxels.forest_plot(n, seed=0)",
           "cpu_baseline": "scipy cKDTree.query_pairs(r) + csgraph.connected_components, one process, on the first cpu_subset_n points",
           "tolerances": {}}
    for tol in a.tol:
        row = {"gpu": gpu_runs(xyz, tol, a.repeat), "gpu_subset": gpu_runs(sub, tol, a.repeat)}
        if not a.no_cpu:
            row["cpu_subset"] = cpu_baseline(plot[:a.cpu_n].double().numpy(), tol)
            assert row["cpu_subset"]["components"] == row["gpu_subset"]["components"], (row["cpu_subset"], row["gpu_subset"])
        res["tolerances"][str(tol)] = row
        g = row["gpu"]
        print(f"r={tol}: {a.n} pts  grid {g['grid_ms']:.1f}  link {g['link_ms']:.1f}  compress {g['compress_ms']:.1f}  "
              f"number {g['number_ms']:.1f} ms  = {g['points_per_s'] / 1e6:.1f} M pts/s  pairs {g['pairs']:.3e}  components "
              f"{g['components']}  (table {g['table']}, {g['n_cells']:.3e} cells)", flush=True)
        gs = row["gpu_subset"]
        line = f"   subset {a.cpu_n}: GPU {gs['gpu_ms']:.1f} ms ({gs['points_per_s'] / 1e6:.1f} M pts/s)"
        if "cpu_subset" in row:
            c = row["cpu_subset"]
            line += f"  CPU scipy {c['s'] * 1e3:.0f} ms ({c['points_per_s'] / 1e6:.2f} M pts/s), {c['components']} components"
        print(line, flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
