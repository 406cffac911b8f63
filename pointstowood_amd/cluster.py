"""Euclidean clustering of a point cloud on the GPU: ``EuclideanCluster`` (``pointstowood/src/euclidean_clustering.py:7-47``).

Points i and j are joined when their float64 distance is at most ``cluster_tolerance`` (the reference's
``cKDTree.query_ball_point(points[i], r)``, p = 2, on the caller's float64 coordinates); a cluster is a connected component
of that graph; components of ``min_cluster_size <= size <= max_cluster_size`` points are numbered 0, 1, ... in ascending
order of their smallest point index (the order the reference's seed loop meets them) and every other point is -1.

The reference grows every cluster by a Python breadth-first search, one KD-tree query per point.  Here the points are
sorted once into the plot's uniform cell grid (``plotgrid.build``), and ``p2w_euclid_cluster`` (``csrc/p2w_cluster.hip``)
joins every pair of adjacent cells by a lock-free union-find and numbers the components - deterministic whatever the scheduling,
because a component's root is its smallest index.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, plotgrid
from ._lib import check, lib, ptr
from .plotgrid import safe_cell  # noqa: F401  (the derivation lives beside the grid's construction)

_NONFINITE = "data must be finite, check for nan or inf values"      # what scipy's cKDTree raises
_BIG = 1 << 62


def _size_bounds(min_size, max_size):
    """The reference's ``min_cluster_size <= len(cluster) <= max_cluster_size`` for any real bounds, as int64 (a NaN bound
    keeps nothing, like the reference's comparison)."""
    lo, hi = float(min_size), float(max_size)
    if math.isnan(lo) or math.isnan(hi):
        return _BIG, 0
    lo = 0 if lo <= 0 else (_BIG if lo >= _BIG else math.ceil(lo))
    hi = -1 if hi < 0 else (_BIG if hi >= _BIG else math.floor(hi))
    return lo, hi


def _check_tolerance(tolerance) -> float:
    r = float(tolerance)
    if not (r >= 0.0) or math.isinf(r):
        raise ValueError(f"cluster_tolerance must be a finite number >= 0, got {tolerance!r}")
    return r


def euclidean_cluster(xyz: torch.Tensor, tolerance: float, min_size=1, max_size=np.inf, cell: float | None = None,
                      table_cells: int = 1 << 30, stats: dict | None = None):
    """(labels [n] int64 on xyz's device, n_clusters) of the points ``xyz`` [n, 3] (float32 or float64, CUDA).

    ``cell``: the grid's cell size (default and minimum: ``safe_cell``); ``table_cells``: largest grid whose cell -> first point
    table is built (beyond it the runs are found by bisection of the sorted keys).  ``stats`` (a dict, optional) receives the GPU
    time of every stage in ms (grid / link / compress / number: the stages run one after the other, each timed by events) and
    the number of point pairs the link stage measured."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"points must be an [n, 3] array, got shape {tuple(getattr(xyz, 'shape', ()))}")
    if xyz.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"points must be float32 or float64, got {xyz.dtype}")
    r = _check_tolerance(tolerance)
    lo, hi = _size_bounds(min_size, max_size)
    _lib.require_cuda(xyz)
    n, dev = xyz.shape[0], xyz.device
    if n >= (1 << 31) - 1:
        raise ValueError(f"{n} points: at most 2^31 - 2 are supported")
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), 0
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError(_NONFINITE)
    L = lib()
    mark, elapsed_ms = _lib.stage_timer(stats is not None)

    def checked_cell(loc):
        safe = safe_cell(r, float(loc.max()))
        if not (cell is None or float(cell) >= safe):
            raise ValueError(f"cell {cell} is smaller than the safe cell {safe} for tolerance {r}")
        return safe if cell is None else cell

    mark()
    g = plotgrid.build(xyz, checked_cell, table_cells)
    mark()
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    pairs = torch.zeros(1, dtype=torch.int64, device=dev) if stats is not None else None
    ws = torch.empty(int(L.p2w_euclid_cluster_ws_bytes(n)), dtype=torch.uint8, device=dev)
    args = (ptr(g.xyz_sorted), ptr(g.order), ptr(g.keys), ptr(g.cell_start), ptr(g.grid), n, r, lo, hi)
    tail = (ptr(labels), ptr(counts), ptr(pairs), ptr(ws), ws.numel(), _lib.stream())
    if stats is None:
        check(L.p2w_euclid_cluster(*args, _lib.CLUSTER_ALL, *tail), "euclid_cluster")
    else:
        for st in (_lib.CLUSTER_LINK, _lib.CLUSTER_COMPRESS, _lib.CLUSTER_NUMBER):
            check(L.p2w_euclid_cluster(*args, st, *tail), "euclid_cluster")
            mark()
    nc, nn = counts.cpu().tolist()
    if stats is not None:
        ms = elapsed_ms()
        stats.update(grid_ms=ms[0], link_ms=ms[1], compress_ms=ms[2], number_ms=ms[3], pairs=int(pairs.item()),
                     cell=g.cell if cell is None else float(cell), n_cells=g.n_cells, table=g.cell_start is not None, n_noise=nn)
    return labels, nc


class EuclideanCluster:
    """``EuclideanCluster(cluster_tolerance, min_cluster_size, max_cluster_size=np.inf).cluster(points)`` -> labels, as the
    reference's class (euclidean_clustering.py:7-30).  ``points``: [n, 3] float32 / float64, a numpy array (labels: numpy
    int64) or a CUDA tensor (labels: CUDA int64)."""

    def __init__(self, cluster_tolerance, min_cluster_size, max_cluster_size=np.inf):
        self.cluster_tolerance = cluster_tolerance
        self.min_cluster_size = min_cluster_size
        self.max_cluster_size = max_cluster_size

    def cluster(self, points):
        host = not isinstance(points, torch.Tensor)
        if host:
            a = np.asarray(points)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"points must be an [n, 3] array, got shape {a.shape}")
            if a.dtype != np.float32:
                a = a.astype(np.float64)
            if not np.isfinite(a).all():
                raise ValueError(_NONFINITE)
            points = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        labels, _ = euclidean_cluster(points, self.cluster_tolerance, self.min_cluster_size, self.max_cluster_size)
        return labels.cpu().numpy() if host else labels
