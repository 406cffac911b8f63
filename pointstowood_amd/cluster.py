"""Euclidean clustering of a point cloud on the GPU: ``EuclideanCluster`` (``pointstowood/src/euclidean_clustering.py:7-47``).

Points i and j are joined when their float64 distance is at most ``cluster_tolerance`` (the reference's
``cKDTree.query_ball_point(points[i], r)``, p = 2, on the caller's float64 coordinates); a cluster is a connected component
of that graph; components of ``min_cluster_size <= size <= max_cluster_size`` points are numbered 0, 1, ... in ascending
order of their smallest point index (the order the reference's seed loop meets them) and every other point is -1.

The reference grows every cluster by a Python breadth-first search, one KD-tree query per point.  Here the points are
sorted once into a uniform cell grid the way ``backproject.neighbours`` does it (fp32 coordinates local to the cloud's
minimum -> ``p2w_voxel_sample`` -> ``p2w_cell_starts``), and ``p2w_euclid_cluster`` (``csrc/p2w_cluster.hip``) joins every
pair of adjacent cells by a lock-free union-find and numbers the components - deterministic whatever the scheduling,
because a component's root is its smallest index.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr

_NONFINITE = "data must be finite, check for nan or inf values"      # what scipy's cKDTree raises
_BIG = 1 << 62
_EPS32 = 2.0 ** -23


def safe_cell(tolerance: float, extent: float) -> float:
    """Smallest grid cell (a float32 value) for which every pair the fp64 predicate joins lies in the same or adjacent cells.

    ``extent`` = the largest per-axis extent of the cloud, E.  The grid is built in fp32:
      * local coordinates u = fl32(fl64(x - o)) with o the per-axis minimum: |u - (x - o)| <= (2^-24 + 2^-53) E < 2^-23 E;
      * the grid origin is min u = 0 exactly (the minimum point's x - o is 0), so the key is trunc(fl32(u / res)) and
        |fl32(u / res) - u / res| <= 2^-24 E / res;
      * a joined pair has ((dx*dx + dy*dy) + dz*dz) <= r*r in fp64, so its true per-axis difference is at most r (1 + 2^-50).
    Per axis the two quotients then differ by at most (r (1 + 2^-50) + 2 * 2^-23 E + 2 * 2^-24 E) / res, which is below 1 for
    res >= r (1 + 2^-20) + 4 * 2^-23 E, and quotients less than 1 apart truncate (both >= 0) to cells at most 1 apart.  The
    value is rounded UP to float32 (the kernel divides by the float32 cell).  The cell is also at least 2^-20 E, so that the
    grid has at most 2^20 + 1 cells per axis (int64 keys, exact fp32 quotients), and positive for tolerance 0 (duplicates
    only) or a cloud of one position."""
    c = max(tolerance * (1.0 + 2.0 ** -20) + 4.0 * _EPS32 * extent, extent * 2.0 ** -20)
    if not c > 0.0:
        c = 1.0
    c32 = np.float32(c)
    if float(c32) < c:
        c32 = np.nextafter(c32, np.float32(np.inf))
    return float(c32)


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
    i32 = dict(dtype=torch.int32, device=dev)
    ev = []

    def mark():
        if stats is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

    mark()
    x64 = xyz.to(torch.float64)
    origin = torch.stack([x64[:, d].min() for d in range(3)])     # (a column reduction of [n, 3] runs on 3 outputs: 7 ms at 10^7)
    loc = x64 - origin
    extent = float(loc.max())
    safe = safe_cell(r, extent)
    if cell is None:
        cell = safe
    elif not float(cell) >= safe:
        raise ValueError(f"cell {cell} is smaller than the safe cell {safe} for tolerance {r}")
    rec = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rec[:, :3] = loc
    del loc
    ptr_c = torch.tensor([0, n], **i32)
    order = torch.empty(n, **i32)
    skeys = torch.empty(n, dtype=torch.int64, device=dev)
    grid = torch.zeros(8, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.p2w_voxel_sample_ws_bytes(n)), dtype=torch.uint8, device=dev)
    idx, ptr_out, batch_out = torch.empty(n, **i32), torch.empty(2, **i32), torch.empty(n, **i32)
    check(L.p2w_voxel_sample(ptr(rec), ptr(ptr_c), 1, n, float(cell), ptr(idx), ptr(ptr_out), ptr(batch_out), ptr(order),
                             ptr(skeys), None, ptr(grid), None, None, ptr(ws), ws.numel(), _lib.stream()), "voxel_sample")
    del idx, batch_out, ws, rec
    cs = x64[order.long()].contiguous()          # float64 coordinates in the grid's cell-sorted order
    del x64
    dims = grid.cpu()[4:7].tolist()
    n_cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    cell_start = None
    if 0 < n_cells <= int(table_cells):
        cell_start = torch.empty(n_cells + 1, **i32)
        ws = torch.empty(int(L.p2w_cell_starts_ws_bytes(n_cells)) + 256, dtype=torch.uint8, device=dev)
        check(L.p2w_cell_starts(ptr(skeys), n, n_cells, ptr(cell_start), ptr(ws), ws.numel(), _lib.stream()), "cell_starts")
        del ws
    mark()
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, **i32)
    pairs = torch.zeros(1, dtype=torch.int64, device=dev) if stats is not None else None
    ws = torch.empty(int(L.p2w_euclid_cluster_ws_bytes(n)), dtype=torch.uint8, device=dev)
    args = (ptr(cs), ptr(order), ptr(skeys), ptr(cell_start), ptr(grid), n, r, lo, hi)
    tail = (ptr(labels), ptr(counts), ptr(pairs), ptr(ws), ws.numel(), _lib.stream())
    if stats is None:
        check(L.p2w_euclid_cluster(*args, _lib.CLUSTER_ALL, *tail), "euclid_cluster")
    else:
        for st in (_lib.CLUSTER_LINK, _lib.CLUSTER_COMPRESS, _lib.CLUSTER_NUMBER):
            check(L.p2w_euclid_cluster(*args, st, *tail), "euclid_cluster")
            mark()
    nc, nn = counts.cpu().tolist()
    if stats is not None:
        ms = [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]
        stats.update(grid_ms=ms[0], link_ms=ms[1], compress_ms=ms[2], number_ms=ms[3], pairs=int(pairs.item()),
                     cell=float(cell), n_cells=n_cells, table=cell_start is not None, n_noise=nn)
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
        if isinstance(points, torch.Tensor):
            labels, _ = euclidean_cluster(points, self.cluster_tolerance, self.min_cluster_size, self.max_cluster_size)
            return labels
        a = np.asarray(points)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"points must be an [n, 3] array, got shape {a.shape}")
        if a.dtype != np.float32:
            a = a.astype(np.float64)
        if not np.isfinite(a).all():
            raise ValueError(_NONFINITE)
        t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        labels, _ = euclidean_cluster(t, self.cluster_tolerance, self.min_cluster_size, self.max_cluster_size)
        return labels.cpu().numpy()
