"""The plot-level cell grid of ``backproject.neighbours``, ``cluster.euclidean_cluster`` and ``pathlength.knn_rows``: float64
coordinates -> origin = per-axis minimum -> local coordinates rounded once to float32 -> ``p2w_voxel_sample`` on one voxel ->
``p2w_cell_starts``' table.  ``safe_cell`` and ``knn_slack`` are statements about this arithmetic, so they live beside it.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr

_EPS32 = 2.0 ** -23


def safe_cell(tolerance: float, extent: float) -> float:
    """Smallest grid cell (a float32 value) for which every pair the fp64 predicate joins lies in the same or adjacent cells.

    ``extent`` = the largest per-axis extent of the cloud, E.  The grid is built in fp32 by ``build``:
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


def knn_slack(extent: float) -> float:
    """How far the fp32 grid can misplace a point across a cell boundary of a cloud of largest per-axis extent ``extent`` (the
    error terms of ``safe_cell``: local coordinates and key division, each within 2^-23 E), with a factor 4 to spare."""
    return 8.0 * _EPS32 * extent + 1e-300


def records(loc: torch.Tensor) -> torch.Tensor:
    """[n, 4] float32 records (x, y, z, 0) of the coordinates ``loc`` [n, 3], each rounded once to float32."""
    rec = torch.zeros((loc.shape[0], 4), dtype=torch.float32, device=loc.device)
    rec[:, :3] = loc
    return rec


def local(x64: torch.Tensor):
    """(origin [3] float64 = the per-axis minimum, loc [n, 3] float64 = x64 - origin): the coordinates ``records`` rounds."""
    origin = torch.stack([x64[:, d].min() for d in range(3)])     # (a column reduction of [n, 3] runs on 3 outputs: 7 ms at 10^7)
    return origin, x64 - origin


def voxel_sample(rec: torch.Tensor, cell: float, *, order=None, keys=None, grid=None, inverse=None):
    """``p2w_voxel_sample`` over ``rec`` as one voxel: (idx [n] int32, ptr_out [2] int32: ptr_out[1] = occupied cells); the
    optional outputs are written into the caller's tensors.  The workspace is released on return."""
    L, n, dev = lib(), rec.shape[0], rec.device
    i32 = dict(dtype=torch.int32, device=dev)
    ptr_in = torch.tensor([0, n], **i32)
    idx, ptr_out, batch_out = torch.empty(n, **i32), torch.empty(2, **i32), torch.empty(n, **i32)
    ws = torch.empty(int(L.p2w_voxel_sample_ws_bytes(max(n, 1))), dtype=torch.uint8, device=dev)
    check(L.p2w_voxel_sample(ptr(rec), ptr(ptr_in), 1, n, float(cell), ptr(idx), ptr(ptr_out), ptr(batch_out), ptr(order),
                             ptr(keys), None, ptr(grid), ptr(inverse), None, ptr(ws), ws.numel(), _lib.stream()), "voxel_sample")
    return idx, ptr_out


@dataclasses.dataclass
class PlotGrid:
    cell: float                       # the float32 value the sampler divided by
    origin: torch.Tensor              # [3] float64: the per-axis minimum
    order: torch.Tensor               # [n] int32: sorted position -> point index
    keys: torch.Tensor                # [n] int64 ascending: (cz * dims[1] + cy) * dims[0] + cx
    grid: torch.Tensor                # [8] int64: the p2w_grid of the sampling call
    dims: tuple                       # (d0, d1, d2) on the host
    n_cells: int
    cell_start: torch.Tensor | None   # [n_cells + 1] int32: first sorted position of every cell; None = found by bisection
    xyz_sorted: torch.Tensor          # [n, 3] float64: the caller's coordinates in cell order
    records_sorted: torch.Tensor | None   # [n, 4] float32: the local records in cell order, w = the point's index
    occupied: torch.Tensor            # int32 scalar on the device: the number of occupied cells (reading it waits for the device)


def build(xyz: torch.Tensor, cell, table_cells: int, *, sorted_records: bool = False) -> PlotGrid:
    """The grid of the CUDA points ``xyz`` [n >= 1, 3] (float32 or float64, taken as float64).  ``cell``: the cell size, or a function
    of the float64 local coordinates [n, 3] that returns it (a size that follows the cloud's extent); ``table_cells``: largest grid
    whose cell table is built.  Waits for the device once, for the grid's size; every temporary is released before it returns."""
    L, n, dev = lib(), xyz.shape[0], xyz.device
    x64 = xyz.to(torch.float64)
    origin, loc = local(x64)
    if callable(cell):
        cell = cell(loc)
    rec = records(loc)
    del loc
    order, keys = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    grid = torch.zeros(8, dtype=torch.int64, device=dev)
    occupied = voxel_sample(rec, cell, order=order, keys=keys, grid=grid)[1][1]
    records_sorted = None
    if sorted_records:
        records_sorted = torch.empty((n, 4), dtype=torch.float32, device=dev)
        ptr_in = torch.tensor([0, n], dtype=torch.int32, device=dev)
        check(L.p2w_index_records(ptr(rec), ptr(order), ptr(ptr_in), 1, n, ptr(records_sorted), _lib.stream()), "index_records")
    del rec
    xyz_sorted = x64[order.long()].contiguous()
    del x64
    # cell -> first-point table (one load per run instead of a bisection of the keys); the grid's size is read back once - a
    # plot whose grid would not fit `table_cells` entries is searched by bisection
    dims = tuple(int(d) for d in grid.cpu()[4:7].tolist())
    n_cells = dims[0] * dims[1] * dims[2]
    cell_start = None
    if 0 < n_cells <= int(table_cells):
        cell_start = torch.empty(n_cells + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.p2w_cell_starts_ws_bytes(n_cells)) + 256, dtype=torch.uint8, device=dev)
        check(L.p2w_cell_starts(ptr(keys), n, n_cells, ptr(cell_start), ptr(ws), ws.numel(), _lib.stream()), "cell_starts")
    return PlotGrid(float(np.float32(cell)), origin, order, keys, grid, dims, n_cells, cell_start, xyz_sorted, records_sorted, occupied)
