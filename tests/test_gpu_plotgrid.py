"""The plot-level cell grid (pointstowood_amd.plotgrid.build) on the MI355X: what the back-projection, the clustering and the path
length's kNN assume about it, and the documented arithmetic of its keys (the one ``safe_cell`` and ``knn_slack`` reason about)."""
import numpy as np
import pytest
import torch

from pointstowood_amd import plotgrid
from tests.test_gpu_cluster import _clustered_cloud

pytestmark = pytest.mark.gpu

EASTING = (512345.25, 6012345.5, 80.0)          # a plot in projected coordinates: the offset is far beyond fp32's resolution


def _host_keys(xyz, cell):
    """(key of every point, dims) by the construction's arithmetic: u = fl32(x - min x) in fp64 first, key_d = trunc(fl32(u / res))
    with res = fl32(cell) and the grid origin min u = 0, dims_d = trunc(fl32(max u / res)) + 1, key = (kz * d1 + ky) * d0 + kx."""
    u = (xyz - xyz.min(axis=0)).astype(np.float32)
    res = np.float32(cell)
    assert u.dtype == np.float32 and (u.min(axis=0) == 0).all()
    k = (u / res).astype(np.int64)
    dims = ((u.max(axis=0) / res).astype(np.int64) + 1).tolist()
    return (k[:, 2] * dims[1] + k[:, 1]) * dims[0] + k[:, 0], dims


def _check_grid(g, x64):
    n = x64.shape[0]
    assert g.order.shape == (n,) and g.keys.shape == (n,) and g.order.dtype == torch.int32 and g.keys.dtype == torch.int64 and g.grid.shape == (8,)
    assert bool((g.keys[1:] >= g.keys[:-1]).all()) and int(g.keys[0]) >= 0
    assert torch.equal(torch.sort(g.order.long()).values, torch.arange(n, device=x64.device))
    assert torch.equal(g.origin, x64.min(dim=0).values)
    assert g.dims == tuple(g.grid.cpu()[4:7].tolist()) and g.n_cells == g.dims[0] * g.dims[1] * g.dims[2]
    assert int(g.keys[-1]) < g.n_cells
    assert g.occupied.is_cuda and int(g.occupied) == int(torch.unique(g.keys).numel())


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), EASTING])
def test_build_sorts_the_cloud_into_cells(offset):
    xyz = _clustered_cloud(200_000, 0, offset)
    x64 = torch.from_numpy(xyz).cuda()
    cell = 0.25
    g = plotgrid.build(x64, cell, 1 << 30, sorted_records=True)
    _check_grid(g, x64)
    assert g.cell == float(np.float32(cell))
    order = g.order.long()
    assert torch.equal(g.xyz_sorted, x64[order])
    want, dims = _host_keys(xyz, cell)
    assert list(g.dims) == dims
    assert np.array_equal(g.keys.cpu().numpy(), want[order.cpu().numpy()])
    assert g.cell_start is not None and g.cell_start.dtype == torch.int32 and g.cell_start.shape == (g.n_cells + 1,)
    cells = torch.arange(g.n_cells + 1, device=x64.device)
    assert torch.equal(g.cell_start.long(), torch.searchsorted(g.keys, cells))
    u = (x64 - g.origin).to(torch.float32)
    assert torch.equal(g.records_sorted[:, :3], u[order])
    assert torch.equal(g.records_sorted[:, 3].contiguous().view(torch.int32), g.order)


def test_records_are_produced_on_request_only_and_large_grids_get_no_table():
    x64 = torch.from_numpy(_clustered_cloud(120_000, 0)).cuda()
    full = plotgrid.build(x64, 0.5, 1 << 30)
    assert full.records_sorted is None and full.cell_start is not None
    for table_cells in (0, 1, full.n_cells - 1):
        g = plotgrid.build(x64, 0.5, table_cells)
        _check_grid(g, x64)
        assert g.cell_start is None and g.records_sorted is None
        assert torch.equal(g.keys, full.keys) and torch.equal(g.order, full.order) and torch.equal(g.grid, full.grid)
    g = plotgrid.build(x64, 0.5, full.n_cells)
    assert torch.equal(g.cell_start, full.cell_start)


def test_cell_from_the_local_coordinates_and_float32_input():
    xyz = _clustered_cloud(100_000, 3, EASTING)
    x64 = torch.from_numpy(xyz).cuda()
    seen = {}

    def cell(loc):
        seen["loc"] = loc.clone()
        return plotgrid.safe_cell(0.1, float(loc.max()))

    g = plotgrid.build(x64, cell, 1 << 30)
    assert torch.equal(seen["loc"], x64 - x64.min(dim=0).values)
    extent = float((xyz - xyz.min(axis=0)).max())
    assert g.cell == plotgrid.safe_cell(0.1, extent)
    assert torch.equal(g.keys, plotgrid.build(x64, plotgrid.safe_cell(0.1, extent), 1 << 30).keys)
    x32 = x64.to(torch.float32)                  # a float32 cloud is gridded on its float64 values
    a, b = plotgrid.build(x32, 0.3, 1 << 30), plotgrid.build(x32.to(torch.float64), 0.3, 1 << 30)
    assert torch.equal(a.keys, b.keys) and torch.equal(a.order, b.order) and torch.equal(a.xyz_sorted, b.xyz_sorted)
    assert a.xyz_sorted.dtype == torch.float64
