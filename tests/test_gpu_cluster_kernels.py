"""p2w_euclid_cluster (csrc/p2w_cluster.hip) on the MI355X through the C ABI, on device copies of the grid that the plain reference
tests/cluster_ref.py builds - not through plotgrid.build - for every named case of that file (tests/test_cluster_ref_cpu.py pins
the reference to the recorded fixtures and to scipy, and asserts that every case meets the condition it is named for and which
wrong kernel it catches).  Labels, counts and pair counts are integers: every comparison is exact.  The last two tests tie the
hand-built grid to the one the product builds, and the host layer to the same answers."""
import numpy as np
import pytest
import torch

from pointstowood_amd import _lib, plotgrid
from pointstowood_amd.cluster import euclidean_cluster
from tests import cluster_ref as R

pytestmark = pytest.mark.gpu

ALL = sorted(R.CASES)
SAFE_CELL = [name for name in ALL if R.CASES[name]()[4] is None]             # the cases that leave the cell to the host layer
PROTOCOL = ["stencil_+1-1+1_in_rev_near", "interleaved_lines", "n4097_kept_roots_both_sides", "line_shuffled", "one_cell"]
IN_ORDER = (_lib.CLUSTER_LINK, _lib.CLUSTER_COMPRESS, _lib.CLUSTER_NUMBER)
SENTINEL = -0x0123456789ABCDEF


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda().contiguous()


_inputs = {}


def _device_inputs(name):
    """The reference's grid of the case on the device: (xyz_sorted, order, keys_sorted, cell_start, p2w_grid)."""
    if name not in _inputs:
        g = R.solved(name).grid
        _inputs[name] = (_dev(g.xyz_sorted), _dev(g.order), _dev(g.keys_sorted.view(np.int64)), _dev(g.cell_start), _dev(g.image.view(np.int64)))
    return _inputs[name]


def _cluster(name, stages=(_lib.CLUSTER_ALL,), table=True, with_pairs=True, garbage=False, bounds=None):
    """(labels [n] int64, [n_kept, n_noise], pairs or None) of one or several calls on one workspace of exactly the stated size."""
    L, s = _lib.lib(), R.solved(name)
    xs, order, keys, cell_start, grid = _device_inputs(name)
    n = len(s.xyz)
    mn, mx = (s.min_size, s.max_size) if bounds is None else bounds
    labels = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    pairs = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(int(L.p2w_euclid_cluster_ws_bytes(n)), dtype=torch.uint8, device="cuda")
    if garbage:
        for t in (labels, counts, pairs, ws):
            t.view(torch.uint8).fill_(0xFF)
    for st in stages:
        code = L.p2w_euclid_cluster(xs.data_ptr(), order.data_ptr(), keys.data_ptr(), cell_start.data_ptr() if table else None, grid.data_ptr(),
                                    n, s.r, mn, mx, st, labels.data_ptr(), counts.data_ptr(), pairs.data_ptr() if with_pairs else None,
                                    ws.data_ptr(), ws.numel(), _lib.stream())
        assert code == 0, (name, st, code)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), counts.cpu().tolist(), int(pairs.item()) if with_pairs else None


def _assert_answers(name, got):
    s = R.solved(name)
    labels, counts, pairs = got
    assert np.array_equal(labels, s.labels), name
    assert counts == [s.n_kept, s.n_noise], name
    assert pairs is None or pairs == s.pairs, name


@pytest.mark.parametrize("name", ALL)
def test_labels_counts_and_pairs_equal_the_reference(name):
    """P2W_CLUSTER_ALL with the cell table.  pairs_out is the number of unordered pairs of points in equal or adjacent cells: a
    stencil that misses a neighbour cell, measures one twice or runs past a face gives another number even where the labels agree."""
    _assert_answers(name, _cluster(name))


@pytest.mark.parametrize("name", PROTOCOL)
def test_stages_one_at_a_time_equal_all(name):
    _assert_answers(name, _cluster(name, stages=IN_ORDER))


@pytest.mark.parametrize("name", PROTOCOL)
def test_bisection_of_the_keys_equals_the_table(name):
    _assert_answers(name, _cluster(name, table=False))
    _assert_answers(name, _cluster(name, stages=IN_ORDER, table=False))


@pytest.mark.parametrize("name", PROTOCOL)
def test_second_call_gives_the_same_bits(name):
    a, b = _cluster(name), _cluster(name)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


@pytest.mark.parametrize("name", PROTOCOL)
def test_garbage_in_the_workspace_and_the_outputs_changes_nothing(name):
    """Every byte of the workspace and of the three outputs is 0xFF before the call: the entry point initialises what it reads."""
    _assert_answers(name, _cluster(name, garbage=True))
    _assert_answers(name, _cluster(name, stages=IN_ORDER, table=False, garbage=True))


@pytest.mark.parametrize("name", PROTOCOL)
def test_pairs_out_may_be_null(name):
    _assert_answers(name, _cluster(name, with_pairs=False))
    _assert_answers(name, _cluster(name, stages=IN_ORDER, with_pairs=False))


def test_no_points_write_zero_counts_and_leave_the_labels_alone():
    L = _lib.lib()
    xs, order, keys, cell_start, grid = _device_inputs("n_1")
    labels = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
    ws = torch.zeros(max(int(L.p2w_euclid_cluster_ws_bytes(0)), 16), dtype=torch.uint8, device="cuda")
    for stages in ((_lib.CLUSTER_ALL,), IN_ORDER):
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        pairs = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        for st in stages:
            assert L.p2w_euclid_cluster(xs.data_ptr(), order.data_ptr(), keys.data_ptr(), cell_start.data_ptr(), grid.data_ptr(), 0, 0.1, 1, R.BIG,
                                        st, labels.data_ptr(), counts.data_ptr(), pairs.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()) == 0
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == [0, 0] and int(pairs.item()) == 0
        assert labels.cpu().tolist() == [SENTINEL] * 4


@pytest.mark.parametrize("bounds,want", [((1, R.BIG), 0), ((0, 1), 0), ((1, 1), 0), ((2, R.BIG), -1), ((0, 0), -1), ((2, 1), -1)])
def test_one_point_is_a_cluster_where_the_bounds_admit_one(bounds, want):
    labels, counts, pairs = _cluster("n_1", bounds=bounds)
    assert labels.tolist() == [want] and counts == ([1, 0] if want == 0 else [0, 1]) and pairs == 0


@pytest.mark.parametrize("name", SAFE_CELL)
def test_host_layer_gives_the_reference_labels(name):
    s = R.solved(name)
    labels, n_kept = euclidean_cluster(_dev(s.xyz), s.r, s.min_size, s.max_size)
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), s.labels) and n_kept == s.n_kept


@pytest.mark.parametrize("name", SAFE_CELL)
def test_product_grid_equals_the_reference_grid_bit_for_bit(name):
    s = R.solved(name)
    g = s.grid
    G = plotgrid.build(_dev(s.xyz), g.cell, 1 << 30)
    assert G.cell == g.cell and G.dims == tuple(int(d) for d in g.dims) and G.n_cells == g.n_cells
    assert np.array_equal(G.keys.cpu().numpy(), g.keys_sorted.view(np.int64))
    assert np.array_equal(G.order.cpu().numpy(), g.order)
    assert G.cell_start is not None and np.array_equal(G.cell_start.cpu().numpy(), g.cell_start)
    assert np.array_equal(G.xyz_sorted.cpu().numpy().view(np.uint64), g.xyz_sorted.view(np.uint64))
    assert np.array_equal(G.grid.cpu().numpy().view(np.uint8)[:56], g.image)
    assert np.array_equal(G.origin.cpu().numpy(), g.origin)
