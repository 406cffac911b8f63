"""p2w_knn_refine_f64, p2w_vote and p2w_morton_order on the MI355X, each called alone through the C ABI, against the plain reference
tests/backproject_ref.py (held to oracle/backproject.py and scipy's KD-tree by tests/test_backproject_ref_cpu.py, which also asserts
that every case below meets the condition it is named for).  Every comparison is exact: indices and counts equal, pwood bit for bit;
no query and no row is left out."""
import numpy as np
import pytest
import torch

from pointstowood_amd import _lib, plotgrid
from tests import backproject_ref as R

pytestmark = pytest.mark.gpu

P2W_EWORKSPACE = -4


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))                                # (a copy: the cached cases are read-only)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


# ---- p2w_knn_refine_f64 -----------------------------------------------------------------------------------------------------------------

class _Grid:
    """The candidates on their plot-level grid, as backproject.neighbours forms it."""
    def __init__(self, cand, cell=R.CELL):
        self.nc = len(cand)
        self.g = plotgrid.build(_dev(cand), cell, 1 << 30, sorted_records=True)
        self.pos_of = torch.empty(self.nc, dtype=torch.int32, device="cuda")
        self.pos_of[self.g.order.long()] = torch.arange(self.nc, dtype=torch.int32, device="cuda")
        self.origin = self.g.origin.cpu().tolist()
        assert self.g.cell_start is not None

    def refine(self, q, rows, deg, k, table=True):
        """(nbr [m, k], deg [m]) after the call; ``rows`` [m, k] and ``deg`` [m] are its input."""
        g, m = self.g, len(q)
        nbr, dg, qd = _dev(rows, torch.int32), _dev(deg, torch.int32), _dev(q, torch.float64)
        assert nbr.shape == (m, k) and qd.shape == (m, 3)
        _lib.check(_lib.lib().p2w_knn_refine_f64(_lib.ptr(g.xyz_sorted), _lib.ptr(g.order), _lib.ptr(self.pos_of), _lib.ptr(g.keys),
                                                 _lib.ptr(g.cell_start) if table else None, _lib.ptr(g.grid), *self.origin, _lib.ptr(qd),
                                                 m, self.nc, k, _lib.ptr(nbr), _lib.ptr(dg), _lib.stream()), "knn_refine_f64")
        return nbr.cpu().numpy(), dg.cpu().numpy()

    def both(self, q, rows, deg, k):
        """The call through the cell table; the bisection (cell_start = NULL) must give the same bytes."""
        a, b = self.refine(q, rows, deg, k), self.refine(q, rows, deg, k, table=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        return a


_grids = {}


def _grid(name):
    if name not in _grids:
        cand = {"uniform": lambda: R.uniform_ranked()[0], "shifted": lambda: R.uniform_ranked(True)[0],
                "ties": lambda: R.tie_cloud()[0]}[name]()
        _grids[name] = _Grid(cand)
    return _grids[name]


def test_a_ball_over_the_box_takes_several_row_batches_and_chunks():
    """What the t = nc cases rest on, from the grid itself: the scan of a ball that covers the box walks dims[1] * dims[2] rows in
    batches of 64, and the candidates of a batch are staged 256 positions at a time."""
    for name in ("uniform", "shifted"):
        G = _grid(name)
        d0, d1, d2 = G.g.dims
        assert d1 * d2 > 64 and G.nc > 256
        keys = G.g.keys.cpu().numpy()
        assert keys.min() >= 0 and keys.max() < d0 * d1 * d2
        per_batch = np.bincount((keys // d0) // 64)
        assert len(per_batch) > 2 and per_batch.max() > 256              # more than one batch, more than one chunk in a batch
        order = G.g.order.cpu().numpy()
        assert sorted(order.tolist()) == list(range(G.nc)) and (order != np.arange(G.nc)).mean() > 0.9   # a shuffled cand_index


@pytest.mark.parametrize("k,t", R.REFINE_TARGETS)
@pytest.mark.parametrize("name", ["uniform", "shifted"])
def test_refine_from_a_subset_of_the_t_nearest(name, k, t):
    """T = t candidates lie within the bound of the row handed in (a random k of the t nearest, the t-th among them): t <= 128 ranks
    a list, t >= 129 extracts the k smallest one by one, t = nc scans every row of the grid.  203 queries in, around and on the cell
    boundaries of the box; with the survey offset the reference ranks the shifted float64 values.  (Both paths are exact, so a
    kernel that sent T = 128 to the extraction would pass unseen, only slower; one that ranked a list of 129 would lose a candidate.)"""
    cand, q, d2, full = R.uniform_ranked(name == "shifted")
    rows = R.rows_for_target(full, k, t, seed=t)
    nbr, deg = _grid(name).both(q, rows, np.full(R.M, k), k)
    assert np.array_equal(deg, np.full(R.M, k))
    assert np.array_equal(nbr, full[:, :k])


@pytest.mark.parametrize("name", ["uniform", "shifted"])
def test_refine_from_the_k_farthest(name):
    """The largest bound there is: the answer does not depend on which candidates were handed in."""
    cand, q, d2, full = R.uniform_ranked(name == "shifted")
    nbr, deg = _grid(name).both(q, R.farthest_rows(full, 64, seed=5), np.full(R.M, 64), 64)
    assert np.array_equal(deg, np.full(R.M, 64)) and np.array_equal(nbr, full[:, :64])


@pytest.mark.parametrize("k", R.TIE_KS)
def test_refine_breaks_ties_by_the_reported_index(k):
    """Bit-equal d2 across the k-th place (two distinct points) and piles of 128 / 129 coincident points, each through the list
    (T <= 128) and through the extraction: the lower indices win, in index order - the indices the result reports (cand_index is
    the grid's own shuffled order), not the sorted positions."""
    cand, members = R.tie_cloud()
    q, rows, T = R.tie_case(k)
    nbr, deg = _grid("ties").both(q, rows, np.full(len(q), k), k)
    want = R.refine(cand, q, k)
    assert np.array_equal(deg, np.full(len(q), k))
    assert np.array_equal(nbr, want)
    assert np.array_equal(nbr[2], members["pile128"][:k]) and np.array_equal(nbr[3], members["pile129"][:k])


@pytest.mark.parametrize("nc", [1, 20])
def test_refine_with_fewer_candidates_than_k(nc):
    """deg = nc < k: all candidates ascending by (d2, index), the slots behind them and deg untouched."""
    cand, q, rows, deg_in = R.few_cloud(nc)
    nbr, deg = _Grid(cand).both(q, rows, deg_in, 64)
    assert np.array_equal(deg, deg_in)
    assert np.array_equal(nbr[:, :nc], R.refine(cand, q, 64))
    assert (nbr[:, nc:] == R.SENTINEL).all()


def test_refine_leaves_empty_rows_alone():
    """Rows with deg = 0 between full rows (the waves of a workgroup part ways): sentinel and deg kept."""
    cand, q, d2, full = R.uniform_ranked()
    k = 32
    rows = R.rows_for_target(full, k, 40, seed=9)
    deg_in = np.full(R.M, k, dtype=np.int32)
    empty = np.arange(R.M) % 3 == 1
    empty[-3:] = True
    rows[empty], deg_in[empty] = R.SENTINEL, 0
    nbr, deg = _grid("uniform").both(q, rows, deg_in, k)
    assert np.array_equal(deg, deg_in)
    assert (nbr[empty] == R.SENTINEL).all() and np.array_equal(nbr[~empty], full[~empty, :k])


# ---- p2w_vote ---------------------------------------------------------------------------------------------------------------------------

def _vote(nbr, deg, k, pred, prob, any_wood):
    n = len(deg)
    nb, dg, pd, pr = _dev(nbr, torch.int32), _dev(deg, torch.int32), _dev(pred, torch.float32), _dev(prob, torch.float32)
    assert nb.shape == (n, k)
    lab = torch.full((n,), float(R.SENTINEL), dtype=torch.float32, device="cuda")
    pw = torch.full_like(lab, float(R.SENTINEL))
    _lib.check(_lib.lib().p2w_vote(_lib.ptr(nb), _lib.ptr(dg), k, _lib.ptr(pd), _lib.ptr(pr), n, float(any_wood), _lib.ptr(lab),
                                   _lib.ptr(pw), _lib.stream()), "vote")
    return lab.cpu().numpy(), pw.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("k", R.VOTE_KS)
def test_vote_over_every_count(k):
    """Row counts 1, 3, 4, 5, 257 (whole and partly empty workgroups), deg over 0 .. k and one above k, repeated probabilities, the
    four any_wood settings; the slots from deg[i] on hold -1, nc + 7 and INT_MAX, which the call must not follow.  Median: an odd
    count's middle value, an even count's (a + b) / 2 in one fp32 rounding; no valid slot: (0, 0)."""
    for n in R.VOTE_NS:
        for variant in range(5 if n < 5 else 1):
            nbr, deg = R.vote_case(n, k, variant)
            for any_wood in R.VOTE_ANY_WOOD:
                pred, prob = R.vote_table(rare=any_wood != 1)
                label, pwood, undecided = R.vote(nbr, deg, k, pred, prob, any_wood)
                assert not undecided.any()                               # a condition of the input, not a filter
                lab, pw = _vote(nbr, deg, k, pred, prob, any_wood)
                assert np.array_equal(lab, label), (n, variant, any_wood)
                assert _same_bits(pw, pwood), (n, variant, any_wood)


@pytest.mark.parametrize("k", R.VOTE_PLANTED_KS)
def test_vote_on_planted_rows(k):
    """any_wood = 1: v1 == v0 exactly -> 0 (argmax keeps the first maximum), 2^-10 more on either side -> 1 / 0.  any_wood = 0.5: the
    only wood neighbour in the last valid slot counts, in slot deg[i] it does not."""
    for nbr, deg, pred, prob, any_wood, want in R.vote_planted(k):
        label, pwood, undecided = R.vote(nbr, deg, k, pred, prob, any_wood)
        assert not undecided.any() and np.array_equal(label, want)
        lab, pw = _vote(nbr, deg, k, pred, prob, any_wood)
        assert np.array_equal(lab, want), any_wood
        assert _same_bits(pw, pwood), any_wood


# ---- p2w_morton_order -------------------------------------------------------------------------------------------------------------------

def _grid_struct(lo, res):
    """A p2w_grid on the device (include/p2w.h): float lo[3], res, hi[3]; int32 b_lo; int64 dims[3].  The call reads lo and res."""
    g = np.zeros(1, dtype=np.dtype([("lo", "<f4", 3), ("res", "<f4"), ("hi", "<f4", 3), ("b_lo", "<i4"), ("dims", "<i8", 3)]))
    assert g.dtype.itemsize == 56
    g["lo"], g["res"], g["hi"], g["dims"] = lo, res, np.asarray(lo) + 2.0, 1
    return _dev(np.frombuffer(g.tobytes() + bytes(8), dtype=np.int64))


def _morton(rec, grid, n, ws, ws_bytes):
    out = torch.full((max(n, 1),), R.SENTINEL, dtype=torch.int32, device="cuda")
    st = _lib.lib().p2w_morton_order(_lib.ptr(rec), n, _lib.ptr(grid), _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream())
    return st, out.cpu().numpy()


@pytest.mark.parametrize("beyond", [False, True])
@pytest.mark.parametrize("res", R.MORTON_RES)
@pytest.mark.parametrize("n", R.MORTON_NS)
def test_morton_order_is_the_stable_argsort_of_the_keys(n, res, beyond):
    """Records below lo (cell 0), beyond 2^21 cells (clamped), with NaN coordinates (cell 0) and long runs of one cell (input order
    kept); cell sizes whose widest key has 3, 5 and 8 bytes - the radix sort's passes - and 2^-20 m, where all 21 bits of an axis
    are in use.  The workspace's content does not matter; one that is too small is refused before anything is written."""
    rec = R.morton_records(n, beyond)
    want = R.morton(rec[:, :3], R.MORTON_LO, res)[1]
    need = int(_lib.lib().p2w_morton_order_ws_bytes(n))
    recd, grid = _dev(rec), _grid_struct(R.MORTON_LO, res)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st, got = _morton(recd, grid, n, ws, need)
    assert st == 0
    assert sorted(got.tolist()) == list(range(n))
    assert np.array_equal(got, want)
    ws.fill_(0xff)
    st, again = _morton(recd, grid, n, ws, need)
    assert st == 0 and np.array_equal(again, got)
    st, untouched = _morton(recd, grid, n, ws, need - 1)
    assert st == P2W_EWORKSPACE and (untouched == R.SENTINEL).all()
