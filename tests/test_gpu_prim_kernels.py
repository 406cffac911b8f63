"""The device-wide primitives under every geometry path - the radix sort and the exclusive scan of csrc/p2w_sort.h, p2w_key_runs,
p2w_cell_starts and p2w_cells_nd of csrc/p2w_geom.hip - on the MI355X through the C ABI, on device copies of what the plain reference
tests/prim_ref.py builds, for every named case of that file (tests/test_prim_ref_cpu.py ties the reference to independent restatements
and asserts that every case meets the condition it is named for and which wrong kernel it catches).  Everything is integers: every
comparison is exact.  Every output lies between guard elements and is filled with a sentinel before the call, every workspace with
0xFF; inputs are compared with their host copies afterwards.  Sorted key arrays are handed over with copies of their first and last
key in front of and behind them, so a kernel that looks at keys[-1] or keys[n] merges a run instead of meeting a lucky value."""
import time

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import prim_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                                                 # elements in front of and behind every output
S32, S64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


class _Out:
    """n elements between two guards, all filled with the sentinel; ptr = the first element behind the front guard (16-byte aligned)."""

    def __init__(self, n, dtype):
        self.n, self.fill = n, S32 if dtype == torch.int32 else S64
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())


def _sorted_keys(keys):
    """(tensor, pointer to key 0): two copies of the first key in front, two of the last behind."""
    if keys is None:
        return None, None
    t = _dev(np.concatenate([keys[:1], keys[:1], keys, keys[-1:], keys[-1:]]))
    return t, t.data_ptr() + 16


def _ws(nbytes, slack=0):
    return torch.full((int(nbytes) + slack,), 0xFF, dtype=torch.uint8, device="cuda")


def _same(t, a):
    a = np.ascontiguousarray(a)
    return np.array_equal(t.cpu().numpy(), a.view(np.int64) if a.dtype == np.uint64 else a)


# ---- p2w_sort_pairs_u64 ---------------------------------------------------------------------------------------------------------------------

def _sort(L, c, ws):
    dk, dv = _dev(c.keys), None if c.vals is None else _dev(c.vals)
    ko, vo = _Out(c.n, torch.int64), _Out(c.n, torch.int32)
    code = L.p2w_sort_pairs_u64(dk.data_ptr(), ko.ptr, None if dv is None else dv.data_ptr(), vo.ptr, c.n, ws.data_ptr(),
                                int(L.p2w_sort_pairs_u64_ws_bytes(c.n)), _lib.stream())
    assert code == 0
    torch.cuda.synchronize()
    assert _same(dk, c.keys) and (dv is None or _same(dv, c.vals))         # inputs unmodified
    assert ko.guards_intact() and vo.guards_intact()                       # nothing behind n, nothing in front
    return ko.body().cpu().numpy().view(np.uint64), vo.body().cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.SORT_CASES))
def test_sort_pairs_is_the_stable_unsigned_sort(name):
    """keys_out / vals_out equal np.argsort(kind="stable") on uint64, inputs and guards untouched, on a workspace of 0xFF; the same
    call again on the same workspace, with another case of the same size sorted in between, gives the same bits."""
    L, c = _lib.lib(), R.sort_case(name)
    other = R.sort_case(next(k for k, v in sorted(R.SORT_CASES.items()) if v[1] == c.n and v[0] != c.family))
    ws = _ws(L.p2w_sort_pairs_u64_ws_bytes(c.n))
    want_k, want_v = R.sort_pairs(c.keys, c.vals)
    got_k, got_v = _sort(L, c, ws)
    assert np.array_equal(got_k, want_k)
    assert np.array_equal(got_v, want_v)
    ok, ov = _sort(L, other, ws)
    wk, wv = R.sort_pairs(other.keys, other.vals)
    assert np.array_equal(ok, wk) and np.array_equal(ov, wv)
    again_k, again_v = _sort(L, c, ws)
    assert np.array_equal(again_k, got_k) and np.array_equal(again_v, got_v)


# ---- p2w_key_runs ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.RUN_CASES))
def test_key_runs_keeps_the_runs_of_at_least_min_count(name):
    """*n_out, starts_out[:k] and counts_out[:k] equal the reference; the entries from k on and the guards still hold the sentinel."""
    L, c = _lib.lib(), R.run_case(name)
    n = len(c.keys)
    want_s, want_c = R.key_runs(c.keys, c.min_count)
    keys, kp = _sorted_keys(c.keys)
    so, co, no = _Out(n, torch.int32), _Out(n, torch.int32), _Out(1, torch.int32)
    need = int(L.p2w_key_runs_ws_bytes(n))
    ws = _ws(need)
    assert L.p2w_key_runs(kp, n, c.min_count, so.ptr, co.ptr, no.ptr, ws.data_ptr(), need, _lib.stream()) == 0
    torch.cuda.synchronize()
    k = int(no.body()[0])
    assert k == len(want_s)
    assert np.array_equal(so.body()[:k].cpu().numpy(), want_s) and np.array_equal(co.body()[:k].cpu().numpy(), want_c)
    assert bool((so.body()[k:] == S32).all()) and bool((co.body()[k:] == S32).all())
    assert so.guards_intact() and co.guards_intact() and no.guards_intact()
    assert _same(keys[2:2 + n], c.keys)


def test_key_runs_of_no_keys_writes_a_zero_count():
    L = _lib.lib()
    no = _Out(1, torch.int32)
    assert L.p2w_key_runs(None, 0, 1, None, None, no.ptr, None, 0, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert int(no.body()[0]) == 0 and no.guards_intact()


# ---- p2w_cell_starts (the exclusive scan behind it) -------------------------------------------------------------------------------------------

def _cell_starts(L, c):
    keys, kp = _sorted_keys(c.keys)
    table = _Out(c.n_cells + 1, torch.int32)
    need = int(L.p2w_cell_starts_ws_bytes(c.n_cells))
    ws = _ws(need)
    n = 0 if c.keys is None else len(c.keys)
    assert L.p2w_cell_starts(kp, n, c.n_cells, table.ptr, ws.data_ptr(), need, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert c.keys is None or _same(keys[2:2 + n], c.keys)
    return table


@pytest.mark.parametrize("name", [t for t in R.TABLE_CASES if t != "deep"])
def test_cell_starts_counts_the_keys_below_every_cell(name):
    """table[c] = number of keys below c for c = 0 .. n_cells, the guard behind entry n_cells untouched."""
    c = R.table_case(name)
    table = _cell_starts(_lib.lib(), c)
    assert np.array_equal(table.body().cpu().numpy(), R.table_expected(name))
    assert table.guards_intact()


def test_cell_starts_of_the_deep_table_carries_between_scan_rounds():
    """8192 * 4096 + 1 entries: 8193 scan tiles, so the one workgroup over the tile sums takes a second round of 8192 and carries the
    first round's total into it - the only size at which that loop runs twice.  Expected table built on the host, compared on the
    device."""
    c, want = R.table_case("deep"), R.table_expected("deep")
    t0 = time.perf_counter()
    table = _cell_starts(_lib.lib(), c)
    t1 = time.perf_counter()
    assert torch.equal(table.body(), torch.from_numpy(want).cuda())
    assert table.guards_intact()
    print(f"deep table: call + sync {t1 - t0:.3f} s, compare {time.perf_counter() - t1:.3f} s")


# ---- p2w_cells_nd ---------------------------------------------------------------------------------------------------------------------------

def _cells(L, c):
    P = _dev(c.P)
    out = _Out(c.n, torch.int64)
    ws = _ws(256, slack=256)                                               # 256 bytes are the workspace, 256 more watch what lies behind
    assert L.p2w_cells_nd(P.data_ptr(), c.n, c.D, c.ld, c.size, out.ptr, ws.data_ptr(), 256, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((ws[256:] == 0xFF).all()) and out.guards_intact()
    assert np.array_equal(P.cpu().numpy().view(np.int32), c.P.view(np.int32))
    return out.body()


@pytest.mark.parametrize("name", R.CELLS_CASES)
def test_cells_nd_is_the_float32_quotient_of_columns_0_to_D(name):
    """cell_out equals the reference of individually rounded float32 operations, with the pitch and the NaN pad columns as built, on a
    workspace of exactly 256 bytes."""
    c = R.cells_case(name)
    got = _cells(_lib.lib(), c).cpu().numpy()
    assert np.array_equal(got, R.cells_nd(c.P, c.D, c.ld, c.size))


@pytest.mark.parametrize("name,size,min_pts", [("planted_0.04", None, 2), ("nonfinite_rows_1e30", 3.0, 2)])
def test_the_voxelisers_chain_equals_the_tensor_restatement(name, size, min_pts):
    """p2w_cells_nd -> p2w_sort_pairs_u64 as an argsort -> gather -> p2w_key_runs == oracle.preprocess.TensorBackend.grid_segments, on
    the planted case and on the table with non-finite rows at a cell size that puts several rows into a cell."""
    from oracle import preprocess as OP
    L, c = _lib.lib(), R.cells_case(name)
    c = c if size is None else c._replace(size=size)
    n = c.n
    order_ref, starts_ref, counts_ref = OP.TensorBackend.grid_segments(torch.from_numpy(c.P[:, :c.D].copy()), c.size, min_pts)
    per_cell = np.unique(R.cells_nd(c.P, c.D, c.ld, c.size), return_counts=True)[1]
    assert len(starts_ref) > 3 and per_cell.min() < min_pts < per_cell.max()   # some runs dropped, some kept, none at random
    cell = _cells(L, c)
    ks, order = _Out(n, torch.int64), _Out(n, torch.int32)
    ws = _ws(max(L.p2w_sort_pairs_u64_ws_bytes(n), L.p2w_key_runs_ws_bytes(n)))
    assert L.p2w_sort_pairs_u64(cell.data_ptr(), ks.ptr, None, order.ptr, n, ws.data_ptr(), ws.numel(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(order.body().cpu().long(), order_ref)               # (before it is followed as an index)
    gathered = cell[order.body().long()]
    assert torch.equal(gathered, ks.body())
    so, co, no = _Out(n, torch.int32), _Out(n, torch.int32), _Out(1, torch.int32)
    assert L.p2w_key_runs(gathered.data_ptr(), n, min_pts, so.ptr, co.ptr, no.ptr, ws.data_ptr(), ws.numel(), _lib.stream()) == 0
    torch.cuda.synchronize()
    k = int(no.body()[0])
    starts, counts = so.body()[:k].cpu().long(), co.body()[:k].cpu().long()
    if k and int(gathered[starts[-1]]) == R.CELL_NONFINITE:                # rows with a non-finite value belong to no voxel
        assert name.startswith("nonfinite")
        starts, counts = starts[:-1], counts[:-1]
    assert torch.equal(order.body().cpu().long(), order_ref) and torch.equal(starts, starts_ref) and torch.equal(counts, counts_ref)
    assert ks.guards_intact() and order.guards_intact() and so.guards_intact() and co.guards_intact()


# ---- the sort and the cell table feeding run_sum: p2w_interp_bwd over slot lists no kNN produces ------------------------------------------------

@pytest.mark.parametrize("name", R.INTERP_CASES)
def test_interp_bwd_over_hand_made_slot_tables(name):
    """|grad_x - float64 scatter-add| <= (L_j + 8) 2^-23 sum |a| |g| per element (the bound tests/test_gpu_ops_backward.py derives: L_j
    fp32 additions of the run's products, 8 for the fp32 weights); rows nobody references are exactly 0.  A slot counts when it lies
    below min(deg, kw) and its index lies in 0 .. n_coarse - 1."""
    L, c = _lib.lib(), R.interp_case(name)
    (m, kw), nc, F = c.nbr.shape, len(c.xyzr_c), c.g.shape[1]
    g, rc, rf, nbr, deg = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.g, c.xyzr_c, c.xyzr_f, c.nbr, c.deg))
    gx = torch.full((nc + 1, F), float("nan"), dtype=torch.float32, device="cuda")
    need = int(L.p2w_interp_bwd_ws_bytes(m, kw, nc))
    ws = _ws(need)
    assert need > 0 and L.p2w_interp_bwd(g.data_ptr(), F, F, rc.data_ptr(), rf.data_ptr(), nbr.data_ptr(), deg.data_ptr(), kw, m, nc,
                                         gx.data_ptr(), F, ws.data_ptr(), need, _lib.stream()) == 0
    torch.cuda.synchronize()
    got = gx.cpu().numpy().astype(np.float64)
    assert np.isnan(got[nc]).all() and np.isfinite(got[:nc]).all()         # every row written, none behind n_coarse
    err = np.abs(got[:nc] - c.ref)
    print(f"interp {name}: max err / bound {float((err / np.maximum(c.bound, 1e-300)).max()):.3f}, longest run {int(c.run.max())}")
    assert np.all(err <= c.bound)
    assert np.all(got[:nc][c.run == 0] == 0)
