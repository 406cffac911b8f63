"""The geometry kernels (csrc/p2w_geom.hip: sampler, level gather, ball query, kNN in brute-force, grid and indexed form, the k = 2
hints, the tile boxes) on the MI355X through the C ABI, on device copies of what the plain reference tests/geom_ref.py builds, for
every named case of that file (tests/test_geom_ref_cpu.py ties the reference to oracle/ops.py and asserts that every case meets the
condition it is named for and which wrong kernel it catches).  Every table is integers or float32 bit patterns: every comparison is
exact.  Outputs are filled with a sentinel before every call; rows and entries a call must not write are compared with it."""
import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import geom_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
X, QROW, BOX = R.X_INDEX_IN_W, R.Q_ROW_IN_W, R.BOX
SLACK = 70                                                                  # m_bound / n_bound beyond the device-side counts
FILL = 0x5A                                                                 # byte the sampler's outputs are filled with


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _ok(code, what):
    assert code == 0, (what, code)


# ---- searches ------------------------------------------------------------------------------------------------------------------------------

_inputs = {}


def _search_inputs(name):
    if name not in _inputs:
        c = R.search_case(name)
        qidx, ptr_qs = c.self_queries()
        boxes = R.tile_bbox(c.x, c.ptr_x, int(_lib.lib().p2w_tile_bbox_count(len(c.ptr_x) - 1, len(c.x))))
        d = dict(x=_dev(c.x), ptr_x=_dev(c.ptr_x), q=_dev(c.q), ptr_q=_dev(c.ptr_q), qidx=_dev(qidx) if len(qidx) else None, ptr_qs=_dev(ptr_qs),
                 boxes=_dev(boxes), keys=None if c.keys is None else _dev(c.keys), grid=None if c.grid is None else _dev(np.concatenate([c.grid, np.zeros(8, np.uint8)])),
                 cell_start=None if c.cell_start is None else _dev(c.cell_start), qidx_host=qidx, ptr_qs_host=ptr_qs)
        _inputs[name] = d
    return _inputs[name]


def _search(name, entry, mode, param, flags, self_q=False, boxes=False, table=False, hint=None, x=None, bbox=None):
    """One call of one entry point on the named case; (nbr, deg) on the host, the rows beyond the queries included."""
    L, c, d = _lib.lib(), R.search_case(name), _search_inputs(name)
    B = len(c.ptr_x) - 1
    xq, qidx, ptr_q, m = (d["x"], d["qidx"], d["ptr_qs"], int(d["ptr_qs_host"][-1])) if self_q else (d["q"], None, d["ptr_q"], int(c.ptr_q[-1]))
    xx = d["x"] if x is None else x
    if self_q and x is not None:
        xq = xx
    r, k = (param[0], param[1]) if mode == "ball" else (None, param)
    rows = max(c.rows, m) + SLACK
    nbr = torch.full((rows, k), R.SENTINEL, dtype=torch.int32, device="cuda")
    deg = torch.full((rows,), R.SENTINEL, dtype=torch.int32, device="cuda")
    m_bound, s = m + SLACK, _lib.stream()
    bb = _p(bbox) if bbox is not None else (_p(d["boxes"]) if boxes else None)
    cs = _p(d["cell_start"]) if table else None
    if entry == "brute" and mode == "knn":
        code = L.p2w_knn(_p(xx), _p(d["ptr_x"]), _p(xq), _p(qidx), _p(ptr_q), B, m_bound, k, _p(nbr), _p(deg), bb, flags, s)
    elif entry == "brute":
        code = L.p2w_ball_query(_p(xx), _p(d["ptr_x"]), _p(xq), _p(qidx), _p(ptr_q), B, m_bound, r, k, _p(nbr), _p(deg), bb, flags, s)
    elif entry == "grid" and mode == "knn":
        code = L.p2w_knn_grid(_p(xx), _p(d["keys"]), _p(d["ptr_x"]), _p(d["grid"]), _p(xq), _p(qidx), _p(ptr_q), B, m_bound, k, _p(nbr), _p(deg),
                              _p(hint), flags, s)
    elif entry == "grid":
        code = L.p2w_ball_query_grid(_p(xx), _p(d["keys"]), _p(d["ptr_x"]), _p(d["grid"]), _p(xq), _p(qidx), _p(ptr_q), B, m_bound, r, k, _p(nbr),
                                     _p(deg), flags, s)
    elif mode == "knn":
        code = L.p2w_knn_grid_indexed(_p(xx), _p(d["keys"]), _p(d["ptr_x"]), _p(d["grid"]), cs, _p(xq), _p(qidx), _p(ptr_q), B, m_bound, k, _p(nbr),
                                      _p(deg), _p(hint), flags, s)
    else:
        code = L.p2w_ball_query_grid_indexed(_p(xx), _p(d["keys"]), _p(d["ptr_x"]), _p(d["grid"]), cs, _p(xq), _p(qidx), _p(ptr_q), B, m_bound, r, k,
                                             _p(nbr), _p(deg), flags, s)
    _ok(code, (name, entry, mode, param, flags))
    torch.cuda.synchronize()
    return _host(nbr), _host(deg)


_wanted = {}


def _want(name, mode, param, flags, self_q, x=None):
    """The reference's (nbr, deg), rows as _search allocates them."""
    key = (name, mode, param, flags & (X | QROW), self_q)
    if x is not None or key not in _wanted:
        c, d = R.search_case(name), _search_inputs(name)
        xs = c.x if x is None else x
        q, qidx, ptr_q = (None, d["qidx_host"], d["ptr_qs_host"]) if self_q else (c.q, None, c.ptr_q)
        rows = max(c.rows, int(ptr_q[-1])) + SLACK
        if mode == "knn":
            got = R.knn(xs, c.ptr_x, q, ptr_q, param, flags & (X | QROW), qidx=qidx, rows=rows)
        else:
            got = R.ball(xs, c.ptr_x, q, ptr_q, param[0], param[1], flags & (X | QROW), qidx=qidx, rows=rows)
        if x is not None:
            return got
        _wanted[key] = got
    return _wanted[key]


def _calls(c, mode, param):
    """(entry, flags, self_q, boxes, table) of every entry point that applies to one search of a case."""
    k = param if mode == "knn" else param[1]
    out = [("brute", fl, sq, bx, False) for fl, sq in ((0, False), (X, False), (X | QROW, False), (0, True), (X, True)) for bx in (False, True)]
    if c.keys is not None and k <= 64:
        out += [("grid", fl, sq, False, False) for fl, sq in ((0, False), (X, False), (X | QROW, False), (BOX, False), (BOX | X, False), (0, True), (BOX | X, True))]
        if c.cell_start is not None:
            out += [("indexed", fl, sq, False, True) for fl, sq in ((0, False), (BOX | X | QROW, False), (X, True))]
        out += [("indexed", X, False, False, False)]                        # cell_start NULL: the bisection behind the indexed entry point
    return out


SEARCHES = sorted(R.SEARCH)


@pytest.mark.parametrize("name", SEARCHES)
def test_every_search_entry_point_equals_the_reference(name):
    c = R.search_case(name)
    wrong = []                                                             # every call of the case is made before the test fails
    for mode, params in (("knn", c.ks), ("ball", c.balls)):
        for param in params:
            for entry, flags, self_q, boxes, table in _calls(c, mode, param):
                if self_q and _search_inputs(name)["qidx"] is None:
                    continue
                nbr, deg = _search(name, entry, mode, param, flags, self_q, boxes, table)
                want = _want(name, mode, param, flags, self_q)
                bad = np.flatnonzero((nbr != want[0]).any(1) | (deg != want[1]))
                if len(bad):
                    wrong.append(((mode, param, entry, flags, self_q, boxes, table), bad[:4].tolist(), nbr[bad[0]].tolist(), want[0][bad[0]].tolist(),
                                  int(deg[bad[0]]), int(want[1][bad[0]])))
    assert not wrong, (name, len(wrong), wrong[:6])


@pytest.mark.parametrize("hint_name", sorted(R.search_case("hints_planted").hints))
def test_planted_hints_change_no_result(hint_name):
    """A hint is an upper bound that is verified: exact, bogus (the float below the true k-th d2: a rescan, no candidate twice), one
    +inf among 31 finite ones, the largest at and above 9 res^2, zero on coincident points, a voxel of one candidate with k = 2."""
    c = R.search_case("hints_planted")
    k, h = c.hints[hint_name]
    hint = _dev(np.concatenate([h, np.full(SLACK, np.nan, F)]))
    for entry, flags, table in (("grid", 0, False), ("grid", BOX, False), ("indexed", X, True), ("indexed", X | QROW | BOX, True)):
        nbr, deg = _search("hints_planted", entry, "knn", k, flags, table=table, hint=hint)
        want = _want("hints_planted", "knn", k, flags, False)
        assert np.array_equal(nbr, want[0]) and np.array_equal(deg, want[1]), (hint_name, entry, flags)


@pytest.mark.parametrize("name", sorted(R.HINT2))
def test_knn_hint2_equals_its_restatement_bit_for_bit_and_seeds_exact_searches(name):
    L = _lib.lib()
    q, rank, ptr_q, xc, ptr_c, keys_c, grid, cstart = R.hint2_case(name)
    m, B = len(q), len(ptr_q) - 1
    dq, dr, dpq, dxc, dpc = _dev(q), _dev(rank), _dev(ptr_q), _dev(xc), _dev(ptr_c)
    hint = torch.full((m + SLACK,), float("nan"), dtype=torch.float32, device="cuda")
    _ok(L.p2w_knn_hint2(_p(dq), _p(dr), _p(dpq), B, m + SLACK, _p(dxc), _p(hint), _lib.stream()), name)
    got = _host(hint)
    want = R.knn_hint2(q, rank, ptr_q, xc)
    assert np.array_equal(R.bits(got[:m]), R.bits(want)) and np.isnan(got[m:]).all()
    true2 = R.kth_d2(xc, ptr_c, q, ptr_q, 2)
    two = np.repeat(np.diff(ptr_c) >= 2, np.diff(ptr_q))
    assert (got[:m][two] >= true2[two]).all()
    dk, dg, dcs = _dev(keys_c), _dev(np.concatenate([grid, np.zeros(8, np.uint8)])), _dev(cstart)
    for k in (1, 2):
        ref = R.knn(xc, ptr_c, q, ptr_q, k, rows=m + SLACK)
        for flags, cs in ((0, None), (0, dcs), (BOX, dcs)):
            nbr = torch.full((m + SLACK, k), R.SENTINEL, dtype=torch.int32, device="cuda")
            deg = torch.full((m + SLACK,), R.SENTINEL, dtype=torch.int32, device="cuda")
            _ok(L.p2w_knn_grid_indexed(_p(dxc), _p(dk), _p(dpc), _p(dg), _p(cs), _p(dq), None, _p(dpq), B, m + SLACK, k, _p(nbr), _p(deg), _p(hint),
                                       flags, _lib.stream()), (name, k, flags))
            assert np.array_equal(_host(nbr), ref[0]) and np.array_equal(_host(deg), ref[1]), (name, k, flags)


@pytest.mark.parametrize("mode,param", [("knn", 8), ("knn", 100), ("knn", 2), ("ball", (0.45, 8)), ("ball", (0.45, 100))])
def test_a_nan_candidate_is_never_reported(mode, param):
    """Brute force only: a candidate with a NaN coordinate is never reported, deg counts only admitted candidates (the five-candidate
    voxel keeps four), and every other row equals the reference's, which orders the remaining candidates alone."""
    name = "sizes_k_and_cap_sweep"
    c = R.search_case(name)
    x = c.x.copy()
    bad = [int(c.ptr_x[0]) + 2, int(c.ptr_x[1]) + 7]
    x[bad[0], 0], x[bad[1], 2] = np.nan, np.nan
    dx, L, B = _dev(x), _lib.lib(), len(c.ptr_x) - 1
    box = torch.full((int(L.p2w_tile_bbox_count(B, len(x))), 6), float("nan"), dtype=torch.float32, device="cuda")
    _ok(L.p2w_tile_bbox(_p(dx), _p(_search_inputs(name)["ptr_x"]), B, len(x), _p(box), _lib.stream()), "tile_bbox")   # the boxes of the NaN-bearing records
    assert not torch.isnan(box[:3]).any()
    for flags, self_q, bbox in ((0, False, None), (X, False, None), (0, True, None), (0, False, box), (X, False, box), (0, True, box)):
        nbr, deg = _search(name, "brute", mode, param, flags, self_q, x=dx, bbox=bbox)
        want = _want(name, mode, param, flags, self_q, x=x)
        assert np.array_equal(nbr, want[0]) and np.array_equal(deg, want[1]), (mode, param, flags, self_q)
        reported = set(nbr[nbr >= 0].tolist())
        assert not reported & set(bad if not flags & X else x[bad, 3].view(np.int32).tolist())
        if mode == "knn" and not self_q:
            assert (deg[:33] == min(param, 4)).all()


# ---- the sampler and its companions ----------------------------------------------------------------------------------------------------

SAMPLINGS = sorted(R.SAMPLER)


def _filled(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def _sampler_outputs(n_bound, B, cells):
    i32, i64 = torch.int32, torch.int64
    o = dict(idx=_filled(n_bound, i32), ptr=_filled(B + 1, i32), batch=_filled(n_bound, i32), order=_filled(n_bound, i32), skeys=_filled(n_bound, i64),
             ckeys=_filled(n_bound, i64), grid=_filled(8, i64), inv=_filled(n_bound, i32), rank=_filled(n_bound, i32))
    if cells:
        o.update(cs=_filled(cells + 1, i32), css=_filled(cells + 1, i32), status=_filled(1, i32))
    return o


def _padded(c):
    """The case's records followed by SLACK records of NaN that no kernel may read (n_bound > ptr[B])."""
    return _dev(np.concatenate([c.xyzr, np.full((SLACK, 4), np.nan, F)]))


def _assert_level(name, o, S, n, stable, cells=None):
    """Every output of one sampler call against the reference; `stable`: the order inside a cell is ascending (the sort sampler)."""
    M = len(S.idx)
    assert np.array_equal(_host(o["ptr"]), S.ptr), name
    assert np.array_equal(_host(o["idx"])[:M], S.idx) and _untouched(_host(o["idx"])[M:]), name
    assert np.array_equal(_host(o["batch"])[:M], S.batch) and _untouched(_host(o["batch"])[M:]), name
    assert np.array_equal(_host(o["ckeys"], np.uint64)[:M], S.cell_keys) and _untouched(_host(o["ckeys"])[M:]), name
    assert np.array_equal(_host(o["inv"])[:n], S.inv) and _untouched(_host(o["inv"])[n:]), name
    assert np.array_equal(_host(o["skeys"], np.uint64)[:n], S.sorted_keys) and _untouched(_host(o["skeys"])[n:]), name
    assert np.array_equal(_host(o["rank"])[:n], S.rank_sorted) and _untouched(_host(o["rank"])[n:]), name
    assert np.array_equal(_host(o["grid"]).view(np.uint8)[:56], S.grid), name
    order = _host(o["order"])
    assert _untouched(order[n:]) and np.array_equal(np.sort(order[:n]), np.arange(n)), name          # a permutation ...
    assert np.array_equal(S.keys[order[:n]], S.sorted_keys), name                                   # ... ascending in key
    if stable:
        assert np.array_equal(order[:n], S.order), name
    if cells is not None:
        assert np.array_equal(_host(o["cs"])[:S.T + 1], S.cell_start()) and _untouched(_host(o["cs"])[S.T + 1:]), name
        assert np.array_equal(_host(o["css"])[:S.T + 1], S.cell_start_sorted()) and _untouched(_host(o["css"])[S.T + 1:]), name
        assert _host(o["status"]).tolist() == [0], name


def _assert_refused(name, o, res, B):
    """The grid does not fit the table: the status word is set and an empty level with a one-cell grid is handed out."""
    assert _host(o["status"]).tolist() == [1], name
    assert _host(o["ptr"]).tolist() == [0] * (B + 1), name
    assert np.array_equal(_host(o["grid"]).view(np.uint8)[:56], R.grid_image([0, 0, 0], res, [0, 0, 0], 0, [1, 1, 1])), name


def _table_args(c, x, ptr, o, cells, ws):
    B, n_bound = len(c.ptr) - 1, len(c.xyzr) + SLACK
    return (_p(x), _p(ptr), B, n_bound, c.res, _p(o["idx"]), _p(o["ptr"]), _p(o["batch"]), _p(o["order"]), _p(o["skeys"]), _p(o["ckeys"]), _p(o["grid"]),
            _p(o["inv"]), _p(o["rank"]), _p(o["cs"]), _p(o["css"]), _p(o["status"]), cells, _p(ws), ws.numel(), _lib.stream())


@pytest.mark.parametrize("name", SAMPLINGS)
def test_sort_sampler_equals_the_reference(name):
    L, c, S = _lib.lib(), R.sampler_case(name), R.sampled(name)
    n, B, n_bound = len(c.xyzr), len(c.ptr) - 1, len(c.xyzr) + SLACK
    x, ptr, o = _padded(c), _dev(c.ptr), _sampler_outputs(n_bound, B, 0)
    ws = _filled(int(L.p2w_voxel_sample_ws_bytes(n_bound)), torch.uint8)
    ws.fill_(0xFF)
    _ok(L.p2w_voxel_sample(_p(x), _p(ptr), B, n_bound, c.res, _p(o["idx"]), _p(o["ptr"]), _p(o["batch"]), _p(o["order"]), _p(o["skeys"]), _p(o["ckeys"]),
                           _p(o["grid"]), _p(o["inv"]), _p(o["rank"]), _p(ws), ws.numel(), _lib.stream()), name)
    torch.cuda.synchronize()
    _assert_level(name, o, S, n, stable=True)
    # the two halves as separate operators
    cell, inv, perm, count = _filled(n, torch.int64), _filled(n, torch.int32), _filled(n, torch.int32), _filled(1, torch.int32)
    ws.fill_(0xFF)
    _ok(L.p2w_voxel_grid(_p(x), _p(ptr), B, n, c.res, _p(cell), _p(ws), ws.numel(), _lib.stream()), name)
    ws2 = _filled(int(L.p2w_voxel_sample_ws_bytes(n)), torch.uint8)
    ws2.fill_(0xFF)
    _ok(L.p2w_consecutive_cluster(_p(cell), n, _p(inv), _p(perm), _p(count), _p(ws2), ws2.numel(), _lib.stream()), name)
    M = len(S.idx)
    assert np.array_equal(_host(cell, np.uint64), S.keys) and _host(count).tolist() == [M]
    assert np.array_equal(_host(inv), S.inv) and np.array_equal(_host(perm)[:M], S.idx) and _untouched(_host(perm)[M:])


@pytest.mark.parametrize("name", SAMPLINGS)
def test_table_sampler_equals_the_reference_or_refuses(name):
    """p2w_voxel_sample_table on a workspace of 0xFF bytes at every capacity of the case (default: the grid's own size), then
    prepare + prepared twice on one workspace: same results; a grid that does not fit sets the status word and hands out an empty level."""
    L, c, S = _lib.lib(), R.sampler_case(name), R.sampled(name)
    n, B, n_bound = len(c.xyzr), len(c.ptr) - 1, len(c.xyzr) + SLACK
    x, ptr = _padded(c), _dev(c.ptr)
    for cells in (c.table_cells or (S.T,)):
        ws = torch.empty(int(L.p2w_voxel_sample_table_ws_bytes(n_bound, cells)), dtype=torch.uint8, device="cuda")
        for entry in ("table", "prepared", "prepared"):
            o = _sampler_outputs(n_bound, B, cells)
            if entry == "table":
                ws.fill_(0xFF)
                _ok(L.p2w_voxel_sample_table(*_table_args(c, x, ptr, o, cells, ws)), (name, cells))
                ws.fill_(0xFF)
                _ok(L.p2w_voxel_sample_table_prepare(_p(ws), ws.numel(), _lib.stream()), (name, cells))
            else:
                _ok(L.p2w_voxel_sample_table_prepared(*_table_args(c, x, ptr, o, cells, ws)), (name, cells, entry))
            torch.cuda.synchronize()
            if S.T <= cells:
                _assert_level((name, cells, entry), o, S, n, stable=False, cells=cells)
            else:
                _assert_refused((name, cells, entry), o, c.res, B)


@pytest.mark.parametrize("name", SAMPLINGS)
def test_index_records_tile_boxes_and_level_gather_equal_the_reference(name):
    L, c, S = _lib.lib(), R.sampler_case(name), R.sampled(name)
    n, B, n_bound = len(c.xyzr), len(c.ptr) - 1, len(c.xyzr) + SLACK
    x, ptr = _padded(c), _dev(c.ptr)
    out = _filled((n_bound, 4), torch.float32)
    order = _dev(np.concatenate([S.order, np.full(SLACK, -1, np.int32)]))
    _ok(L.p2w_index_records(_p(x), _p(order), _p(ptr), B, n_bound, _p(out), _lib.stream()), name)
    got = _host(out)
    assert np.array_equal(R.bits(got[:n]), R.bits(R.records(c.xyzr[S.order][:, :3], S.order))) and _untouched(got[n:])
    rows = int(L.p2w_tile_bbox_count(B, n_bound))
    box = _filled((rows, 6), torch.float32)
    _ok(L.p2w_tile_bbox(_p(x), _p(ptr), B, n_bound, _p(box), _lib.stream()), name)
    want, got = R.tile_bbox(c.xyzr, c.ptr, rows), _host(box)
    used = ~np.isnan(want[:, 0])
    assert used.sum() == sum(-(-int(v) // R.TILE) for v in np.diff(c.ptr)) and np.array_equal(R.bits(got[used]), R.bits(want[used])) and _untouched(got[~used])
    sf = np.array([R.SF_LIST[b % len(R.SF_LIST)] for b in range(B)], F)
    M = len(S.idx)
    dst = _filled((n_bound, 4), torch.float32)
    idx, batch = _dev(np.concatenate([S.idx, np.full(n_bound - M, -1, np.int32)])), _dev(np.concatenate([S.batch, np.full(n_bound - M, -1, np.int32)]))
    ptr_dst, dsf = _dev(S.ptr), _dev(sf)                                   # (named: a device array must outlive the call that reads it)
    _ok(L.p2w_level_gather(_p(x), _p(idx), _p(batch), _p(ptr_dst), B, n_bound, _p(dsf), _p(dst), _lib.stream()), name)
    got = _host(dst)
    assert np.array_equal(R.bits(got[:M]), R.bits(R.gather(c.xyzr, S.idx, S.batch, sf))) and _untouched(got[M:])


# ---- the engine's chain -------------------------------------------------------------------------------------------------------------------

def test_engine_chain_equals_the_reference_table_by_table():
    """sample (prepared table sampler), gather with the round trip, sample again ..., then the ball query, the two kNN searches and the
    three hinted k = 2 searches with the arguments and flags of engine.py, on two voxels whose scale factors move sampled points across
    cell faces: every search runs over round-tripped coordinates with the keys of the coordinates before the round trip."""
    L, s = _lib.lib(), _lib.stream()
    x, ptr, sf = R.chain_input()
    N, B, k, cells = len(x), len(ptr) - 1, R.CHAIN_K, 1 << 14
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    ws = torch.empty(int(L.p2w_voxel_sample_table_ws_bytes(N, cells)), dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)
    _ok(L.p2w_voxel_sample_table_prepare(_p(ws), ws.numel(), s), "prepare")
    lv = [dict(xyzr=_dev(x), ptr=_dev(ptr))]
    dsf, out = _dev(sf), []
    for l, res in enumerate(R.CHAIN_RES):
        o = _sampler_outputs(N, B, cells)
        src = lv[l]
        _ok(L.p2w_voxel_sample_table_prepared(_p(src["xyzr"]), _p(src["ptr"]), B, N, res, _p(o["idx"]), _p(o["ptr"]), _p(o["batch"]),
                                              _p(o["order"]) if l == 0 else None, _p(o["skeys"]) if l == 0 else None, _p(o["ckeys"]), _p(o["grid"]),
                                              _p(o["inv"]) if l > 0 else None, _p(o["rank"]) if l == 0 else None, _p(o["cs"]),
                                              _p(o["css"]) if l == 0 else None, _p(o["status"]), cells, _p(ws), ws.numel(), s), ("sample", l))
        nxt = dict(xyzr=_filled((N, 4), f32), ptr=o["ptr"])
        _ok(L.p2w_level_gather(_p(src["xyzr"]), _p(o["idx"]), _p(o["batch"]), _p(o["ptr"]), B, N, _p(dsf), _p(nxt["xyzr"]), s), ("gather", l))
        lv.append(nxt)
        out.append(o)
    sorted0 = _filled((N, 4), f32)
    _ok(L.p2w_index_records(_p(lv[0]["xyzr"]), _p(out[0]["order"]), _p(lv[0]["ptr"]), B, N, _p(sorted0), s), "index_records")
    torch.cuda.synchronize()
    order = _host(out[0]["order"])
    T = R.chain(x, ptr, sf, order0=order)
    S0 = T["S"][0]
    assert np.array_equal(np.sort(order), np.arange(N)) and np.array_equal(S0.keys[order], S0.sorted_keys)
    assert np.array_equal(R.bits(_host(sorted0)), R.bits(T["sorted0"])) and np.array_equal(_host(out[0]["rank"]), S0.inv[order])
    assert np.array_equal(_host(out[0]["css"])[:S0.T + 1], S0.cell_start_sorted()) and np.array_equal(_host(out[0]["skeys"], np.uint64), S0.sorted_keys)
    for l in range(3):
        S, o, M = T["S"][l], out[l], len(T["S"][l].idx)
        assert _host(o["status"]).tolist() == [0] and np.array_equal(_host(o["ptr"]), S.ptr) and np.array_equal(_host(o["idx"])[:M], S.idx)
        assert np.array_equal(_host(o["batch"])[:M], S.batch) and np.array_equal(_host(o["ckeys"], np.uint64)[:M], S.cell_keys)
        assert np.array_equal(_host(o["grid"]).view(np.uint8)[:56], S.grid) and np.array_equal(_host(o["cs"])[:S.T + 1], S.cell_start())
        assert l == 0 or np.array_equal(_host(o["inv"])[:len(S.inv)], S.inv)
        assert np.array_equal(R.bits(_host(lv[l + 1]["xyzr"])[:M]), R.bits(T["xyzr"][l + 1])), ("gather", l)

    def table(kk):
        return torch.full((N, kk), R.SENTINEL, dtype=i32, device="cuda"), torch.full((N,), R.SENTINEL, dtype=i32, device="cuda")

    def same(got, want, what):
        assert np.array_equal(_host(got[0]), want[0]) and np.array_equal(_host(got[1]), want[1]), what
    got = table(k)
    _ok(L.p2w_ball_query_grid_indexed(_p(sorted0), _p(out[0]["skeys"]), _p(lv[0]["ptr"]), _p(out[0]["grid"]), _p(out[0]["css"]), _p(lv[0]["xyzr"]),
                                      _p(out[0]["idx"]), _p(lv[1]["ptr"]), B, N, R.CHAIN_RES[0] * 2, k, _p(got[0]), _p(got[1]), X, s), "ball")
    same(got, T["sa"][0], "ball")
    for l in (1, 2):
        got = table(k)
        _ok(L.p2w_knn_grid_indexed(_p(lv[l]["xyzr"]), _p(out[l - 1]["ckeys"]), _p(lv[l]["ptr"]), _p(out[l - 1]["grid"]), _p(out[l - 1]["cs"]),
                                   _p(lv[l]["xyzr"]), _p(out[l]["idx"]), _p(lv[l + 1]["ptr"]), B, N, k, _p(got[0]), _p(got[1]), None, 0, s), ("knn", l))
        same(got, T["sa"][l], ("knn", l))
    for f in (2, 1, 0):
        q, fl, rank = (sorted0, QROW, out[0]["rank"]) if f == 0 else (lv[f]["xyzr"], 0, out[f]["inv"])
        hint = torch.full((N,), float("nan"), dtype=f32, device="cuda")
        _ok(L.p2w_knn_hint2(_p(q), _p(rank), _p(lv[f]["ptr"]), B, N, _p(lv[f + 1]["xyzr"]), _p(hint), s), ("hint", f))
        m = len(T["hint"][f])
        assert np.array_equal(R.bits(_host(hint)[:m]), R.bits(T["hint"][f])), ("hint", f)
        got = table(2)
        _ok(L.p2w_knn_grid_indexed(_p(lv[f + 1]["xyzr"]), _p(out[f]["ckeys"]), _p(lv[f + 1]["ptr"]), _p(out[f]["grid"]), _p(out[f]["cs"]), _p(q), None,
                                   _p(lv[f]["ptr"]), B, N, 2, _p(got[0]), _p(got[1]), _p(hint), fl, s), ("knn2", f))
        same(got, T["fp"][f], ("knn2", f))
