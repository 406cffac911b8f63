"""The voxeliser's cap on the GPU: p2w_cap_subset through the C ABI against tests/cap_ref.py, with a caller-owned workspace filled with
0xFF bytes beforehand - planted keys bit for bit, generated keys within one float32 ulp and the selection bit for bit on the device's
own keys, the replacement mode bit for bit; then ``ops.cap_subset``, ``preprocessing.voxelise(cap=)`` and ``pipeline.segment_plot``.
T = P2W_SAMPLE_TILE = 1024 rows per workgroup; a segment's tiles start at the segment's first row.  The scan of the segments' tile
counts takes a second level from 4096 segments on, the scan of the per-tile counters where n / 1024 + S + 1 exceeds 2048."""
import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import cap_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = (0x1234 << 32) | 0x9abcdef1
T = 1024
UNTOUCHED = 0x5a5a5a5a


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def _call(n, starts, counts, k, keys=None, weight=None, row_id=None, seed=SEED, c1=3, c2=5, want_keys=False, fill=0xFF):
    """-> (idx [S, k] int64, keys_out [n] uint32 or None) as numpy arrays; every output is pre-filled with a value no draw can give."""
    L = _lib.lib()
    S = len(starts)
    ws = torch.full((max(int(L.p2w_cap_subset_ws_size(n, S)), 1),), fill, dtype=torch.uint8, device=DEV)
    idx = torch.full((S, k), -7, dtype=torch.int64, device=DEV)
    kout = torch.full((n,), UNTOUCHED, dtype=torch.int32, device=DEV) if want_keys else None
    kin = None if keys is None else _dev(np.asarray(keys, dtype=np.uint32).view(np.int32), np.int32)
    st, ct, w, rid = _dev(starts, np.int64), _dev(counts, np.int64), _dev(weight, np.float32), _dev(row_id, np.int64)
    _lib.check(L.p2w_cap_subset(n, _lib.ptr(st), _lib.ptr(ct), S, k, _lib.ptr(w), _lib.ptr(rid), seed, c1, c2, _lib.ptr(kin),
                                _lib.ptr(idx), _lib.ptr(kout), _lib.ptr(ws), ws.numel(), _lib.stream()), "p2w_cap_subset")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), None if kout is None else kout.cpu().numpy().view(np.uint32)


def _random_keys(n, seed):
    """uint32 keys with many duplicates in every digit position"""
    g = np.random.default_rng(seed)
    key = g.integers(0, 1 << 32, n, dtype=np.uint64)
    key[::3] &= 0xffffff00
    key[1::5] = key[0]
    return key.astype(np.uint32)


def _planted(n, starts, counts, k, keys):
    got, kout = _call(n, starts, counts, k, keys=keys, want_keys=True)
    want = R.select(n, starts, counts, k, keys)
    assert np.array_equal(got, want)
    inside = np.zeros(n, bool)
    for a, c in zip(*R.ranges(n, starts, counts)):
        inside[a:a + c] = True
    assert np.array_equal(kout[inside], np.asarray(keys, np.uint32)[inside]) and (kout[~inside] == UNTOUCHED).all()
    return got


# ---- planted keys ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [2, 63, 64, 65, 1023, 1024, 1025, 2049, 5197])
def test_one_segment_bit_for_bit(count):
    n, start = count + 40, 17
    keys = _random_keys(n, count)
    for k in sorted({1, max(1, count // 2), count - 1}):
        got = _planted(n, [start], [count], k, keys)
        assert (np.diff(got[0]) > 0).all() and start <= got[0, 0] and got[0, -1] < start + count


def test_a_segment_that_starts_at_row_1000():
    """rows 1000 .. 2499: across the row space's multiple of 1024 and across the segment's own tile boundary at row 2024"""
    n = 3000
    keys = _random_keys(n, 7)
    for k in (1, 700, 1499):
        _planted(n, [1000], [1500], k, keys)


def test_many_small_segments_in_one_call():
    g = np.random.default_rng(3)
    counts = g.integers(6, 41, 300)
    gaps = g.integers(0, 4, 300)
    starts = np.cumsum(counts + gaps) - counts
    n = int(starts[-1] + counts[-1] + 9)
    got = _planted(n, starts, counts, 5, _random_keys(n, 11))
    assert (got >= starts[:, None]).all() and (got < (starts + counts)[:, None]).all()


def test_one_large_segment_next_to_many_small_ones():
    counts = np.array([30] * 40 + [40000] + [17] * 40)
    starts = np.cumsum(counts + 2) - counts
    n = int(starts[-1] + counts[-1])
    _planted(n, starts, counts, 16, _random_keys(n, 13))
    _planted(n, starts, counts, 20000, _random_keys(n, 14))      # (the small ones are below k: all their rows, then -1)


def test_segments_at_or_below_k_are_filled_with_minus_one():
    counts = [0, 1, 3, 5, 8, 0]
    starts = [0, 2, 4, 9, 15, 30]
    got = _planted(30, starts, counts, 5, _random_keys(30, 5))
    for s, (a, c) in enumerate(zip(starts, counts)):
        assert got[s, :min(c, 5)].tolist() == (list(range(a, a + c)) if c <= 5 else sorted(got[s].tolist()))
        assert (got[s, min(c, 5):] == -1).all()


def test_starts_and_counts_are_clamped_to_the_row_space():
    n = 50
    starts, counts = [-5, 10, n - 3, n + 7, 40], [8, 20, 100, 5, -2]
    got = _planted(n, starts, counts, 4, _random_keys(n, 17))
    assert set(got[0].tolist()) <= set(range(8)) and got[2].tolist() == [47, 48, 49, -1] and (got[3:] == -1).all()


def _shapes():
    n = 4 * T + 100
    i = np.arange(n, dtype=np.uint64)
    cases = {"all_equal": (np.full(n, 0x12345678), n // 2), "all_zero": (np.zeros(n), n // 3), "all_ones": (np.full(n, 0xffffffff), n - 1),
             "descending": ((n - 1 - i) * 70001, 1234)}
    # the boundary value on rows 900 .. 1200 of the segment (across its tile boundary at 1024), 100 rows below it in two other tiles,
    # everything else above: k = 300 takes the 100 and the lowest 200 of the 301 equal rows
    two = np.full(n, 0xf0000000)
    two[900:1201] = 0x80000001
    two[0:50] = 0x80000000
    two[2 * T + 500:2 * T + 550] = 0x7fffffff
    cases["threshold_straddles"] = (two, 300)
    cases["threshold_two_tiles"] = (np.where((i % 3) == 0, 7, 9), n // 3 - 400)
    for d in range(4):                                            # keys that differ in ONE digit only: that select pass decides alone
        digit = (i * 37 + 11) % 256
        base = 0xa5c3e17b & ~(0xff << (8 * d)) & 0xffffffff
        cases[f"digit{d}_only"] = (base | (digit << np.uint64(8 * d)), n // 2 + 3)
    return n, {name: (np.asarray(v, dtype=np.uint64).astype(np.uint32), k) for name, (v, k) in cases.items()}


SHAPE_N, SHAPES = _shapes()
OFFSET = 333                                                      # the segment's first row: tiles are counted from there


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_planted_shapes(name):
    """The segment is rows 333 .. 333 + n of a wider row space, between two small segments whose keys would win if they were looked at."""
    seg, k = SHAPES[name]
    keys = np.concatenate([np.zeros(OFFSET, np.uint32), seg, np.zeros(50, np.uint32)])
    got = _planted(len(keys), [0, OFFSET, OFFSET + SHAPE_N + 5], [300, SHAPE_N, 40], k, keys)
    mine = got[1] - OFFSET
    assert np.array_equal(got[0, :300], np.arange(300)) and (got[0, 300:] == -1).all()
    if name.startswith("all_"):
        assert np.array_equal(mine, np.arange(k))
    if name == "descending":
        assert np.array_equal(mine, np.arange(SHAPE_N - k, SHAPE_N))
    if name == "threshold_straddles":
        assert np.array_equal(mine, np.concatenate([np.arange(0, 50), np.arange(900, 1100), np.arange(2 * T + 500, 2 * T + 550)]))


def test_second_level_of_the_segment_scan():
    """4096 segments: S + 1 = 4097 tile counts, the smallest number that needs a second 4096-entry tile of the scan (and, with
    n / 1024 + S + 1 = 4129 tiles, the counters' scan is on its second level too)"""
    S = 4096
    counts = 5 + (np.arange(S) * 7) % 11
    starts = np.cumsum(counts) - counts
    n = int(counts.sum())
    _planted(n, starts, counts, 6, _random_keys(n, 19))


def test_second_level_of_the_counter_scan():
    """two segments over 2047 x 1024 + 5 rows: n / 1024 + S + 1 = 2050 tiles, 4100 counters"""
    n = 2047 * T + 5
    keys = _random_keys(n, 23)
    _planted(n, [0, 1500 * T + 3], [1500 * T, n - 1500 * T - 3], 100000, keys)


# ---- generated keys ----------------------------------------------------------------------------------------------------------------

def _weights(n, seed):
    g = np.random.default_rng(seed)
    w = np.exp(g.uniform(-12, 6, n)).astype(np.float32)
    w[::37] = [0.0, -1.0, np.inf, np.nan, -0.0, -np.inf][seed % 6]
    w[5::11] = 1.2e-38                                            # keys near and beyond the top of float32 (+inf is a valid key)
    w[7::59] = 3e38
    return w


def test_generated_keys_and_the_selection_on_them():
    """keys_out against the float64 restatement: a valid key within 1 float32 ulp (half an ulp of the final rounding, plus the device's
    double log - 1 ulp in double - moving a rounding boundary: no more); invalid weights exactly 0xFFFFFFFF; rows of no segment
    unwritten; idx_out bit for bit the restatement's selection on the device's own keys."""
    counts = np.array([40, 1025, 7000, 3, 300])
    starts = np.cumsum(counts + 11) - counts
    n = int(starts[-1] + counts[-1] + 5)
    g = np.random.default_rng(1)
    row_id = g.permutation(n).astype(np.int64) + (np.arange(n, dtype=np.int64) % 3 << 32) * (np.arange(n) % 2)
    differ = 0
    for case, (k, rid) in enumerate([(20, row_id), (512, None), (4000, row_id)]):
        w = _weights(n, case)
        got, key = _call(n, starts, counts, k, weight=w, row_id=rid, want_keys=True, c1=case, c2=9)
        want = R.race_keys(np.arange(n) if rid is None else rid, w, SEED, case, 9)
        inside = np.zeros(n, bool)
        for a, c in zip(starts, counts):
            inside[a:a + c] = True
        valid = np.isfinite(w) & (w > 0)
        assert (key[~inside] == UNTOUCHED).all()
        assert (key[inside & ~valid] == 0xFFFFFFFF).all() and (~valid[inside]).sum() > 50
        off = np.abs(key[inside & valid].astype(np.int64) - want[inside & valid].astype(np.int64))
        differ += int((off != 0).sum())
        assert off.max() <= 1 and (key[inside & valid] <= 0x7f800000).all()
        assert (key[inside] == 0x7f800000).sum() > 0
        assert np.array_equal(got, R.select(n, starts, counts, k, key))
    print(f"keys that are not identical to the float64 restatement's: {differ}")


def test_counters_seed_and_row_id_reach_the_generator():
    n, k = 3000, 700
    w = _weights(n, 1)
    draws = {}
    for seed, c1, c2 in [(SEED, 0, 0), (SEED, 1, 0), (SEED, 0, 1), (SEED ^ 1, 0, 0), (SEED ^ (1 << 40), 0, 0), (141190, 0xffffffff, 0xfffffffe)]:
        got, key = _call(n, [0], [n], k, weight=w, seed=seed, c1=c1, c2=c2, want_keys=True)
        assert np.abs(key.astype(np.int64) - R.race_keys(np.arange(n), w, seed, c1, c2).astype(np.int64)).max() <= 1
        draws[(seed, c1, c2)] = got.tobytes()
    draws["row_id"] = _call(n, [0], [n], k, weight=w, row_id=np.arange(n) + 1, c1=0, c2=0)[0].tobytes()
    assert len(set(draws.values())) == len(draws)


# ---- replacement mode --------------------------------------------------------------------------------------------------------------

def test_replacement_mode_bit_for_bit():
    n = 1 << 24                                                   # (no array of n elements exists in this mode)
    starts, counts = [0, 70, 5000, 100000, n + 4], [64, 1, 0, n - 100000, 9]
    row_id = None
    for k, c2 in [(1, 0), (300, 7), (5000, 0xffffffff)]:
        got, _ = _call(n, starts, counts, k, c2=c2)
        assert np.array_equal(got, R.replace(n, starts, counts, k, SEED, c2, row_id))
        assert (got[2] == -1).all() and (got[4] == -1).all() and (got[1] == 70).all()
    m = 6000
    rid = np.random.default_rng(2).permutation(m).astype(np.int64) + (1 << 33)
    got, _ = _call(m, [5, 4000], [3000, 2000], 777, row_id=rid, c2=3)
    assert np.array_equal(got, R.replace(m, [5, 4000], [3000, 2000], 777, SEED, 3, rid))
    assert not np.array_equal(got, _call(m, [5, 4000], [3000, 2000], 777, c2=3)[0])


# ---- purity ------------------------------------------------------------------------------------------------------------------------

def test_a_segment_depends_on_its_own_rows_alone():
    """The same voxel (row_ids and weights) alone, among other segments and at another position: the same chosen row_ids."""
    g = np.random.default_rng(4)
    c, k = 2500, 600
    rid, w = g.permutation(100000)[:c].astype(np.int64), np.exp(g.uniform(-3, 3, c)).astype(np.float32)
    alone, _ = _call(c, [0], [c], k, weight=w, row_id=rid)
    pad = lambda m, s: (g.permutation(100000)[:m].astype(np.int64) + 200000 * s, np.exp(g.uniform(-3, 3, m)).astype(np.float32))
    (r1, w1), (r2, w2) = pad(1777, 1), pad(900, 2)
    among, _ = _call(1777 + c + 900, [0, 1777, 1777 + c], [1777, c, 900], k, weight=np.concatenate([w1, w, w2]),
                     row_id=np.concatenate([r1, rid, r2]))
    moved, _ = _call(c + 123, [123], [c], k, weight=np.concatenate([w2[:123], w]), row_id=np.concatenate([r2[:123], rid]))
    assert np.array_equal(rid[alone[0]], rid[among[1] - 1777]) and np.array_equal(rid[alone[0]], rid[moved[0] - 123])
    # replacement mode knows a segment by row_id[start] and its count
    a, _ = _call(c, [0], [c], k, row_id=rid)
    b, _ = _call(1777 + c, [0, 1777], [1777, c], k, row_id=np.concatenate([r1, rid]))
    assert np.array_equal(a[0], b[1] - 1777)


def test_same_bits_on_every_run_whatever_the_workspace_held():
    counts = np.array([30] * 10 + [9000] + [1025] * 3)
    starts = np.cumsum(counts + 2) - counts
    n = int(starts[-1] + counts[-1])
    w = _weights(n, 2)
    first, k1 = _call(n, starts, counts, 500, weight=w, want_keys=True)
    again, k2 = _call(n, starts, counts, 500, weight=w, want_keys=True)
    zeroed, k3 = _call(n, starts, counts, 500, weight=w, want_keys=True, fill=0x00)
    assert first.tobytes() == again.tobytes() == zeroed.tobytes() and k1.tobytes() == k2.tobytes() == k3.tobytes()
    seg, k = SHAPES["threshold_straddles"]
    assert _call(SHAPE_N, [0], [SHAPE_N], k, keys=seg)[0].tobytes() == _call(SHAPE_N, [0], [SHAPE_N], k, keys=seg, fill=0x00)[0].tobytes()


def test_refused_calls_write_nothing():
    L = _lib.lib()
    idx = torch.full((2, 8), -7, dtype=torch.int64, device=DEV)
    seg = torch.tensor([0, 8], dtype=torch.int64, device=DEV)
    w = torch.ones(16, device=DEV)
    ws = torch.empty(int(L.p2w_cap_subset_ws_size(16, 2)), dtype=torch.uint8, device=DEV)
    call = lambda k, weight, size: L.p2w_cap_subset(16, seg.data_ptr(), seg.data_ptr(), 2, k, weight, None, SEED, 0, 0, None, idx.data_ptr(),
                                                    None, ws.data_ptr(), size, _lib.stream())
    assert call(0, w.data_ptr(), ws.numel()) == -1 and call(8, w.data_ptr(), ws.numel() - 1) == -4 and call(0, None, 0) == -1
    assert call(8, w.data_ptr() + 2, ws.numel()) == -3
    torch.cuda.synchronize()
    assert (idx == -7).all()


# ---- the operator ------------------------------------------------------------------------------------------------------------------

def test_operator_is_the_c_abi_and_makes_no_host_wait():
    """ops.cap_subset gives the C ABI's bits, and it completes under torch's synchronisation watch in its raising mode."""
    from pointstowood_amd import ops
    counts = np.array([40, 1025, 7000, 3, 300])
    starts = np.cumsum(counts + 11) - counts
    n = int(starts[-1] + counts[-1] + 5)
    w, rid = _weights(n, 3), np.random.default_rng(8).permutation(n).astype(np.int64)
    st, ct, dw, drid = _dev(starts, np.int64), _dev(counts, np.int64), _dev(w, np.float32), _dev(rid, np.int64)
    want, want_keys = _call(n, starts, counts, 128, weight=w, row_id=rid, c1=9, c2=2, want_keys=True)
    want_rep, _ = _call(n, starts, counts, 128, row_id=rid, c1=9, c2=2)
    ops.cap_subset(n, st, ct, 128, SEED, counter=(9, 2), weight=dw, row_id=drid)     # (library and allocator blocks before the watch)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got, key = ops.cap_subset(n, st, ct, 128, SEED, counter=(9, 2), weight=dw, row_id=drid, return_keys=True)
        rep = ops.cap_subset(n, st, ct, 128, SEED, counter=(9, 2), row_id=drid)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert got.dtype == torch.int64 and got.shape == (5, 128) and got.is_cuda and key.dtype == torch.int32
    inside = want_keys != UNTOUCHED
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(key.cpu().numpy().view(np.uint32)[inside], want_keys[inside])
    assert np.array_equal(rep.cpu().numpy(), want_rep)
    planted = _random_keys(n, 29)
    got = ops.cap_subset(n, st, ct, 128, 0, keys=_dev(planted.view(np.int32), np.int32))
    assert np.array_equal(got.cpu().numpy(), R.select(n, starts, counts, 128, planted))
    assert ops.cap_subset(n, st[:0], ct[:0], 4, SEED, weight=dw).shape == (0, 4)
    with pytest.raises(ValueError):
        ops.cap_subset(n, st, ct, 0, SEED, weight=dw)
    with pytest.raises(ValueError):
        ops.cap_subset(n, st, ct, 4, SEED, weight=dw[:-1])
    with pytest.raises(ValueError):
        ops.cap_subset(n, st, ct, 4, SEED, return_keys=True)
    with pytest.raises(RuntimeError):
        ops.cap_subset(n, st.cpu(), ct.cpu(), 4, SEED)


# ---- the voxeliser -----------------------------------------------------------------------------------------------------------------

MAX_PTS = 300
GRIDS = (2.0, 4.0)


def _recorded_voxelise(monkeypatch, pc, **kw):
    """voxelise(max_pts = 300, cap = ...) with every ops.cap_subset call recorded: (arguments, result)."""
    from pointstowood_amd import ops
    from pointstowood_amd import preprocessing as PP
    calls, real = [], ops.cap_subset

    def recording(n, seg_start, seg_count, k, seed, counter=(0, 0), weight=None, row_id=None, keys=None, return_keys=False):
        out = real(n, seg_start, seg_count, k, seed, counter=counter, weight=weight, row_id=row_id, keys=keys, return_keys=return_keys)
        calls.append((dict(n=n, seg_start=seg_start, seg_count=seg_count, k=k, seed=seed, counter=counter, weight=weight, row_id=row_id), out))
        return out
    monkeypatch.setattr(ops, "cap_subset", recording)
    try:
        return PP.voxelise(pc, GRIDS, min_pts=64, max_pts=MAX_PTS, mode="xyz", **kw), calls
    finally:
        monkeypatch.setattr(ops, "cap_subset", real)


@pytest.fixture(scope="module")
def plots():
    from tests.test_host_cpu import _plot
    return {refl: _plot(n=60000, seed=3, refl=refl).cuda() for refl in (True, False)}


@pytest.mark.parametrize("refl", [True, False])
def test_voxelise_with_a_device_cap(refl, plots, monkeypatch):
    from pointstowood_amd import ops
    from pointstowood_amd import preprocessing as PP
    pc = plots[refl]
    full, nz_full = PP.voxelise(pc, GRIDS, min_pts=64, max_pts=100000, mode="xyz")
    host, _ = PP.voxelise(pc, GRIDS, min_pts=64, max_pts=MAX_PTS, mode="xyz", generator=torch.Generator(device=DEV).manual_seed(1))
    (got, nz), calls = _recorded_voxelise(monkeypatch, pc, cap=PP.DeviceCap(77, counter=6))
    assert len(got) == len(full) == len(host) and torch.equal(nz, nz_full)
    over = [j for j, f in enumerate(full) if f.shape[0] > MAX_PTS]
    assert len(over) >= 20 and len(calls) == 2 and [a["counter"] for a, _ in calls] == [(0, 6), (1, 6)]
    chosen, first = [], []
    for a, out in calls:
        assert a["seed"] == 77 and a["k"] == MAX_PTS and a["n"] == pc.shape[0] and (a["weight"] is not None) == refl
        starts, counts, rid = a["seg_start"].cpu().numpy(), a["seg_count"].cpu().numpy(), a["row_id"].cpu().numpy()
        assert sorted(rid.tolist()) == list(range(pc.shape[0]))
        if refl:                                                  # the rows are the restatement's selection on the device's own keys
            again, key = ops.cap_subset(**a, return_keys=True)
            key = key.cpu().numpy().view(np.uint32)
            assert torch.equal(again, out) and np.array_equal(out.cpu().numpy(), R.select(a["n"], starts, counts, MAX_PTS, key))
            want = R.race_keys(rid, a["weight"].cpu().numpy(), 77, a["counter"][0], 6)
            inside = np.concatenate([np.arange(s, s + c) for s, c in zip(starts, counts)])
            assert np.abs(key[inside].astype(np.int64) - want[inside].astype(np.int64)).max() <= 1
        else:
            assert np.array_equal(out.cpu().numpy(), R.replace(a["n"], starts, counts, MAX_PTS, 77, 6, rid))
        chosen += list(out.cpu().numpy() - starts[:, None])
        first += counts.tolist()
    assert first == [full[j].shape[0] for j in over]
    for j, (v, f, h) in enumerate(zip(got, full, host)):
        if j not in over:                                         # under the cap: the route without a cap, bit for bit
            assert torch.equal(v, f) and torch.equal(v, h)
            continue
        sel = chosen[over.index(j)]
        assert v.shape == (MAX_PTS, f.shape[1]) and sel.min() >= 0 and sel.max() < f.shape[0]
        assert torch.equal(v, f[torch.from_numpy(sel).to(DEV)])   # rows of the same voxel of the uncapped run
        if refl:
            assert (np.diff(sel) > 0).all()                       # distinct, and in the uncapped voxel's order
    (twice, _), _ = _recorded_voxelise(monkeypatch, pc, cap=PP.DeviceCap(77, counter=6))
    assert all(torch.equal(a, b) for a, b in zip(got, twice))
    (other, _), _ = _recorded_voxelise(monkeypatch, pc, cap=PP.DeviceCap(77, counter=7))
    assert not all(torch.equal(got[j], other[j]) for j in over)


def test_cap_none_with_a_generator_is_the_route_as_it_stands(plots):
    """cap=None takes the per-voxel draws from the generator: torch.multinomial / torch.randint on every oversized voxel, in order."""
    from pointstowood_amd import preprocessing as PP
    for refl in (True, False):
        pc = plots[refl]
        got, _ = PP.voxelise(pc, (4.0,), min_pts=64, max_pts=MAX_PTS, mode="xyz", generator=torch.Generator(device=DEV).manual_seed(5))
        full, _ = PP.voxelise(pc, (4.0,), min_pts=64, max_pts=100000, mode="xyz")
        pos = PP.ground_normalise(pc.to(torch.float32))
        if refl:
            pos[:, 3] = PP.quantile_normalize_reflectance(pos[:, 3].reshape(-1))
        weight = pos[:, 3] - pos[:, 3].min() + 1e-8
        g = torch.Generator(device=DEV).manual_seed(5)
        for v, f in zip(got, full):
            if f.shape[0] <= MAX_PTS:
                assert torch.equal(v, f)
                continue
            if refl:                                              # the voxel's weights: its (normalised) reflectance column, shifted
                draw = torch.multinomial(f[:, 3] - pos[:, 3].min() + 1e-8, MAX_PTS, generator=g)
            else:
                draw = torch.randint(0, f.shape[0], (MAX_PTS,), generator=g, device=DEV)
            assert torch.equal(v, f[draw])
        assert weight.min() > 0
    with pytest.raises(ValueError):
        PP.voxelise(plots[True], cap=PP.DeviceCap(1), generator=torch.Generator(device=DEV))


def test_a_voxels_sample_does_not_depend_on_the_other_voxels(plots):
    """With reflectance: the positions of the far half of the plot (x above the middle) are permuted among its points - the grid and
    every point's weight stay, the far voxels get other members - and every voxel of the near half keeps its sample.  Without: the far
    points stand at the end of the cloud and are dropped, so the far voxels vanish and the list changes; the near voxels keep theirs."""
    from pointstowood_amd import preprocessing as PP
    cap = PP.DeviceCap(5, counter=1)
    kw = dict(min_pts=64, max_pts=MAX_PTS, mode="xyz", cap=cap)
    pc = plots[True]
    mid = (pc[:, 0].min() + pc[:, 0].max()) / 2
    far = torch.nonzero(pc[:, 0] > mid + 0.5).reshape(-1)
    moved = pc.clone()
    moved[far, :3] = pc[far[torch.randperm(far.numel(), generator=torch.Generator().manual_seed(2)).to(DEV)], :3]
    a, _ = PP.voxelise(pc, GRIDS, **kw)
    b, _ = PP.voxelise(moved, GRIDS, **kw)
    full, _ = PP.voxelise(pc, GRIDS, min_pts=64, max_pts=100000, mode="xyz")         # (a voxel's extent is that of ALL its rows)
    assert len(a) == len(b) == len(full)
    near = [j for j, f in enumerate(full) if f.shape[0] > MAX_PTS and float(f[:, 0].max()) <= float(mid) + 0.5]
    changed = [j for j, f in enumerate(full) if f.shape[0] > MAX_PTS and float(f[:, 0].min()) > float(mid) + 0.5]
    assert len(near) >= 5 and len(changed) >= 5
    assert all(torch.equal(a[j], b[j]) for j in near) and not any(torch.equal(a[j], b[j]) for j in changed)
    # without reflectance
    pc = plots[False]
    is_min = (pc[:, :3] == pc[:, :3].amin(dim=0)).any(dim=1)                        # (the grid's origin stays)
    drop = (pc[:, 0] > mid + 2.0) & ~is_min
    ordered = torch.cat([pc[~drop], pc[drop]])
    a, _ = PP.voxelise(ordered, GRIDS, ground=False, **kw)
    b, _ = PP.voxelise(pc[~drop], GRIDS, ground=False, **kw)
    assert len(b) < len(a) - 10
    by_first = {}
    for v in b:
        by_first.setdefault(tuple(v[0].tolist()), []).append(v)
    full, _ = PP.voxelise(ordered, GRIDS, min_pts=64, max_pts=100000, mode="xyz", ground=False)
    near = [v for v, f in zip(a, full) if f.shape[0] > MAX_PTS and float(f[:, 0].max()) <= float(mid) + 2.0]
    assert len(a) == len(full) and len(near) >= 5
    for v in near:
        assert any(torch.equal(v, u) for u in by_first.get(tuple(v[0].tolist()), []))


def test_segment_plot_with_a_cap_runs_end_to_end():
    from pointstowood_amd import Net
    from pointstowood_amd import preprocessing as PP
    from pointstowood_amd import synthetic_weights as weights
    from pointstowood_amd.pipeline import segment_plot
    from tests.test_host_cpu import _plot
    model = Net(num_classes=1, C=8, k=16)
    model.load_state_dict(weights.synth_state_dict(1, 8, seed=0), strict=True)
    model = model.to(DEV).eval()
    pc = _plot(n=20000, seed=8)[:, :4].cuda()
    out = [segment_plot(pc, model, GRIDS, 64, MAX_PTS, cap=PP.DeviceCap(3)) for _ in range(2)]
    n_z, label, pwood = out[0]
    assert n_z.shape == label.shape == pwood.shape == (20000,) and bool(torch.isfinite(pwood).all())
    assert all(torch.equal(x, y) for x, y in zip(out[0], out[1]))
    with pytest.raises(ValueError):
        segment_plot(pc, model, GRIDS, 64, MAX_PTS, cap=PP.DeviceCap(3), generator=torch.Generator(device=DEV))
