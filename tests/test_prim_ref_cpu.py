"""tests/prim_ref.py without a GPU: the plain references of the sort, the scan, the run filter, the cell table and the n-column cell
ids agree with independent restatements (torch.sort, torch.unique_consecutive, Python loops, oracle/preprocess.py), every case of
tests/test_gpu_prim_kernels.py meets the condition it is named for, computed from its data, and a list of wrong kernels - written
here as variants of the reference - each change the answer of a named case, so no GPU test can pass by being vacuous."""
import math

import numpy as np
import pytest
import torch

from oracle import preprocess as OP
from tests import prim_ref as R

U64, I64, I32, F32, F64 = R.U64, R.I64, R.I32, R.F32, R.F64
SORT, RUNS, TABLES, CELLS = sorted(R.SORT_CASES), sorted(R.RUN_CASES), list(R.TABLE_CASES), list(R.CELLS_CASES)
SMALL_TABLES = [t for t in TABLES if t != "deep"]


# ---- the references against independent restatements --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SORT)
def test_sort_reference_agrees_with_torch_and_a_python_sort(name):
    c = R.sort_case(name)
    ko, vo = R.sort_pairs(c.keys, c.vals)
    assert ko.dtype == U64 and vo.dtype == I32 and len(ko) == len(vo) == c.n
    if c.n <= 4097:                                                        # Python's sort is stable and its ints are unbounded
        order = sorted(range(c.n), key=lambda i: int(c.keys[i]))
        assert ko.tolist() == [int(c.keys[i]) for i in order]
        assert vo.tolist() == (order if c.vals is None else [int(c.vals[i]) for i in order])
    if int(c.keys.max()) < 1 << 63:
        tk, ti = torch.sort(torch.from_numpy(c.keys.view(I64)), stable=True)
        assert np.array_equal(tk.numpy().view(U64), ko)
        assert np.array_equal(ti.numpy().astype(I32) if c.vals is None else c.vals[ti.numpy()], vo)


def _loop_runs(keys, min_count):
    starts, counts, i, n = [], [], 0, len(keys)
    while i < n:
        j = i
        while j < n and keys[j] == keys[i]:
            j += 1
        if j - i >= min_count:
            starts.append(i)
            counts.append(j - i)
        i = j
    return starts, counts


@pytest.mark.parametrize("name", RUNS)
def test_key_runs_reference_agrees_with_unique_consecutive_and_a_loop(name):
    c = R.run_case(name)
    s, k = R.key_runs(c.keys, c.min_count)
    assert len(c.keys) == int(c.runs.sum()) and np.all(c.keys[1:] >= c.keys[:-1])
    _, counts = torch.unique_consecutive(torch.from_numpy(c.keys.view(I64)), return_counts=True)
    assert np.array_equal(counts.numpy(), c.runs)                          # the runs are the run-length list the case was built from
    starts = torch.cumsum(counts, 0) - counts
    keep = counts >= c.min_count
    assert np.array_equal(starts[keep].numpy(), s) and np.array_equal(counts[keep].numpy(), k)
    if len(c.keys) <= 5000:
        ls, lk = _loop_runs(c.keys.tolist(), c.min_count)
        assert s.tolist() == ls and k.tolist() == lk
    assert R.key_runs(np.zeros(0, dtype=U64), 1)[0].size == 0


@pytest.mark.parametrize("name", SMALL_TABLES)
def test_cell_table_reference_agrees_with_a_loop_and_the_scan_model(name):
    c = R.table_case(name)
    want = R.table_expected(name)
    assert want.dtype == I32 and len(want) == c.n_cells + 1
    keys = [] if c.keys is None else c.keys.tolist()
    loop, p = [], 0
    for cell in range(c.n_cells + 1):
        while p < len(keys) and keys[p] < cell:
            p += 1
        loop.append(p)
    assert want.tolist() == loop
    assert np.array_equal(R.cell_starts(c.keys, c.n_cells, dense=True), want)
    assert np.array_equal(R.scan_model(R.cell_counts(c.keys, c.n_cells)), want)


def test_deep_table_reference_agrees_with_searchsorted_and_the_scan_model():
    c, want = R.table_case("deep"), R.table_expected("deep")
    assert len(want) == 8192 * 4096 + 1 and want[0] == 0 and int(want[-1]) == int((c.keys < U64(c.n_cells)).sum()) == 15
    probe = np.unique(np.concatenate([[0, 1, c.n_cells - 1, c.n_cells], *[[k - 1, k, k + 1] for k in c.counts if 0 < k < c.n_cells]]))
    assert np.array_equal(want[probe], np.searchsorted(c.keys, probe.astype(U64), "left"))
    assert np.array_equal(R.scan_model(R.cell_counts(c.keys, c.n_cells)), want)


def _oracle_cells(c):
    return OP.cells_nd(torch.from_numpy(c.P[:, :c.D].copy()), c.size).numpy()


@pytest.mark.parametrize("name", CELLS)
def test_cells_reference_equals_the_oracle_bit_for_bit(name):
    c = R.cells_case(name)
    got = R.cells_nd(c.P, c.D, c.ld, c.size)
    assert got.dtype == I64 and np.array_equal(got, _oracle_cells(c))


# ---- every case meets the condition it is named for -----------------------------------------------------------------------------------------

def test_sort_cases_cover_the_sizes_the_families_and_every_pass_count():
    table = R.SORT_CASES
    assert {n for _, n, _ in table.values()} == set(R.SORT_SIZES)
    for n in (4097, 131073):                                               # every family at a partial tile and above the scan switch
        assert {f for f, m, _ in table.values() if m == n} == set(R.SORT_FAMILIES)
        assert {R.passes(R.sort_case(k).keys) for k, v in table.items() if v[1] == n} == set(range(9))
    assert {f for f, _, _ in table.values()} == set(R.SORT_FAMILIES)
    for fam in R.SORT_FAMILIES:                                            # given values and vals_in = NULL, both
        assert {w for f, _, w in table.values() if f == fam} == {True, False}
    # the scan switch: 256 * ceil(n / 4096) against 8192 - the last one-level size is 131 072 keys
    assert R.hist_entries(131071) == R.hist_entries(131072) == R.SCAN_ONE and R.hist_entries(131073) == R.SCAN_ONE + 256
    assert all(R.hist_entries(n) <= R.SCAN_ONE for n in R.SORT_SIZES if n <= 131072)
    # the last tile's fill, a wave's 1024 keys, a 64-key chunk
    assert {n % R.TILE for n in R.SORT_SIZES} >= {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095}


@pytest.mark.parametrize("name", SORT)
def test_sort_case_is_what_its_family_says(name):
    c = R.sort_case(name)
    fam, n, k, P = c.family, c.n, c.keys, R.passes(c.keys)
    chunks = [k[i:i + 64] & U64(255) for i in range(0, n, 64)]
    if fam.startswith("byte"):
        b = int(fam[4:])
        assert P == b + 1 and not np.any(k & U64((1 << 8 * b) - 1)) and not np.any(k >> U64(8 * b + 8))
    elif fam == "bit63":
        top = (k >> U64(63)).astype(bool)
        assert P == 8 and top.any() and (n < 63 or 0.3 < top.mean() < 0.7) and int(k[~top].max(initial=0)) < 1000
    elif fam in ("zeros", "ones", "allmax"):
        assert np.all(k == k[0]) and int(k[0]) == {"zeros": 0, "ones": 1, "allmax": (1 << 64) - 1}[fam] and P == {"zeros": 0, "ones": 1, "allmax": 8}[fam]
    elif fam == "alternate":
        assert set(k.tolist()) <= {R.ALT_A, R.ALT_B} and (n < 2 or (k[0] > k[1] and len(set(k.tolist())) == 2)) and P == 8
    elif fam == "chunk_digit":
        assert all(len(set(ch.tolist())) == 1 for ch in chunks) and (n < 4096 or len({int(ch[0]) for ch in chunks}) > 32) and P <= 2
    elif fam == "lane_digit":
        assert all(len(set(ch.tolist())) == len(ch) for ch in chunks) and P <= 2
    elif fam == "ascending":
        assert np.all(k[1:] > k[:-1]) and P == R.passes(np.asarray([(n - 1) * 0x10001], dtype=U64))
    elif fam == "descending":
        assert np.all(k[1:] < k[:-1])
    elif fam == "alphabet16":
        assert set(k.tolist()) <= set(R.ALPHABET) and (n < 4096 or len(set(k.tolist())) == 16) and P == 8
        if n >= 1023:                                                      # stability decides almost every position
            assert np.mean(_unstable(k, None)[1] != R.sort_pairs(k, None)[1]) > 0.9
    if c.vals is not None:
        assert c.vals[0] == R.INT32_MIN and (n < 3 or (R.INT32_MAX in c.vals and (c.vals < 0).sum() > 1))


@pytest.mark.parametrize("name", RUNS)
def test_run_case_is_what_its_name_says(name):
    c = R.run_case(name)
    runs, mc = c.runs, c.min_count
    starts = np.cumsum(runs) - runs
    s, k = R.key_runs(c.keys, mc)
    if name.startswith("ones_"):
        assert len(runs) == int(name.split("_")[1]) == len(c.keys)
        assert len(s) == (0 if name.endswith("none_kept") else len(runs))
    if name == "runs_4097_mixed":
        assert len(runs) == 4097 and len(s) == 2049                        # the keep flags' scan crosses its tile too
    if name.startswith("end_"):
        e = int(name[4:])
        assert e in starts and e - 1 == starts[2] - 1 and len(s) == 3 and runs[2] == mc - 1 and runs[0] == mc + 1
    if name == "first_dropped_last_kept":
        assert runs[0] < mc <= runs[-1] and s[-1] == starts[-1]
    if name == "first_kept_last_dropped":
        assert runs[-1] < mc <= runs[0] and s[0] == 0 and s[-1] != starts[-1]
    if name == "min_count_present":
        assert mc in runs and mc - 1 in runs and 0 < len(s) < len(runs)
    if name == "min_count_above_max":
        assert mc == runs.max() + 1 and len(s) == 0
    if name in ("min_count_1", "min_count_0", "min_count_minus3"):
        assert mc == {"1": 1, "0": 0, "minus3": -3}[name.split("_")[2]] and len(s) == len(runs) and 1 in runs
    if name == "bit63":
        assert np.all(c.keys >> U64(63) == 1) and 0 < len(s) < len(runs)
    if name == "nonfinite_tail":
        assert int(c.keys[-1]) == R.CELL_NONFINITE and int((c.keys == U64(R.CELL_NONFINITE)).sum()) == runs[-1] >= mc


@pytest.mark.parametrize("name", TABLES)
def test_table_case_is_what_its_name_says(name):
    c = R.table_case(name)
    tiles = R.scan_tiles(c.n_cells + 1)
    if name.startswith("len_"):
        L = int(name[4:])
        assert c.n_cells + 1 == L and tiles == {1: 1, 2: 1, 4095: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 12289: 4}[L]
        assert (c.keys == U64(c.n_cells)).sum() == 2 and (L == 1 or (c.keys == U64(c.n_cells - 1)).any())
    if name == "deep":
        assert c.n_cells + 1 == 8192 * 4096 + 1 and tiles == 8193 > R.SCAN_ROUND      # the tile sums take a second round, with a carry
        assert sorted(c.counts) == [0, 4095, 4096, 8191 * 4096 + 7, 8192 * 4096 - 1, 8192 * 4096]
        assert sum(v for k, v in c.counts.items() if k < 8192 * 4096) > 0 and c.counts[8192 * 4096 - 1] > 0   # a non-zero carry, used
    if name == "run_lengths":
        runs = set(np.unique(c.keys, return_counts=True)[1].tolist())
        assert runs == set(range(1, 10)) | {(1 << k) + d for k in range(4, 17) for d in (-1, 0, 1)}
    if name == "run_ends_at_n":
        assert int(c.keys[-1]) < c.n_cells - 1 and (c.keys == c.keys[-1]).sum() == 1000
    if name == "last_cell":
        assert int(c.keys.max()) == c.n_cells - 1
    if name == "keys_at_n_cells":
        assert int(c.keys.max()) == c.n_cells and (c.keys == U64(c.n_cells)).sum() == 9
    if name == "keys_far_above":
        assert (c.keys > U64(c.n_cells)).sum() == 3 and int(c.keys[-1]) == (1 << 64) - 1 and not (c.keys == U64(c.n_cells)).any()
    if name == "no_keys":
        assert c.keys is None and not R.table_expected(name).any()
    assert 0 <= c.n_cells < (1 << 31) - 1


@pytest.mark.parametrize("name", CELLS)
def test_cells_case_is_what_its_name_says(name):
    c = R.cells_case(name)
    X, s = c.P[:, :c.D], F32(c.size)
    ok = np.isfinite(X).all(axis=1)
    key = R.cells_nd(c.P, c.D, c.ld, c.size)
    assert c.P.shape == (c.n, c.ld) and 1 <= c.D <= 16
    assert name == "n1" or math.frexp(c.size)[0] != 0.5                    # no power of two: the quotients round
    if ok.any():                                                           # the ranges the cast is defined on
        lo, hi = X[ok].min(0), X[ok].max(0)
        cnt = np.trunc((hi - lo) / s).astype(F64) + 1
        assert cnt.max() < 2.0 ** 31 and float(np.prod(cnt)) < 2.0 ** 62 and np.all(key[ok] >= 0)
    assert np.all(key[~ok] == R.CELL_NONFINITE) and np.all(key[ok] != R.CELL_NONFINITE)
    if name.startswith("planted_"):
        v = X[:, 0]
        q = np.trunc(v / s)
        assert X[:, 0].min() == 0 and np.signbit(X[:, 0].min()) == False   # noqa: E712  v - lo is v
        assert (q != np.trunc(v * (F32(1) / s))).sum() >= 4                # rows a reciprocal multiply truncates differently
        assert (q != np.trunc(v.astype(F64) / F64(s))).sum() >= 4          # rows a float64 quotient truncates differently
        assert ((v / s) == q).sum() >= 5                                   # rows whose float32 quotient is an exact integer
        rec, f64, exact = R.planted_values(c.size)
        assert len(rec) >= 4 and len(f64) >= 4 and len(exact) >= 4 and set(np.concatenate([rec, f64, exact]).tolist()) <= set(v.tolist())
    if name == "d1":
        assert c.D == 1
    if name == "d16":
        assert c.D == 16
    if name == "pad_nan":
        assert c.ld == c.D + 3 and not np.isfinite(c.P[:, c.D:]).any() and np.isnan(c.P[:, c.D]).all() and ok.all()
    if name == "constant_column":
        assert np.all(X[:, 1] == X[0, 1])
    if name == "n1":
        assert c.n == 1 and key[0] == 0
    if name == "negative_minima":
        assert np.all(X.max(0) < 0)
    if name == "signed_zero_minimum":
        z = X[:, 0] == 0
        assert X.min() == 0 and np.signbit(X[z, 0]).any() and not np.signbit(X[z, 0]).all() and np.signbit(X[X[:, 1] == 0, 1]).any()
    if name.startswith("nonfinite_rows"):
        bad = ~ok
        assert bad.sum() == 300 and np.isnan(X[bad]).any() and np.isposinf(X[bad]).any() and np.isneginf(X[bad]).any()
        assert (np.isfinite(X[bad]).sum(axis=1) == c.D - 1).all()          # one column each
        assert (np.abs(X[bad]) == F32(1e30)).any() == name.endswith("1e30") and np.abs(X[ok]).max() < 100
    if name == "all_nonfinite":
        assert not ok.any() and np.all(key == R.CELL_NONFINITE)
    if name == "tail":
        assert c.n == 131073 + 300 and min(X.argmin(0).min(), X.argmax(0).min()) >= 131073   # beyond 512 blocks of 256 rows


@pytest.mark.parametrize("name", R.INTERP_CASES)
def test_interp_table_is_what_its_name_says(name):
    c = R.interp_case(name)
    nc, kw, d = len(c.xyzr_c), c.kw, np.clip(c.deg, 0, c.kw)
    used = np.arange(kw)[None] < d[:, None]
    if name == "same_index_twice":
        assert ((c.nbr[:, 0] == c.nbr[:, 1]) & (d >= 2)).sum() > 100
    if name == "index_out_of_range":
        bad = ((c.nbr < 0) | (c.nbr >= nc)) & used
        assert (c.nbr[used] == nc).any() and (c.nbr[used] < 0).any() and (c.nbr[used] > nc).any() and bad.all(axis=1).any()
    if name == "deg_above_kw":
        assert (c.deg > kw).sum() > 100 and c.deg.max() == R.INT32_MAX
    if name == "deg_negative":
        assert (c.deg < 0).sum() > 100 and c.deg.min() == R.INT32_MIN
    assert int(c.run.sum()) == int((used & (c.nbr >= 0) & (c.nbr < nc)).sum()) and (c.run == 0).sum() >= 0 and np.all(c.bound >= 0)
    assert c.ref.shape == (nc, c.g.shape[1]) and np.abs(c.ref).max() > 0.1


# ---- wrong kernels, as variants of the reference: each changes a named case -------------------------------------------------------------------

def _unstable(keys, vals):
    order = np.lexsort((-np.arange(len(keys)), keys))                      # equal keys in REVERSE input order
    return keys[order], (order.astype(I32) if vals is None else vals[order])


def _signed(keys, vals):
    order = np.argsort(keys.view(I64), kind="stable")
    return keys[order], (order.astype(I32) if vals is None else vals[order])


def _seven_bytes(keys, vals):
    order = np.argsort(keys & U64((1 << 56) - 1), kind="stable")
    return keys[order], (order.astype(I32) if vals is None else vals[order])


def _runs_greater(keys, mc):
    return R.key_runs(keys, mc + 1)


def _runs_without_the_last(keys, mc):
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    counts = np.diff(first)                                                # the run that ends at n is never closed
    keep = counts >= mc
    return first[:-1][keep].astype(I32), counts[keep].astype(I32)


def _changed(cases, build, ref, wrong):
    out = set()
    for name in cases:
        a, b = ref(build(name)), wrong(build(name))
        if any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b)):
            out.add(name)
    return out


SORT_VARIANTS = [("unstable", _unstable, {"alphabet16-4097-arg", "alphabet16-131073-vals", "zeros-4097-arg", "alternate-131073-arg"}),
                 ("signed order", _signed, {"bit63-4097-vals", "bit63-131073-arg"}),
                 ("drops the top byte", _seven_bytes, {"byte7-4097-arg", "byte7-131073-vals"})]


@pytest.mark.parametrize("what,wrong,named", SORT_VARIANTS, ids=[v[0] for v in SORT_VARIANTS])
def test_wrong_sorts_change_named_cases(what, wrong, named):
    changed = _changed(SORT, R.sort_case, lambda c: R.sort_pairs(c.keys, c.vals), lambda c: wrong(c.keys, c.vals))
    assert named <= changed, (what, named - changed)
    if what != "unstable":
        assert all(k.startswith(("bit63", "byte7", "allmax", "alternate", "alphabet16")) for k in changed), changed


def test_wrong_run_filters_change_named_cases():
    ref = lambda c: R.key_runs(c.keys, c.min_count)
    greater = _changed(RUNS, R.run_case, ref, lambda c: _runs_greater(c.keys, c.min_count))
    assert {"min_count_present", "min_count_1", "ones_4097", "runs_4097_mixed"} <= greater
    assert "min_count_above_max" not in greater and "min_count_0" not in greater     # (nothing at the threshold there)
    no_last = _changed(RUNS, R.run_case, ref, lambda c: _runs_without_the_last(c.keys, c.min_count))
    assert {"single", "ones_1", "ones_4096", "first_dropped_last_kept", "nonfinite_tail", "end_4096"} <= no_last
    assert "first_kept_last_dropped" not in no_last                        # (its last run is dropped anyway)


def test_wrong_scans_and_tables_change_named_cases():
    small = {n: R.cell_counts(R.table_case(n).keys, R.table_case(n).n_cells) for n in SMALL_TABLES}
    no_carry = {n for n, a in small.items() if not np.array_equal(R.scan_model(a, carry=False), R.table_expected(n))}
    assert no_carry == set()                                               # no table below 8192 * 4096 entries sees a second round
    shift = {n for n, a in small.items() if not np.array_equal(R.scan_model(a, shift=11), R.table_expected(n))}
    assert {"len_4097", "len_8192", "len_8193", "len_12289"} <= shift and "len_4096" not in shift
    deep = R.cell_counts(R.table_case("deep").keys, R.DEEP_CELLS)
    want = R.table_expected("deep")
    lost = R.scan_model(deep, carry=False)
    assert not np.array_equal(lost, want) and np.array_equal(lost[:8192 * 4096], want[:8192 * 4096]) and lost[-1] == 0 and want[-1] == 15
    assert not np.array_equal(R.scan_model(deep, shift=11), want)
    le = {n for n in SMALL_TABLES if not np.array_equal(np.searchsorted(np.zeros(0, dtype=U64) if R.table_case(n).keys is None else R.table_case(n).keys,
                                                                       np.arange(R.table_case(n).n_cells + 1, dtype=U64), "right"), R.table_expected(n))}
    assert {"len_2", "len_4097", "run_lengths", "run_ends_at_n", "last_cell", "keys_at_n_cells"} <= le and "no_keys" not in le


CELL_VARIANTS = [("recip", {"planted_0.04", "planted_0.1", "planted_0.3"}), ("f64", {"planted_0.04", "planted_0.1", "planted_0.3"}),
                 ("read_ld", {"pad_nan"}), ("nonfinite_in_min", {"nonfinite_rows", "nonfinite_rows_1e30"})]


@pytest.mark.parametrize("flag,named", CELL_VARIANTS, ids=[v[0] for v in CELL_VARIANTS])
def test_wrong_cell_kernels_change_named_cases(flag, named):
    def key(n, **kw):
        c = R.cells_case(n)
        return R.cells_nd(c.P, c.D, c.ld, c.size, **kw)
    changed = {n for n in CELLS if not np.array_equal(key(n, **{flag: True}), key(n))}
    assert named <= changed, (flag, named - changed)
    if flag == "read_ld":
        assert changed == {"pad_nan"}
    if flag == "nonfinite_in_min":
        assert "all_nonfinite" not in changed and "tail" not in changed
