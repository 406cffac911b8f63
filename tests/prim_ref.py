"""A plain reference of the five device-wide primitives every geometry path stands on - the LSD radix sort and the two-level exclusive
scan of ``csrc/p2w_sort.h`` (p2w_sort_pairs_u64, xs_exclusive_scan) and p2w_key_runs / p2w_cell_starts / p2w_cells_nd of
``csrc/p2w_geom.hip`` - with the named cases the kernels are held to.  numpy only: no GPU, nothing of the package under test.

    sort_pairs           np.argsort(kind="stable") on uint64: unsigned order, equal keys keep their input order
    key_runs             (start, count) of every run of equal keys with count >= min_count
    cell_starts          table[c] = number of keys below c, c = 0 .. n_cells (searchsorted; the one large table: cumsum of a bincount)
    scan_model           the exclusive scan the way the kernels split it: 4096-entry tiles, one workgroup over the tile sums in
                         rounds of 8192 with a carry, the add - so that a lost carry or a wrong tile index can be written down
    cells_nd             sum_d trunc((P_d - lo_d) / size) stride_d in individually rounded float32 operations, int64 strides
    interp_bwd           float64 scatter-add of p2w_interp_bwd over a hand-made slot table, with the element-wise bound of
                         tests/test_gpu_ops_backward.py
    SORT_CASES, RUN_CASES, TABLE_CASES, CELLS_CASES, INTERP_CASES
                         name -> builder arguments; sort_case(name) ... interp_case(name) build (seeded, deterministic, cached)

``tests/test_prim_ref_cpu.py`` ties the references to independent restatements and to oracle/preprocess.py, asserts that every case
meets the condition it is named for and names the case that tells each of a list of wrong kernels apart;
``tests/test_gpu_prim_kernels.py`` runs the kernels on every case."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

U64, I64, I32, F32, F64 = np.uint64, np.int64, np.int32, np.float32, np.float64
CELL_NONFINITE = (1 << 63) - 1                                             # P2W_CELL_NONFINITE
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
TILE, RADIX, SCAN_ONE, SCAN_ROUND = 4096, 256, 8192, 8192                  # RS_TILE, RS_RADIX, RS_SCAN_ONE, entries per scan round
EPS = 2.0 ** -23


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the radix sort ----------------------------------------------------------------------------------------------------------------------

def sort_pairs(keys, vals=None):
    """(keys_out, vals_out) of a stable ascending sort of uint64 keys; vals None: the values are 0 .. n-1 (an argsort)."""
    keys = np.asarray(keys, dtype=U64)
    order = np.argsort(keys, kind="stable")
    return keys[order], (order.astype(I32) if vals is None else np.asarray(vals, dtype=I32)[order])


def passes(keys):
    """Digit passes the sort runs: the bytes of the OR of all keys."""
    v = int(np.bitwise_or.reduce(np.asarray(keys, dtype=U64))) if len(keys) else 0
    return (v.bit_length() + 7) // 8


def hist_entries(n):
    """Entries of the [digit][tile] histogram table: up to SCAN_ONE one workgroup scans it in one round, above that two levels."""
    return RADIX * ((max(n, 1) + TILE - 1) // TILE)


SORT_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 131071, 131072, 131073]
SORT_FAMILIES = [f"byte{b}" for b in range(8)] + ["bit63", "zeros", "ones", "allmax", "alternate", "chunk_digit", "lane_digit", "ascending",
                                                   "descending", "alphabet16"]
ALT_A, ALT_B = 0x0123456789ABCDEF, 0x0000000001234567                     # "alternate": A at even positions, the smaller B at odd ones
ALPHABET = [(j * 0x0101010101010101 + (15 - j)) & ((1 << 64) - 1) for j in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 127, 128, 144, 233, 255)]


def _sort_keys(family, n, rng):
    i = np.arange(n, dtype=U64)
    if family.startswith("byte"):                                          # one live byte: passes = b + 1, every lower pass sees digit 0 only
        d = rng.integers(0, 256, n).astype(U64)
        d[0] = 255
        return d << U64(8 * int(family[4:]))
    if family == "bit63":                                                  # about half the keys above 2^63, the others small
        k = rng.integers(0, 1000, n).astype(U64)
        top = rng.random(n) < 0.5
        top[0] = True
        k[top] |= U64(1 << 63) | (rng.integers(0, 1 << 20, int(top.sum())).astype(U64) << U64(8))
        return k
    if family == "zeros":
        return np.zeros(n, dtype=U64)
    if family == "ones":
        return np.ones(n, dtype=U64)
    if family == "allmax":                                                 # the value the scatter pads a partial tile's lanes with
        return np.full(n, (1 << 64) - 1, dtype=U64)
    if family == "alternate":
        return np.where(i % U64(2) == 0, U64(ALT_A), U64(ALT_B))
    r = rng.integers(0, 256, n).astype(U64) << U64(8)                      # a second, random byte: pass 1 sorts what pass 0 left
    if family == "chunk_digit":                                            # every 64-key chunk holds ONE digit in pass 0
        return ((i // U64(64)) * U64(37) + U64(11)) % U64(256) | r
    if family == "lane_digit":                                             # every lane of a chunk holds a DIFFERENT digit in pass 0
        return ((i % U64(64)) * U64(4) + (i // U64(64))) % U64(256) | r
    if family == "ascending":
        return i * U64(0x10001)
    if family == "descending":
        return (i * U64(0x10001))[::-1].copy()
    if family == "alphabet16":                                             # 16 values in runs of 97: stability decides almost every position
        blocks = rng.integers(0, 16, n // 97 + 1)
        return np.asarray(ALPHABET, dtype=U64)[np.repeat(blocks, 97)[:n]]
    raise KeyError(family)


def _sort_vals(n, rng):
    v = rng.integers(INT32_MIN, INT32_MAX, n, endpoint=True).astype(I32)
    v[0] = INT32_MIN
    if n > 1:
        v[n // 2], v[-1] = INT32_MAX, -1
    return v


def _sort_table():
    t = {}
    for fi, fam in enumerate(SORT_FAMILIES):                               # every family at 4097 and at 131 073, once with values, once as argsort
        t[f"{fam}-4097-{'vals' if fi % 2 == 0 else 'arg'}"] = (fam, 4097, fi % 2 == 0)
        t[f"{fam}-131073-{'vals' if fi % 2 == 1 else 'arg'}"] = (fam, 131073, fi % 2 == 1)
    rest = [n for n in SORT_SIZES if n not in (4097, 131073)]
    for si, n in enumerate(rest):                                          # the other sizes: two families each, every family at least once
        for j in range(2):
            fam, with_vals = SORT_FAMILIES[(2 * si + j) % len(SORT_FAMILIES)], (si + j) % 2 == 0
            t[f"{fam}-{n}-{'vals' if with_vals else 'arg'}"] = (fam, n, with_vals)
    return t


SORT_CASES = _sort_table()
SortCase = namedtuple("SortCase", "family n keys vals")


@functools.lru_cache(maxsize=None)
def sort_case(name):
    fam, n, with_vals = SORT_CASES[name]
    rng = _rng(name)
    keys = _sort_keys(fam, n, rng)
    assert keys.dtype == U64 and len(keys) == n
    return SortCase(fam, n, keys, _sort_vals(n, rng) if with_vals else None)


# ---- runs of equal keys -------------------------------------------------------------------------------------------------------------------

def key_runs(keys, min_count):
    """(starts, counts) int32 of the runs of equal keys that hold at least min_count elements, in order."""
    keys = np.asarray(keys, dtype=U64)
    n = len(keys)
    if n == 0:
        return np.zeros(0, dtype=I32), np.zeros(0, dtype=I32)
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    counts = np.diff(np.concatenate([first, [n]]))
    keep = counts >= min_count
    return first[keep].astype(I32), counts[keep].astype(I32)


def _mixed_runs(rng):
    return rng.integers(1, 13, 3000).tolist()                              # counts 1 .. 12, about 19 500 keys


_ENDS = (255, 256, 257, 4095, 4096, 4097, 4098)                            # index the run behind the planted one starts at
RUN_CASES = {                                                              # name -> (run lengths, min_count, key style)
    "single": (lambda r: [1000], 1, "plain"),
    **{f"ones_{n}": ((lambda n: lambda r: [1] * n)(n), 1, "plain") for n in (1, 255, 256, 257, 4096, 4097)},
    "ones_4097_none_kept": (lambda r: [1] * 4097, 2, "plain"),
    "runs_4097_mixed": (lambda r: [1, 2] * 2048 + [2], 2, "plain"),
    **{f"end_{e}": ((lambda e: lambda r: [7, e - 7, 5, 300])(e), 6, "plain") for e in _ENDS},
    "first_dropped_last_kept": (lambda r: [2, 9, 3, 9, 4, 8], 5, "plain"),
    "first_kept_last_dropped": (lambda r: [8, 4, 9, 3, 9, 2], 5, "plain"),
    "min_count_present": (_mixed_runs, 7, "plain"),
    "min_count_above_max": (_mixed_runs, 13, "plain"),
    "min_count_1": (_mixed_runs, 1, "plain"),
    "min_count_0": (_mixed_runs, 0, "plain"),
    "min_count_minus3": (_mixed_runs, -3, "plain"),
    "bit63": (_mixed_runs, 4, "bit63"),
    "nonfinite_tail": (lambda r: [5, 1, 6, 2, 40], 3, "tail"),
}
RunCase = namedtuple("RunCase", "runs keys min_count")


@functools.lru_cache(maxsize=None)
def run_case(name):
    make, min_count, style = RUN_CASES[name]
    runs = np.asarray(make(_rng("mixed" if make is _mixed_runs else name)), dtype=I64)
    ids = np.arange(len(runs), dtype=U64)
    vals = {"plain": ids * U64(5) + U64(3), "bit63": ids * U64(3) + U64(1 << 63), "tail": ids * U64(5) + U64(3)}[style]
    if style == "tail":
        vals[-1] = U64(CELL_NONFINITE)                                     # the run p2w_cells_nd's non-finite rows sort into
    return RunCase(runs, np.repeat(vals, runs), min_count)


# ---- the cell table and the scan under it ------------------------------------------------------------------------------------------------

def cell_starts(keys, n_cells, dense=False):
    """table[c] = number of keys below c, c = 0 .. n_cells, int32.  dense: by an int64 cumsum of a bincount (the one large table)."""
    keys = np.zeros(0, dtype=U64) if keys is None else np.asarray(keys, dtype=U64)
    if not dense:
        return np.searchsorted(keys, np.arange(n_cells + 1, dtype=U64), "left").astype(I32)
    counts = np.bincount(keys[keys < U64(n_cells)].astype(I64), minlength=n_cells + 1)
    return (np.cumsum(counts, dtype=I64) - counts).astype(I32)


def cell_counts(keys, n_cells):
    """What the scan is handed: keys per cell 0 .. n_cells - 1 and a last entry of 0."""
    keys = np.zeros(0, dtype=U64) if keys is None else np.asarray(keys, dtype=U64)
    return np.bincount(keys[keys < U64(n_cells)].astype(I64), minlength=n_cells + 1).astype(I32)


def scan_tiles(n):
    return (n + TILE - 1) // TILE


def scan_model(a, carry=True, shift=12):
    """Exclusive scan of int32 the way xs_exclusive_scan splits it: 4096-entry tiles, the tile sums scanned by one workgroup in rounds
    of 8192 entries with a carry between rounds, entry i += tile_sum_scan[i >> shift].  carry=False and shift=11 are wrong kernels
    (a tile sum read behind the last one counts as 0)."""
    a = np.asarray(a, dtype=I32)
    n, nt = len(a), scan_tiles(len(a))
    pad = np.zeros(nt * TILE, dtype=I32)
    pad[:n] = a
    t = pad.reshape(nt, TILE)
    inc = np.cumsum(t, axis=1, dtype=I32)
    out = (inc - t).reshape(-1)[:n]
    if nt == 1:
        return out
    tsum, ts, c = inc[:, -1], np.zeros(2 * nt + 2, dtype=I32), 0
    for base in range(0, nt, SCAN_ROUND):
        seg = tsum[base:base + SCAN_ROUND]
        ts[base:base + len(seg)] = np.cumsum(seg, dtype=I32) - seg + I32(c)
        if carry:
            c += int(seg.sum())
    return out + ts[np.arange(n, dtype=I32) >> shift]


DEEP_CELLS = SCAN_ROUND * TILE                                             # table of 8192 * 4096 + 1 entries: 8193 tiles, a second scan round
_FAR = [1 << 40, (1 << 63) + 5, (1 << 64) - 1]


def _sparse(n_cells, rng, fill=0.3):
    c = rng.integers(1, 4, n_cells + 1) * (rng.random(n_cells + 1) < fill)
    return {int(i): int(c[i]) for i in np.flatnonzero(c)}


def _run_length_counts(rng):
    runs = list(range(1, 10)) + [(1 << k) + d for k in range(4, 17) for d in (-1, 0, 1)]
    counts, cell = {}, 0
    for r in runs:                                                         # an empty cell behind every second run
        counts[cell] = r
        cell += 1 + (r & 1)
    return counts, cell + 3


def _table_spec(name, rng):
    """(n_cells, {cell: count}, far keys): count[n_cells] = keys EQUAL to n_cells, which belong to no cell like the far ones."""
    if name.startswith("len_"):
        n_cells = int(name[4:]) - 1
        c = _sparse(n_cells, rng)
        c[n_cells] = 2                                                     # (len_1: n_cells = 0, every key is beyond the table)
        if n_cells > 0:
            c[0], c[n_cells - 1] = 1, 3
        return n_cells, c, []
    if name == "deep":
        return DEEP_CELLS, {0: 3, 4095: 2, 4096: 5, 8191 * 4096 + 7: 1, 8192 * 4096 - 1: 4, 8192 * 4096: 2}, []
    if name == "run_lengths":
        c, n_cells = _run_length_counts(rng)
        return n_cells, c, []
    if name == "run_ends_at_n":
        return 700, {3: 2, 350: 1000}, []
    if name == "last_cell":
        return 700, {0: 1, 698: 2, 699: 70}, []
    if name == "keys_at_n_cells":
        return 700, {5: 4, 699: 1, 700: 9}, []
    if name == "keys_far_above":
        return 700, {5: 4, 600: 2}, _FAR
    if name == "no_keys":
        return 5000, {}, []
    raise KeyError(name)


TABLE_CASES = [f"len_{L}" for L in (1, 2, 4095, 4096, 4097, 8192, 8193, 12289)] + ["deep", "run_lengths", "run_ends_at_n", "last_cell",
                                                                                      "keys_at_n_cells", "keys_far_above", "no_keys"]
TableCase = namedtuple("TableCase", "n_cells keys counts")


@functools.lru_cache(maxsize=None)
def table_case(name):
    n_cells, counts, far = _table_spec(name, _rng(name))
    cells = np.asarray(sorted(counts), dtype=U64)
    reps = np.asarray([counts[int(c)] for c in cells], dtype=I64)
    keys = np.concatenate([np.repeat(cells, reps), np.asarray(far, dtype=U64)]).astype(U64)
    assert np.all(keys[1:] >= keys[:-1])
    return TableCase(n_cells, keys if len(keys) else None, counts)


@functools.lru_cache(maxsize=2)
def table_expected(name):
    c = table_case(name)
    return cell_starts(c.keys, c.n_cells, dense=name == "deep")


# ---- n-column cell ids -------------------------------------------------------------------------------------------------------------------

def cells_nd(P, D, ld, size, recip=False, f64=False, read_ld=False, nonfinite_in_min=False):
    """int64 key per row of the float32 table P [n, ld]: columns 0 .. D-1 only, every operation rounded to float32 on its own.  The
    keyword arguments are the wrong kernels of tests/test_prim_ref_cpu.py."""
    P = np.asarray(P, dtype=F32).reshape(-1, ld)
    X = P[:, :ld if read_ld else D]
    s = F32(size)
    ok = np.isfinite(X).all(axis=1)
    out = np.full(len(X), CELL_NONFINITE, dtype=I64)
    inmin = X if nonfinite_in_min else X[ok]
    if not ok.any() or not np.isfinite(inmin).all():
        return out if not nonfinite_in_min else np.where(ok, I64(-1), out)  # (a poisoned minimum: no finite row keeps its key)
    lo, hi = inmin.min(axis=0), inmin.max(axis=0)
    if f64:
        div = lambda d: d.astype(F64) / F64(s)
    elif recip:
        div = lambda d: (d * (F32(1) / s)).astype(F32)
    else:
        div = lambda d: (d / s).astype(F32)
    sub = (lambda a, b: a.astype(F64) - b.astype(F64)) if f64 else (lambda a, b: (a - b).astype(F32))
    cnt = np.trunc(div(sub(hi, lo))).astype(I64) + 1
    stride = np.concatenate([[1], np.cumprod(cnt)[:-1]]).astype(I64)
    out[ok] = (np.trunc(div(sub(X[ok], lo[None]))).astype(I64) * stride[None]).sum(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def planted_values(size, seed=7, draws=1 << 20, top=40.0):
    """Float32 values v in [0, top) from a seeded search: `recip` - trunc(v / size) != trunc(v * (1 / size)) in float32; `f64` -
    trunc(v / size) in float32 != in float64; `exact` - v / size is an integer in float32."""
    rng, s = np.random.default_rng(seed), F32(size)
    e = np.arange(1, int(top / float(s)) - 1, dtype=F32) * s              # the cell boundaries and their float32 neighbours, then random draws
    near = [e]
    for direction in (-np.inf, np.inf):
        x = e
        for _ in range(3):
            x = np.nextafter(x, F32(direction))
            near.append(x)
    v = np.concatenate([rng.permutation(np.concatenate(near)), (rng.random(draws) * top).astype(F32)])
    q = np.trunc(v / s)
    recip = v[q != np.trunc(v * (F32(1) / s))]
    f64 = v[q != np.trunc(v.astype(F64) / F64(s))]
    e = np.arange(1, int(top / float(s)) - 1, dtype=F32) * s
    exact = e[(e / s) == np.trunc(e / s)]
    return recip[:8], f64[:8], exact[::max(1, len(exact) // 8)][:8]


def _planted(size, D, rng):
    rec, f64, exact = planted_values(size)
    col = np.concatenate([[0.0], rec, f64, exact, [39.5]] * 4).astype(F32)  # minimum exactly 0: v - lo = v; every value in four rows
    P = (rng.integers(0, 3, (len(col), D)) * 0.5 - 0.5).astype(F32)        # three values per other column: cells of several rows
    P[:, 0] = col
    return P, D, D, size


def _uniform(n, D, lo, hi, rng):
    return (rng.random((n, D)) * (hi - lo) + lo).astype(F32)


def _cells_spec(name, rng):
    """(P [n, ld], D, ld, size)"""
    if name.startswith("planted_"):
        return _planted(float(name[8:]), {"0.04": 3, "0.1": 2, "0.3": 4}[name[8:]], rng)
    if name == "d1":
        return _uniform(1000, 1, -2.0, 30.0, rng), 1, 1, 0.1
    if name == "d16":
        return _uniform(500, 16, 0.0, 3.0, rng), 16, 16, 0.3              # at most 11 cells per column: 11^16 < 2^62
    if name == "pad_nan":                                                  # ld = D + 3, pad columns NaN / inf: the rows stay finite rows
        P = _uniform(700, 7, -5.0, 5.0, rng)
        P[:, 4:] = np.nan
        P[::3, 5] = np.inf
        return P, 4, 7, 0.1
    if name == "constant_column":
        P = _uniform(600, 3, 0.0, 12.0, rng)
        P[:, 1] = 2.5
        return P, 3, 3, 0.04
    if name == "n1":
        return np.asarray([[1.5, -2.25, 7.0]], dtype=F32), 3, 3, 0.1
    if name == "negative_minima":
        return _uniform(900, 3, -50.0, -10.0, rng), 3, 3, 0.3
    if name == "signed_zero_minimum":
        P = _uniform(400, 2, 0.0, 9.0, rng)
        P[::7, 0], P[3::7, 0], P[5, 1], P[6, 1] = -0.0, 0.0, 0.0, -0.0
        return P, 2, 2, 0.1
    if name in ("nonfinite_rows", "nonfinite_rows_1e30"):
        P = _uniform(2000, 4, 0.0, 20.0, rng)
        bad = rng.permutation(2000)[:300]
        P[bad[:100], 0], P[bad[100:200], 2], P[bad[200:], 3] = np.nan, np.inf, -np.inf
        if name.endswith("1e30"):
            P[bad[::2], 1] = 1e30                                          # a dropped row's finite values must not stretch the grid either
            P[bad[1::4], 1] = -1e30
        return P, 4, 4, 0.1
    if name == "all_nonfinite":
        P = _uniform(300, 3, 0.0, 5.0, rng)
        P[np.arange(300), rng.integers(0, 3, 300)] = np.asarray([np.nan, np.inf, -np.inf], dtype=F32)[np.arange(300) % 3]
        return P, 3, 3, 0.1
    if name == "tail":                                                     # the extremes in the grid-stride tail of the min/max kernel
        n = 131073 + 300
        P = _uniform(n, 2, 10.0, 20.0, rng)
        P[n - 150], P[n - 7] = (1.0, 35.0), (36.0, 0.5)
        return P, 2, 2, 0.3
    raise KeyError(name)


CELLS_CASES = ["planted_0.04", "planted_0.1", "planted_0.3", "d1", "d16", "pad_nan", "constant_column", "n1", "negative_minima",
               "signed_zero_minimum", "nonfinite_rows", "nonfinite_rows_1e30", "all_nonfinite", "tail"]
CellsCase = namedtuple("CellsCase", "P n D ld size")


@functools.lru_cache(maxsize=None)
def cells_case(name):
    P, D, ld, size = _cells_spec(name, _rng(name))
    P = np.ascontiguousarray(P, dtype=F32)
    assert P.shape[1] == ld >= D
    return CellsCase(P, len(P), D, ld, float(F32(size)))


# ---- p2w_interp_bwd over hand-made slot tables ---------------------------------------------------------------------------------------------

INTERP_CASES = ["same_index_twice", "index_out_of_range", "deg_above_kw", "deg_negative"]
InterpCase = namedtuple("InterpCase", "xyzr_c xyzr_f nbr deg kw g ref bound run")


def interp_bwd(xyzr_c, xyzr_f, nbr, deg, g):
    """float64 grad_x [nc, F], the bound (L_j + 8) 2^-23 sum |a| |g| of tests/test_gpu_ops_backward.py and the run lengths L_j: a slot
    s of fine row q counts when s < min(deg[q], kw) and 0 <= nbr[q, s] < nc; a = w / (sum of w over the row's counted slots), w =
    1 / max(d2, 1e-16)."""
    nc, (m, kw) = len(xyzr_c), nbr.shape
    c, f, g = xyzr_c[:, :3].astype(F64), xyzr_f[:, :3].astype(F64), g.astype(F64)
    ref, mag, run = np.zeros((nc, g.shape[1])), np.zeros((nc, g.shape[1])), np.zeros(nc, dtype=I64)
    for q in range(m):
        slots = [int(nbr[q, s]) for s in range(max(0, min(int(deg[q]), kw))) if 0 <= nbr[q, s] < nc]
        d = [c[j] - f[q] for j in slots]
        w = [1.0 / max(float((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), 1e-16) for x in d]
        for j, wj in zip(slots, w):
            ref[j] += wj / sum(w) * g[q]
            mag[j] += wj / sum(w) * np.abs(g[q])
            run[j] += 1
    return ref, (run[:, None] + 8) * EPS * mag, run


@functools.lru_cache(maxsize=None)
def interp_case(name):
    rng = _rng(name)
    nc, m, kw, F = 40, 300, 3, 8
    xyzr_c, xyzr_f = rng.random((nc, 4)).astype(F32), rng.random((m, 4)).astype(F32)
    nbr = rng.integers(0, nc, (m, kw)).astype(I32)
    deg = rng.integers(1, kw + 1, m).astype(I32)
    if name == "same_index_twice":
        nbr[::2, 1], deg[::2] = nbr[::2, 0], kw
        nbr[1::6, 2], deg[1::6] = nbr[1::6, 0], kw
    elif name == "index_out_of_range":
        deg[:] = kw
        nbr[::3, 0], nbr[1::3, 1], nbr[2::9, 2], nbr[5::9, 1] = nc, -1, nc + 5, INT32_MIN
        nbr[7] = (nc, -7, INT32_MAX)                                       # a row without a single slot that counts
    elif name == "deg_above_kw":
        deg[::2], deg[1::4] = kw + 2, INT32_MAX
    elif name == "deg_negative":
        deg[::2], deg[1::4] = -1, INT32_MIN
    else:
        raise KeyError(name)
    g = rng.standard_normal((m, F)).astype(F32)
    return InterpCase(xyzr_c, xyzr_f, nbr, deg, kw, g, *interp_bwd(xyzr_c, xyzr_f, nbr, deg, g))
