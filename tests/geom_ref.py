"""A plain reference of the geometry half of ``include/p2w.h`` (``csrc/p2w_geom.hip``): numpy and the standard library only, written
from the header's comments and from nothing of the package under test.  Every float32 operation is a numpy float32 operation of its
own (individually rounded); where a case has to be classified the arithmetic is redone in ``fractions.Fraction``.

    d2 / exact_d2        ((dx*dx)+(dy*dy))+(dz*dz) in float32, and the wrong forms a compiler or a rewrite could produce
    knn / ball           ascending (bits(d2), carried index), deg = min(k, admitted); the `cap` lowest carried indices with
                         d2 < float32(float64(r)*float64(r)), -1 behind them; both *_IN_W flags
    sample               the sampler: every output of p2w_voxel_sample[_table], the 56-byte p2w_grid and the cell-start tables
    gather               the float32 (p / sf) * sf round trip of p2w_level_gather
    knn_hint2            the rule of p2w_knn_hint2
    tile_bbox            the box of each run of 1024 consecutive records, numbered voxel by voxel
    SEARCH / SAMPLER     named, seeded cases of tests/test_gpu_geom_kernels.py: name -> () -> Search / Sampling

``tests/test_geom_ref_cpu.py`` ties it to ``oracle/ops.py``, asserts that every case meets the condition it is named for and that the
cases tell a list of wrong kernels (the ``form=``, ``strict=``, ``tie=``, ``cells=`` ... arguments below) apart."""
from __future__ import annotations

import functools
import struct
import zlib
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

F = np.float32
X_INDEX_IN_W, Q_ROW_IN_W, BOX = 1, 2, 4                                    # P2W_SEARCH_*
TILE = 1024                                                                # records per tile box (P2W_SAMPLE_TILE's namesake S_TILE)
SENTINEL = -0x01234567                                                     # what the GPU file fills nbr / deg with before a call
_BIG = np.int64(0x7FFFFFFFFFFFFFFF)
INF = F(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def below(v):
    return np.nextafter(F(v), F(-np.inf))


def above(v):
    return np.nextafter(F(v), F(np.inf))


def r2_of(r):
    """float32(float64(r) * float64(r)): the header's (float)(r*r) with r a double."""
    return F(float(r) * float(r))


def r2_f32(r):
    """The wrong one: float32(r) squared in float32."""
    return F(r) * F(r)


def as_w(i):
    """int32 values as the float32 bit patterns that travel in a record's .w"""
    return np.ascontiguousarray(i, dtype=np.int32).view(F)


def records(xyz, w):
    out = np.empty((len(xyz), 4), F)
    out[:, :3] = xyz
    out[:, 3] = as_w(w)
    return out


# ---- distances -------------------------------------------------------------------------------------------------------------------------

FORMS = ("sum", "fma_xy", "fma_z", "reassoc", "f64")


def _combine(dx, dy, dz, form):
    if form == "sum":                                                      # the contract
        return ((dx * dx) + (dy * dy)) + (dz * dz)
    if form == "reassoc":                                                  # dx*dx + (dy*dy + dz*dz)
        return (dx * dx) + ((dy * dy) + (dz * dz))
    x, y, z = (np.asarray(v, np.float64) for v in (dx, dy, dz))
    if form == "fma_xy":                                                   # fma(dz, dz, fma(dy, dy, dx*dx)); float64 holds dy*dy exactly, the
        a = (y * y + (dx * dx).astype(np.float64)).astype(F)               # sum is rounded twice: planted pairs are re-checked in exact_d2
        return (z * z + a.astype(np.float64)).astype(F)
    if form == "fma_z":                                                    # fma(dz, dz, dx*dx + dy*dy): only the outer sum contracted
        return (z * z + ((dx * dx) + (dy * dy)).astype(np.float64)).astype(F)
    raise ValueError(form)


def d2(q, x, form="sum"):
    """[m, n] squared distances of the float32 rows q [m, >= 3] and x [n, >= 3]."""
    q, x = np.asarray(q, F), np.asarray(x, F)
    if form == "f64":
        d = q[:, None, :3].astype(np.float64) - x[None, :, :3].astype(np.float64)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return _combine(q[:, None, 0] - x[None, :, 0], q[:, None, 1] - x[None, :, 1], q[:, None, 2] - x[None, :, 2], form)


def d2_rows(q, x, form="sum"):
    """[m] squared distances of matching rows."""
    q, x = np.asarray(q, F), np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return _combine(q[:, 0] - x[:, 0], q[:, 1] - x[:, 1], q[:, 2] - x[:, 2], form)


def rnd32(fr):
    """The float32 nearest to a Fraction (ties to even, normal range), as a Fraction."""
    fr = Fraction(fr)
    if fr == 0:
        return fr
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    assert -126 <= e <= 127
    scale = Fraction(2) ** (23 - e)
    m = a * scale
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return (n / scale) * (1 if fr > 0 else -1)


def exact_d2(q, c, form="sum"):
    """The same forms on one pair, every rounding done in rational arithmetic: (float32 result as a Fraction; form "f64": the true
    squared distance of the float32 coordinates, unrounded)."""
    d = [Fraction(float(F(a))) - Fraction(float(F(b))) for a, b in zip(q[:3], c[:3])]
    if form == "f64":
        return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    dx, dy, dz = (rnd32(v) for v in d)
    if form == "sum":
        return rnd32(rnd32(rnd32(dx * dx) + rnd32(dy * dy)) + rnd32(dz * dz))
    if form == "reassoc":
        return rnd32(rnd32(dx * dx) + rnd32(rnd32(dy * dy) + rnd32(dz * dz)))
    if form == "fma_xy":
        return rnd32(dz * dz + rnd32(dy * dy + rnd32(dx * dx)))
    if form == "fma_z":
        return rnd32(dz * dz + rnd32(rnd32(dx * dx) + rnd32(dy * dy)))
    raise ValueError(form)


# ---- searches --------------------------------------------------------------------------------------------------------------------------

def _carried(x, flags):
    return x[:, 3].view(np.int32).astype(np.int64) if flags & X_INDEX_IN_W else np.arange(len(x), dtype=np.int64)


def _queries(x, q, qidx, ptr_q):
    m = int(ptr_q[-1])
    src = x if q is None else q
    return (src[np.asarray(qidx[:m], np.int64)] if qidx is not None else src[:m]), m


def _rows(qq, m, flags):
    return qq[:, 3].view(np.int32).astype(np.int64) if flags & Q_ROW_IN_W else np.arange(m, dtype=np.int64)


def knn(x, ptr_x, q, ptr_q, k, flags=0, qidx=None, rows=None, form="sum", tie="carried"):
    """(nbr [rows, k], deg [rows]) int32; rows that no query writes keep SENTINEL.  q None: the queries are x[qidx].
    tie="storage": the wrong kernel that breaks ties by storage position and reports the carried index."""
    qq, m = _queries(x, q, qidx, ptr_q)
    rows = max(rows or 0, m)
    nbr, deg = np.full((rows, k), SENTINEL, np.int32), np.full(rows, SENTINEL, np.int32)
    car, row = _carried(x, flags), _rows(qq, m, flags)
    for b in range(len(ptr_q) - 1):
        q0, q1, c0, c1 = int(ptr_q[b]), int(ptr_q[b + 1]), int(ptr_x[b]), int(ptr_x[b + 1])
        if q1 == q0:
            continue
        out, dg = np.full((q1 - q0, k), -1, np.int32), np.zeros(q1 - q0, np.int32)
        if c1 > c0:
            D = d2(qq[q0:q1], x[c0:c1], form)
            hi = bits(D).astype(np.int64)                                  # (form "f64" is for the ball predicate only)
            low = car[c0:c1] if tie == "carried" else np.arange(c0, c1, dtype=np.int64)
            key = np.where(np.isnan(D), _BIG, (hi << 32) | low[None, :])
            kk = min(k, c1 - c0)
            sel = np.argsort(key, axis=1, kind="stable")[:, :kk]
            ok = np.take_along_axis(key, sel, 1) != _BIG
            out[:, :kk] = np.where(ok, car[c0:c1][sel], -1)
            dg = ok.sum(1).astype(np.int32)
        nbr[row[q0:q1]], deg[row[q0:q1]] = out, dg
    return nbr, deg


def ball(x, ptr_x, q, ptr_q, r, cap, flags=0, qidx=None, rows=None, form="sum", strict=True, r2=None, first="carried"):
    """(nbr [rows, cap], deg [rows]).  first="storage": the wrong kernel that keeps the first `cap` hits in storage order."""
    qq, m = _queries(x, q, qidx, ptr_q)
    rows = max(rows or 0, m)
    nbr, deg = np.full((rows, cap), SENTINEL, np.int32), np.full(rows, SENTINEL, np.int32)
    car, row = _carried(x, flags), _rows(qq, m, flags)
    r2 = r2_of(r) if r2 is None else r2
    for b in range(len(ptr_q) - 1):
        q0, q1, c0, c1 = int(ptr_q[b]), int(ptr_q[b + 1]), int(ptr_x[b]), int(ptr_x[b + 1])
        if q1 == q0:
            continue
        out, dg = np.full((q1 - q0, cap), -1, np.int32), np.zeros(q1 - q0, np.int32)
        if c1 > c0:
            D = d2(qq[q0:q1], x[c0:c1], form)
            with np.errstate(invalid="ignore"):
                hit = (D < r2) if strict else (D <= r2)
            if first == "storage":
                hit &= np.cumsum(hit, axis=1) <= cap
            key = np.where(hit, car[c0:c1][None, :], _BIG)
            cc = min(cap, c1 - c0)
            sel = np.sort(key, axis=1)[:, :cc]
            out[:, :cc] = np.where(sel != _BIG, sel, -1)
            dg = np.minimum(hit.sum(1), cap).astype(np.int32)
        nbr[row[q0:q1]], deg[row[q0:q1]] = out, dg
    return nbr, deg


def kth_d2(x, ptr_x, q, ptr_q, k):
    """[m] float32: the d2 of every query's k-th neighbour (the last one where the voxel holds fewer), +inf for an empty voxel."""
    out = np.full(int(ptr_q[-1]), INF, F)
    for b in range(len(ptr_q) - 1):
        q0, q1, c0, c1 = int(ptr_q[b]), int(ptr_q[b + 1]), int(ptr_x[b]), int(ptr_x[b + 1])
        if q1 > q0 and c1 > c0:
            out[q0:q1] = np.sort(d2(q[q0:q1], x[c0:c1]), axis=1)[:, min(k, c1 - c0) - 1]
    return out


def tile_bbox(x, ptr, rows):
    """[rows, 6] float32 (lo xyz, hi xyz) of every run of TILE consecutive records of a voxel, voxel by voxel; unused rows NaN."""
    out = np.full((rows, 6), np.nan, F)
    t = 0
    for b in range(len(ptr) - 1):
        for s in range(int(ptr[b]), int(ptr[b + 1]), TILE):
            run = x[s:min(s + TILE, int(ptr[b + 1])), :3]
            out[t, :3], out[t, 3:] = run.min(0), run.max(0)
            t += 1
    return out


def box_gap2(box6, p):
    e = [np.maximum(np.maximum(F(box6[a]) - F(p[a]), F(p[a]) - F(box6[a + 3])), F(0)) for a in range(3)]
    return ((e[0] * e[0]) + (e[1] * e[1])) + (e[2] * e[2])


def knn_hint2(q, rank, ptr_q, xc, cross=False, d1_only=False):
    """hint [m] float32: d1 = d2 to the own representative xc[rank[i]]; d2nd = the smallest d2 to the representatives rank[i +- s],
    s = 1 .. 8, that differ from the own one, positions inside the query's voxel only, stopping after the first s >= 2 at which one has
    been seen; hint = max(d1, d2nd), +inf where there is none.  cross / d1_only: the wrong kernels."""
    m = int(ptr_q[-1])
    i = np.arange(m)
    b = np.searchsorted(np.asarray(ptr_q), i, "right") - 1
    lo, hi = (np.zeros(m, np.int64), np.full(m, m)) if cross else (np.asarray(ptr_q)[b], np.asarray(ptr_q)[b + 1])
    own = np.asarray(rank[:m], np.int64)
    d1 = d2_rows(q[:m], xc[own])
    if d1_only:
        return d1
    second, done = np.full(m, INF, F), np.zeros(m, bool)
    for s in range(1, 9):
        for j in (i + s, i - s):
            ok = (j < hi) & (j >= lo) & ~done
            c = np.asarray(rank, np.int64)[np.clip(j, 0, m - 1)]
            ok &= c != own
            second = np.where(ok, np.minimum(second, d2_rows(q[:m], xc[np.where(ok, c, own)])), second)
        if s >= 2:
            done |= second < INF
    return np.maximum(d1, second)


def gather(src, idx, batch, sf):
    """p2w_level_gather: ((p / sf_b) * sf_b, w) of src[idx[i]] in float32."""
    out = np.array(src[np.asarray(idx, np.int64)], F)
    s = np.asarray(sf, F)[np.asarray(batch, np.int64)][:, None]
    out[:, :3] = (out[:, :3] / s) * s
    return out


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------

@dataclass
class Sampled:
    lo: np.ndarray
    hi: np.ndarray
    dims: np.ndarray          # [3] int64
    b_lo: int
    T: int                    # cells of the table sampler's grid: dims product x (last - first non-empty voxel + 1); 2^62 beyond 2^20 per axis
    keys: np.ndarray          # [n] uint64, point order
    order: np.ndarray         # [n] int32: a stable ascending-key permutation
    sorted_keys: np.ndarray   # [n] uint64
    cell_keys: np.ndarray     # [M] uint64
    idx: np.ndarray           # [M] int32
    ptr: np.ndarray           # [B + 1] int32
    batch: np.ndarray         # [M] int32
    inv: np.ndarray           # [n] int32
    rank_sorted: np.ndarray   # [n] int32
    grid: np.ndarray          # [56] uint8

    def cell_start(self):
        return cell_starts(self.cell_keys, self.T)

    def cell_start_sorted(self):
        return cell_starts(self.sorted_keys, self.T)


def cell_starts(keys_sorted, T):
    """[T + 1] int32: for every key t <= T the position of the first element with key >= t."""
    return np.searchsorted(np.asarray(keys_sorted, np.uint64), np.arange(T + 1, dtype=np.uint64), "left").astype(np.int32)


def grid_image(lo, res, hi, b_lo, dims):
    return np.frombuffer(struct.pack("<3ff3fi3q", *map(float, lo), float(res), *map(float, hi), int(b_lo), *map(int, dims)), np.uint8).copy()


def sample(xyzr, ptr, res, cells="div", rep="max", plus1=True):
    """The sampler on the first ptr[B] >= 1 records.  cells: "div" the contract (float32 subtract, float32 divide, truncate), "mul" a
    multiplication by float32(1 / res), "f64" the quotient in float64; rep="min" and plus1=False: two more wrong kernels."""
    ptr = np.asarray(ptr, np.int64)
    n, B = int(ptr[-1]), len(ptr) - 1
    p, res = np.asarray(xyzr, F)[:n, :3], F(res)
    lo, hi = p.min(0), p.max(0)
    dims = ((hi - lo) / res).astype(np.int64) + (1 if plus1 else 0)
    b = np.searchsorted(ptr, np.arange(n), "right") - 1
    occupied = np.flatnonzero(np.diff(ptr) > 0)
    b_lo, b_hi = int(occupied[0]), int(occupied[-1])
    if cells == "div":
        c = ((p - lo) / res).astype(np.int64)
    elif cells == "mul":
        c = ((p - lo) * (F(1) / res)).astype(np.int64)
    else:
        c = ((p.astype(np.float64) - lo.astype(np.float64)) / np.float64(res)).astype(np.int64)
    d0, d1, d2_ = (int(v) for v in dims)
    keys = np.array([(((int(bb) - b_lo) * d2_ + int(cz)) * d1 + int(cy)) * d0 + int(cx) for bb, (cx, cy, cz) in zip(b, c)], np.uint64)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    sorted_keys = keys[order]
    cell_keys, inv = np.unique(keys, return_inverse=True)
    idx = np.zeros(len(cell_keys), np.int32) if rep == "max" else np.full(len(cell_keys), n, np.int32)
    (np.maximum if rep == "max" else np.minimum).at(idx, inv, np.arange(n, dtype=np.int32))
    batch = b[idx].astype(np.int32)
    out_ptr = np.searchsorted(batch, np.arange(B + 1), "left").astype(np.int32)
    per = d0 * d1 * d2_
    T = (1 << 62) if max(d0, d1, d2_) > (1 << 20) else per * (b_hi - b_lo + 1)
    return Sampled(lo, hi, dims, b_lo, T, keys, order, sorted_keys, cell_keys.astype(np.uint64), idx, out_ptr, batch, inv.astype(np.int32),
                   inv[order].astype(np.int32), grid_image(lo, res, hi, b_lo, dims))


# ---- cases: searches -------------------------------------------------------------------------------------------------------------------

@dataclass
class Search:
    """Candidates in ascending cell-key order of `grid` (the order the sampler leaves a level in), each carrying its index in the
    caller's numbering in .w; queries of their own (.w = the row X_ROW_IN_W writes to) - every GPU test also searches from
    x[qidx] with qidx = self_queries()."""
    name: str
    group: str
    x: np.ndarray                 # [n, 4]
    ptr_x: np.ndarray
    q: np.ndarray                 # [m, 4]
    ptr_q: np.ndarray
    ks: tuple = ()                # kNN searches
    balls: tuple = ()             # (r, cap) ball queries
    keys: np.ndarray = None       # [n] uint64 (None: no grid - brute force only)
    grid: np.ndarray = None       # [56] uint8
    cell_start: np.ndarray = None
    hints: dict = field(default_factory=dict)   # name -> (k, hint [m] float32)
    note: dict = field(default_factory=dict)    # what the case is named for, as recorded facts (checked by the CPU file)
    rows: int = 0

    def self_queries(self, stride=3):
        """(qidx, ptr_q): every stride-th candidate of every voxel, last first - queries that are themselves candidates."""
        parts = [np.arange(int(a), int(b))[::-1][::stride] for a, b in zip(self.ptr_x[:-1], self.ptr_x[1:])]
        return (np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32),
                np.concatenate([[0], np.cumsum([len(v) for v in parts])]).astype(np.int32))


def _ptr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def assemble(name, group, pts, qs, res, ks=(), balls=(), sf=None, reverse_in_cell=False, perm_seed=None, note=None, hints=None, table=True):
    """pts / qs: per voxel [n_b, 3] / [m_b, 3] float32 in the caller's numbering.  The candidates are stored in the sampler's order (keys
    and grid of the coordinates as given); with sf they are then moved by the (p / sf) * sf round trip, as the engine's levels are."""
    pts = [np.asarray(v, F).reshape(-1, 3) for v in pts]
    qs = [np.asarray(v, F).reshape(-1, 3) for v in qs]
    P, ptr_x = np.concatenate(pts), _ptr([len(v) for v in pts])
    if perm_seed is not None:                                              # shuffle the caller's numbering inside every voxel
        rng = np.random.default_rng(perm_seed)
        P = np.concatenate([v[rng.permutation(len(v))] for v in pts])
    S = sample(records(P, np.zeros(len(P), np.int32)), ptr_x, res)
    order = S.order
    if reverse_in_cell:                                                    # inside a cell the order is free: highest carried index first
        order = np.lexsort((-np.arange(len(P)), S.keys)).astype(np.int32)
    stored = P[order]
    if sf is not None:
        b = np.searchsorted(ptr_x, np.arange(len(P)), "right") - 1
        stored = gather(records(stored, order), np.arange(len(P)), b, sf)[:, :3]
    Q, ptr_q = (np.concatenate(qs) if qs else np.zeros((0, 3), F)), _ptr([len(v) for v in qs])
    m = len(Q)
    rows = np.arange(m, dtype=np.int32)[::-1] + 5                          # rows written under Q_ROW_IN_W: reversed, shifted by 5
    cs = cell_starts(S.sorted_keys, S.T) if (table and S.T <= (1 << 22)) else None
    return Search(name, group, records(stored, order), ptr_x, records(Q, rows), ptr_q, tuple(ks), tuple(balls), S.sorted_keys, S.grid, cs,
                  dict(hints or {}), dict(note or {}), rows=m + 5)


def plain(name, group, x, ptr_x, q, ptr_q, ks=(), balls=(), note=None):
    """A case without a grid: storage order and carried indices exactly as given (brute force and tile boxes only)."""
    m = len(q)
    return Search(name, group, np.asarray(x, F), np.asarray(ptr_x, np.int32), records(np.asarray(q, F)[:, :3], np.arange(m)[::-1] + 5),
                  np.asarray(ptr_q, np.int32), tuple(ks), tuple(balls), note=dict(note or {}), rows=m + 5)


# -- planted pairs (seeded searches; every pair is re-verified in rational arithmetic by the CPU file) --

R_BALL, RES_BALL = 0.08, 0.04                                              # the engine's ball query: r = 2 * res at the 0.04 level


def _shell(rng, n, r, centre_span=1.0):
    """n (query, candidate) pairs with the candidate on the float32-rounded shell of radius r around the query."""
    q = rng.uniform(-centre_span, centre_span, (n, 3)).astype(F)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return q, (q.astype(np.float64) + r * u).astype(F)


def _inside(D, r2):
    return D < r2


@functools.lru_cache(maxsize=None)
def planted_pairs(r=R_BALL):
    """name -> (q [3], c [3]) for the predicate cases at radius r, found by one seeded search on the shell."""
    rng = np.random.default_rng(20260311)
    r2 = r2_of(r)
    want = {
        "d2_eq_r2": lambda D: D["sum"] == r2,
        "d2_below_r2": lambda D: D["sum"] == below(r2),
        "d2_above_r2": lambda D: D["sum"] == above(r2),
        "sum_in_fma_out": lambda D: _inside(D["sum"], r2) & ~_inside(D["fma_xy"], r2),
        "sum_out_fma_in": lambda D: ~_inside(D["sum"], r2) & _inside(D["fma_xy"], r2),
        "sum_in_fmaz_out": lambda D: _inside(D["sum"], r2) & ~_inside(D["fma_z"], r2),
        "sum_out_fmaz_in": lambda D: ~_inside(D["sum"], r2) & _inside(D["fma_z"], r2),
        "sum_in_reassoc_out": lambda D: _inside(D["sum"], r2) & ~_inside(D["reassoc"], r2),
        "sum_out_reassoc_in": lambda D: ~_inside(D["sum"], r2) & _inside(D["reassoc"], r2),
        "f32_in_f64_out": lambda D: _inside(D["sum"], r2) & ~(D["f64"] < float(r) * float(r)),
        "f32_out_f64_in": lambda D: ~_inside(D["sum"], r2) & (D["f64"] < float(r) * float(r)),
    }
    found = {}
    for _ in range(40):
        q, c = _shell(rng, 200000, r)
        D = {f: d2_rows(q, c, f) for f in ("sum", "fma_xy", "fma_z", "reassoc")}
        dd = q.astype(np.float64) - c.astype(np.float64)
        D["f64"] = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        for name, test in want.items():
            if name in found:
                continue
            for i in np.flatnonzero(test(D))[:8]:                          # the float64 emulation of the FMA forms rounds twice: confirm
                if _confirm(name, q[i], c[i], r):
                    found[name] = (q[i].copy(), c[i].copy())
                    break
        if len(found) == len(want):
            break
    return found


def _confirm(name, q, c, r):
    """The named condition of a planted pair in rational arithmetic."""
    r2, R2 = Fraction(float(r2_of(r))), Fraction(float(r)) * Fraction(float(r))
    e = {f: exact_d2(q, c, f) for f in FORMS}
    inn = {f: e[f] < r2 for f in FORMS if f != "f64"}
    if name == "d2_eq_r2":
        return e["sum"] == r2
    if name == "d2_below_r2":
        return e["sum"] == Fraction(float(below(r2_of(r))))
    if name == "d2_above_r2":
        return e["sum"] == Fraction(float(above(r2_of(r))))
    if name == "f32_in_f64_out":
        return inn["sum"] and not e["f64"] < R2
    if name == "f32_out_f64_in":
        return not inn["sum"] and e["f64"] < R2
    head, other, tail = name.split("_")[1], {"fma": "fma_xy", "fmaz": "fma_z", "reassoc": "reassoc"}[name.split("_")[2]], name.split("_")[3]
    return inn["sum"] == (head == "in") and inn[other] == (tail == "in") and head != tail


RADII = (0.05, 0.06, 0.07, 0.08, 0.1, 0.12, 0.16, 0.2, 0.3, 0.32, 0.64)   # the short list searched for float32(r)^2 != float32(r*r)


@functools.lru_cache(maxsize=None)
def planted_radius():
    """(r, q, c) with float32(r)*float32(r) != float32(r*r) and d2(q, c) between the two (in one, not in the other), or None."""
    rng = np.random.default_rng(20260312)
    for r in RADII:
        a, b = r2_of(r), r2_f32(r)
        if a == b:
            continue
        for _ in range(20):
            q, c = _shell(rng, 200000, r)
            D = d2_rows(q, c)
            hit = np.flatnonzero((D < a) != (D < b))
            if len(hit):
                return r, q[hit[0]].copy(), c[hit[0]].copy()
    return None


def _ball_cloud(name, q0, c0, r, seed, note):
    """One voxel: the planted pair, 150 candidates in the 0.4 m cube around the query and 24 more queries."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([[c0], (q0 + rng.uniform(-0.2, 0.2, (150, 3))).astype(F)])
    qs = np.concatenate([[q0], (q0 + rng.uniform(-0.2, 0.2, (24, 3))).astype(F)])
    return assemble(name, "predicate", [pts], [qs], r / 2, ks=(4,), balls=((r, 32), (r, 3)), perm_seed=seed + 1, note=dict(note, q=q0, c=c0, r=r))


def _predicate_cases():
    out = {}
    for pair_name in sorted(planted_pairs()):
        out["ball_" + pair_name] = (lambda n=pair_name: _ball_cloud("ball_" + n, *planted_pairs()[n], R_BALL, zlib.crc32(n.encode()) % 1000, {"pair": n}))
    if planted_radius() is not None:
        out["ball_radius_f32_squared"] = lambda: _ball_cloud("ball_radius_f32_squared", planted_radius()[1], planted_radius()[2], planted_radius()[0],
                                                             150, {"pair": "radius"})
    return out


@functools.lru_cache(maxsize=None)
def planted_swap():
    """(q, a, b): d2(q, a) < d2(q, b) in the contract's form and the reverse under fma(dz, dz, fma(dy, dy, dx*dx)), both exact."""
    rng = np.random.default_rng(20260313)
    for _ in range(40):
        q = rng.uniform(-1, 1, 3).astype(F)
        u = rng.normal(size=(100000, 3))
        c = (q.astype(np.float64) + 0.3 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
        s, f = d2_rows(np.broadcast_to(q, c.shape), c), d2_rows(np.broadcast_to(q, c.shape), c, "fma_xy")
        o = np.argsort(s, kind="stable")
        for i, j in zip(o[:-1], o[1:]):
            if s[i] < s[j] and f[i] > f[j] and exact_d2(q, c[i]) < exact_d2(q, c[j]) and exact_d2(q, c[i], "fma_xy") > exact_d2(q, c[j], "fma_xy"):
                return q, c[i].copy(), c[j].copy()
    raise AssertionError("no swap pair found")


def _swap_cloud(name, near, k):
    """The planted query with `near` candidates strictly nearer than the pair (a, b), then a, b, then farther ones."""
    q, a, b = planted_swap()
    rng = np.random.default_rng(7 + near)
    u = rng.normal(size=(near + 40, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = np.concatenate([rng.uniform(0.05, 0.2, near), rng.uniform(0.4, 0.6, 40)])
    pts = np.concatenate([[b, a], (q + u * rad[:, None]).astype(F)])
    qs = np.concatenate([[q], (q + rng.uniform(-0.3, 0.3, (9, 3))).astype(F)])
    return assemble(name, "knn_order", [pts], [qs], 0.25, ks=(k,), perm_seed=None, note={"q": q, "a": a, "b": b, "near": near, "k": k})


def _tie_later():
    """k = 4: the 4th and 5th neighbours of the query are mirror images (equal d2 by construction); the one with the LOWER carried
    index lies ~1300 records later in storage (another 1024-tile, another z layer's run)."""
    rng = np.random.default_rng(31)
    q = np.array([0.5, 0.5, 1.0], F)
    off = np.array([0.0625, 0.03125, 0.125], F)
    hi_z, lo_z = q + off, q - off * np.array([-1, 1, 1], F)               # (x + dx, y - dy, z - dz): same |d| per axis
    near = (q + np.array([[0.015625, 0, 0], [0, 0.015625, 0], [0, 0, 0.015625]], F)).astype(F)
    slab = np.column_stack([np.where(rng.uniform(size=2800) < 0.5, rng.uniform(0, 0.3, 2800), rng.uniform(0.7, 1.0, 2800)),
                            rng.uniform(0, 1, 2800), rng.uniform(0.76, 1.24, 2800)])   # the two layers of the pair, |dx| >= 0.2: farther than it
    fill = np.concatenate([slab, rng.uniform(0, 1, (200, 3)) * np.array([1, 1, 0.7])]).astype(F)
    pts = np.concatenate([[hi_z], near, fill, [lo_z]])                     # carried index 0 = the later one in storage (higher z)
    qs = np.concatenate([[q], rng.uniform(0.2, 0.8, (7, 3)).astype(F) + np.array([0, 0, 0.5], F)])
    return assemble("knn_tie_lower_index_later", "knn_order", [pts], [qs], 0.25, ks=(4, 5), note={"q": q, "first": 0, "second": len(pts) - 1})


def _fourfold():
    rng = np.random.default_rng(32)
    base = rng.uniform(0, 1, (90, 3)).astype(F)
    pts = np.concatenate([base, base, base, base])
    qs = np.concatenate([base[:20], rng.uniform(0, 1, (13, 3)).astype(F)])
    return assemble("knn_fourfold_duplicates_reversed", "knn_order", [pts], [qs], 0.25, ks=(1, 2, 3, 6, 8), balls=((0.2, 5), (0.2, 64)),
                    reverse_in_cell=True)


# -- tile boxes (brute force with boxes; storage order given) --

def _box_face_tie():
    """k = 1.  Tile 0 holds a candidate at d2 = 1/16 with carried index 5000 and the query inside its box; tile 1's box face is exactly
    1/4 away and a candidate with carried index 3 sits on it: box_gap2 == thr, and the lower index must still win."""
    rng = np.random.default_rng(41)
    t0 = np.concatenate([[[-0.25, 0, 0]], np.column_stack([rng.uniform(-2, 0.125, 1023), rng.uniform(1, 2, 1023), rng.uniform(-1, 1, 1023)])])
    t1 = np.concatenate([[[0.25, 0, 0]], np.column_stack([rng.uniform(1, 2, 299), rng.uniform(-1, 1, 299), rng.uniform(-1, 1, 299)])])
    w = np.concatenate([[5000], 10 + np.arange(1023), [3], 2000 + np.arange(299)])
    x = records(np.concatenate([t0, t1]).astype(F), w)
    q = np.array([[0, 0, 0, 0], [0.01, 0.02, 0, 0], [1.5, 0, 0, 0]], F)
    return plain("box_face_tie_needs_le", "tile_boxes", x, [0, len(x)], q, [0, len(q)], ks=(1, 2), note={"q": q[0, :3], "on_face": 1024, "held": 0})


@functools.lru_cache(maxsize=None)
def radius_above_quarter():
    """A double r with float32(r*r) == the float above 1/16."""
    target = above(F(0.0625))
    r = float(np.sqrt(np.float64(target)))
    for _ in range(8):
        if r2_of(r) == target:
            return r
        r = float(np.nextafter(r, np.inf if r2_of(r) < target else -np.inf))
    raise AssertionError


def _ball_box(name, r):
    """The ball-query twin: tile 1's box face exactly 1/4 from the query with a candidate on it; r*r is 1/16 (not in the ball, tile not
    needed) or the float above (in the ball: box_gap2 is the float just below r2 and the tile must be staged)."""
    c = _box_face_tie()
    return plain(name, "tile_boxes", c.x, c.ptr_x, c.q, c.ptr_q, balls=((r, 4), (r, 64)), note={"q": c.q[0, :3], "on_face": 1024, "r": r})


# -- sizes --

Q_COUNTS = (0, 0, 1, 31, 0, 32, 33, 0, 0, 0, 63, 64, 65, 0)               # queries per voxel, repeated over B = 300 voxels


def _sizes_queries():
    rng = np.random.default_rng(51)
    B = 300
    mq = [Q_COUNTS[b % len(Q_COUNTS)] for b in range(B)]
    mq[-1] = 0
    nx = [int(v) for v in rng.integers(1, 20, B)]
    for b in (0, 1, 5, 17, 18, 19, B - 1):
        nx[b] = 0                                                          # empty candidate voxels: first, last, in runs, one with queries
    pts = [rng.uniform(0, 1, (n, 3)).astype(F) for n in nx]
    qs = [rng.uniform(0, 1, (m, 3)).astype(F) for m in mq]
    return assemble("sizes_queries_per_voxel_B300", "sizes", pts, qs, 0.25, ks=(3,), balls=((0.3, 4),), note={"mq": mq, "nx": nx})


C_COUNTS = {"small": (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025), "mid": (1791, 1792, 1793), "big": (3585,)}


def _sizes_cands(which, one_cell):
    rng = np.random.default_rng(52 + len(which))
    counts = C_COUNTS[which]
    if one_cell:                                                           # every voxel's candidates in one cell of a 4^3 grid
        pts = [(np.array([0.3, 0.55, 0.8]) + rng.uniform(0, 0.2, (n, 3))).astype(F) for n in counts]
        corner = [np.array([[0, 0, 0], [1, 1, 1]], F)]                     # a last voxel that spans the grid
        pts, extra = pts + corner, [np.zeros((0, 3), F)]
    else:
        pts, extra = [rng.uniform(0, 1, (n, 3)).astype(F) for n in counts], []
    qs = [rng.uniform(0.1, 0.9, (9, 3)).astype(F) for _ in counts] + extra
    return assemble(f"sizes_cands_{which}_{'one_cell' if one_cell else 'spread'}", "sizes", pts, qs, 0.25, ks=(2, 8, 33), balls=((0.25, 16),),
                    note={"counts": counts, "one_cell": one_cell})


K_SWEEP = (1, 2, 7, 8, 63, 64, 65, 100)


def _k_sweep():
    rng = np.random.default_rng(53)
    pts = [rng.uniform(0, 1, (n, 3)).astype(F) for n in (5, 300, 70)]
    qs = [rng.uniform(0, 1, (m, 3)).astype(F) for m in (33, 40, 3)]
    return assemble("sizes_k_and_cap_sweep", "sizes", pts, qs, 0.25, ks=K_SWEEP, balls=tuple((0.45, c) for c in K_SWEEP), note={"n": (5, 300, 70)})


# -- grid geometry --

def _on_faces(offset=0.0, name="grid_candidates_on_cell_faces"):
    """Candidates at lo + c * res with res = 1/4 and lo = offset: multiples of 1/4 are exact in float32 at every offset used."""
    rng = np.random.default_rng(61)
    lat = np.stack(np.meshgrid(*[np.arange(5) * 0.25] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([lat, rng.uniform(0, 1, (200, 3))]) + offset
    qs = np.concatenate([lat[::7] + 0.125, rng.uniform(0, 1, (30, 3))]) + offset
    return assemble(name, "grid", [pts.astype(F)], [qs.astype(F)], 0.25, ks=(1, 2, 8, 32), balls=((0.25, 8), (0.5, 64)), perm_seed=62,
                    note={"offset": offset, "lattice": len(lat)})


SF_LIST = (0.7, 0.9, 1.1, 1.3, 1.7, 2.3, 2.9, 3.1, 0.37, 5.3, 0.013)


@functools.lru_cache(maxsize=None)
def planted_roundtrip():
    """(sf, res, c): the exactly representable face coordinate y = c * res (lo = 0) that float32 (y / sf) * sf moves BELOW the face."""
    res = F(0.25)
    for sf in SF_LIST:
        for c in (2, 3, 1):
            y = F(c) * res
            if (y / F(sf)) * F(sf) < y:
                return float(sf), float(res), c
    raise AssertionError("no scale factor moves a face coordinate down")


def _roundtrip_face():
    """The engine's situation: keys of the coordinates before the round trip, coordinates after it.  P is keyed into the cell row above
    the face (y = face before the trip) and lies one ulp below it afterwards; the lone query sits 0.65 res below the face in a row dense
    enough that the first region ends at the face; D, in the query's own row, is farther than P but nearer than the face.  The true
    nearest neighbour is P, which only the grown region (or the face margin) finds."""
    sf, res, c = planted_roundtrip()
    face = F(c) * F(res)
    rt = lambda v: (F(v) / F(sf)) * F(sf)                                  # noqa: E731
    qy = F(face - F(0.65) * F(res))
    q = np.array([0.125, qy, 0.375], F)
    P_pre = np.array([0.125, face, 0.375], F)
    dP = d2_rows(q[None], np.array([[rt(P_pre[0]), rt(P_pre[1]), rt(P_pre[2])]], F))[0]
    gap2 = (face - qy) * (face - qy)
    D_pre = None
    x = F(0.125) + F(0.65) * F(res)
    for _ in range(64):                                                    # D = (x, qy, qz): walk x down from the face distance
        cand = np.array([rt(x), rt(qy), rt(q[2])], F)
        d = d2_rows(q[None], cand[None])[0]
        if dP < d <= gap2:
            D_pre = np.array([x, qy, q[2]], F)
            break
        x = below(x)
    assert D_pre is not None
    rng = np.random.default_rng(63)
    row = np.column_stack([rng.uniform(0.6, 1.0, 1500), np.full(1500, qy), np.full(1500, 0.375)])   # density of the query's own row
    frame = np.array([[0, 0, 0], [1, 1, 1]], F)
    rest = rng.uniform(0, 1, (60, 3)) * np.array([1, 1, 0.2]) + np.array([0, 0, 0.7])             # other layers, far away
    pts = np.concatenate([[P_pre], [D_pre], row, frame, rest]).astype(F)
    return assemble("grid_roundtrip_moves_kth_across_face", "grid", [pts], [q[None]], res, ks=(1,), sf=[sf],
                    note={"sf": sf, "face": float(face), "q": q, "P": 0, "D": 1})


def slab_schedule(c, k):
    """The pass schedule of the grid kNN search (no hints, no P2W_SEARCH_BOX) for the first workgroup of a one-voxel case - its first 32
    queries - restated from the comments of csrc/p2w_geom.hip: face margin eps = res/32 + 1e-5 max|coordinate|; a density probe over the
    rows that hold the queries gives rk and the first radius rho = 1.1 rk + res/2; a pass scans the rows and layers within rho + eps of
    the queries' box that it has not scanned (a candidate's row and layer are those of its KEY); more than 128 layers, or pass 8, make
    the whole voxel one run and - if anything was scanned - every unfinished query forgets its list; a query is final when its k-th d2 is
    at most the squared gap (less eps) to the nearest face of the scanned box that is not a grid face; else the radius becomes
    sqrt(thr) 1.0001 + 3 eps, or 2 rho + res while fewer than k were found.  Returns one dict per pass: rho, box (y0, y1, z0, z1), whole,
    forgot, found (fewest candidates any active query had seen after the pass), left (queries not final)."""
    lo, res, hi, dims = c.grid[:12].view(F), c.grid[12:16].view(F)[0], c.grid[16:28].view(F), [int(v) for v in c.grid[32:56].view(np.int64)]
    c0, c1 = int(c.ptr_x[0]), int(c.ptr_x[1])
    q = c.q[:min(32, int(c.ptr_q[1])), :3]
    key = c.keys[c0:c1].astype(np.int64)
    cy, cz = (key // dims[0]) % dims[1], (key // (dims[0] * dims[1])) % dims[2]
    D = d2(q, c.x[c0:c1])
    eps = res * F(1 / 32) + F(1e-5) * max(F(1), np.abs(lo).max(), np.abs(hi).max())
    ymin, ymax, zmin, zmax = q[:, 1].min(), q[:, 1].max(), q[:, 2].min(), q[:, 2].max()

    def cell(v, a):
        return int(min(max(np.floor((F(v) - lo[a]) / res), F(0)), F(dims[a] - 1)))

    def region(rho, old):
        box = [cell(ymin - rho - eps, 1), cell(ymax + rho + eps, 1), cell(zmin - rho - eps, 2), cell(zmax + rho + eps, 2)]
        if old is not None:
            box = [min(box[0], old[0]), max(box[1], old[1]), min(box[2], old[2]), max(box[3], old[3])]
        return box

    def inside(box):
        return (cy >= box[0]) & (cy <= box[1]) & (cz >= box[2]) & (cz <= box[3])

    box = region(F(0), None)
    n0 = int(inside(box).sum())
    if box[3] - box[2] + 1 <= 128 and n0 >= 8:
        dens = F(n0) / (((F(dims[0]) * res) * (F(box[1] - box[0] + 1) * res)) * (F(box[3] - box[2] + 1) * res))
    else:
        dens = F(c1 - c0) / max(((F(dims[0]) * res) * (F(dims[1]) * res)) * (F(dims[2]) * res), F(1e-30))
    rk = np.cbrt(F(0.75) * F(k) / (F(3.14159265) * max(dens, F(1e-30))))
    rho = min(F(1.1) * rk, F(1e30)) + F(0.5) * res
    old, whole, active, passes = None, False, np.ones(len(q), bool), []
    seen = np.zeros(c1 - c0, bool)
    for p in range(12):
        was_whole, forgot = whole, False
        if not was_whole:
            box = region(rho, old)
            whole = p >= 8 or box[3] - box[2] + 1 > 128
            forgot = whole and old is not None
        seen = np.ones_like(seen) if whole else seen | inside(box)
        if not was_whole:
            old = box
        kk = min(k, c1 - c0)
        thr = np.sort(np.where(seen[None, :], D, INF), axis=1)[:, kk - 1]
        need = F(0)
        if whole:
            active[:] = False
        else:
            f = [-INF if box[0] <= 0 else lo[1] + F(box[0]) * res, INF if box[1] >= dims[1] - 1 else lo[1] + F(box[1] + 1) * res,
                 -INF if box[2] <= 0 else lo[2] + F(box[2]) * res, INF if box[3] >= dims[2] - 1 else lo[2] + F(box[3] + 1) * res]
            for j in np.flatnonzero(active):
                gap = min(min(q[j, 1] - f[0], f[1] - q[j, 1]), min(q[j, 2] - f[2], f[3] - q[j, 2])) - eps
                if gap > 0 and thr[j] <= gap * gap:
                    active[j] = False
                else:
                    need = max(need, np.sqrt(thr[j]) * F(1.0001) + F(3) * eps if thr[j] < INF else F(2) * rho + res)
        passes.append(dict(rho=float(rho), box=tuple(box), whole=whole, forgot=forgot, found=int(seen.sum()), left=int(active.sum())))
        if not need > 0:
            break
        rho = max(need, rho)
    return passes


def _growth(which):
    """One workgroup of six queries around q, near candidates in q's own cell row, the decisive ones far away in y (y rows do not count
    against the 128-layer limit).  What the schedule does with each (asserted by the CPU file from slab_schedule):
      once      k = 4, three near, the fourth five rows up: the first region (rows 0 .. 2) holds three, the doubled radius finds it;
      clamp     k = 4, the fourth in the LAST of 14 rows: the region grows until it is clamped at the grid face (no face left to test);
      give_up   k = 12, ten near (the probe's density comes from them, so the first radius is under two cells), the others 560 rows
                away: seven doublings do not reach them, pass 8 takes the whole voxel and every query forgets its ten."""
    rng = np.random.default_rng({"once": 64, "clamp": 65, "give_up": 66}[which])
    res, k, n_near = 0.25, (12 if which == "give_up" else 4), (10 if which == "give_up" else 3)
    ny = 600 if which == "give_up" else 14
    q = np.array([0.6, 0.1, 0.6], F)
    near = q + rng.uniform(-0.05, 0.05, (n_near, 3))
    top = ny * res - 0.01
    if which == "once":
        far = np.array([[0.6, 0.1 + 5 * res, 0.6]])
    elif which == "clamp":
        far = np.array([[0.6, top - 0.05, 0.6]])
    else:
        far = np.column_stack([rng.uniform(0, 1, 6), rng.uniform(top - 10 * res, top - 0.05, 6), rng.uniform(0, 1, 6)])
    frame = np.array([[1, top, 1], [0.02, 0.06, 0.02]]) if which == "give_up" else np.array([[1, top, 1]])
    extra = np.zeros((0, 3)) if which != "once" else np.column_stack([rng.uniform(0, 1.0, 40), np.full(40, top), rng.uniform(0, 1, 40)])
    pts = np.concatenate([near, far, extra, frame]).astype(F)
    qs = np.concatenate([[q], q + rng.uniform(-0.04, 0.04, (5, 3))]).astype(F)
    name = {"once": "grid_growth_one_more_pass", "clamp": "grid_growth_into_the_face_clamp", "give_up": "grid_give_up_after_8_passes"}[which]
    return assemble(name, "grid", [pts], [qs], res, ks=(k,), note={"k": k, "near": n_near})


def _fallback():
    """A column of 400 z layers with the workgroup's six queries in the middle: ten near candidates (k = 12), the others 190 layers
    away at both ends.  The first passes scan a few layers and find ten; the doubling radius then spans more than 128 layers, the
    whole voxel becomes one run and every query forgets its partial list before it is shown the ten again."""
    rng = np.random.default_rng(77)
    res, nz = 0.25, 400
    q = np.array([0.6, 0.6, 200 * res + 0.1], F)
    near = q + rng.uniform(-0.05, 0.05, (10, 3))
    ends = np.concatenate([np.column_stack([rng.uniform(0, 1, 5), rng.uniform(0, 1, 5), rng.uniform(0, 8 * res, 5)]),
                           np.column_stack([rng.uniform(0, 1, 5), rng.uniform(0, 1, 5), rng.uniform((nz - 8) * res, nz * res - 0.02, 5)])])
    frame = np.array([[0, 0, 0], [1, 1, nz * res - 0.01]])
    pts = np.concatenate([near, ends, frame]).astype(F)
    qs = np.concatenate([[q], q + rng.uniform(-0.04, 0.04, (5, 3))]).astype(F)
    return assemble("grid_fallback_over_128_layers_forgets", "grid", [pts], [qs], res, ks=(12,), note={"k": 12, "near": 10})


def _thin(axis):
    rng = np.random.default_rng(70 + axis)
    pts = rng.uniform(0, 1, (400, 3))
    pts[:, axis] *= 0.2                                                    # one cell thick at res 0.25
    qs = rng.uniform(0, 1, (40, 3))
    qs[:, axis] *= 0.2
    return assemble(f"grid_one_cell_thick_{'xyz'[axis]}", "grid", [pts.astype(F)], [qs.astype(F)], 0.25, ks=(1, 8), balls=((0.3, 16),),
                    note={"axis": axis})


def _tall():
    """A column of 300 z layers with the 32 queries of the one workgroup spread over all of it: the density probe's own region already
    spans more than 128 layers, so the whole voxel is one run from the first pass on (nothing was scanned, nothing is forgotten)."""
    rng = np.random.default_rng(75)
    res = 0.25
    z = np.sort(rng.uniform(0, 300 * res, 200))
    pts = np.column_stack([rng.uniform(0, 0.5, 200), rng.uniform(0, 0.5, 200), z])
    qz = np.linspace(1, 299 * res, 32)
    qs = np.column_stack([np.full(32, 0.25), np.full(32, 0.25), qz])
    return assemble("grid_probe_region_over_128_layers", "grid", [pts.astype(F)], [qs.astype(F)], res, ks=(2, 40), balls=((0.6, 8),),
                    note={"layers": 300})


def _box_rows():
    """20 x 20 occupied (z, y) rows, queries of one workgroup spread over all of them: with P2W_SEARCH_BOX the region has 400 rows = 800
    runs, more than the 256 a pass's run table holds."""
    rng = np.random.default_rng(76)
    res = 0.25
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([np.column_stack([rng.uniform(0, 1.5, len(g)), (g[:, 1] + rng.uniform(0.1, 0.9, len(g))) * res,
                                           (g[:, 0] + rng.uniform(0.1, 0.9, len(g))) * res]) for _ in range(3)])
    qs = np.column_stack([rng.uniform(0, 1.5, 32), rng.uniform(0, 5, 32), rng.uniform(0, 5, 32)])
    return assemble("grid_box_more_than_256_runs", "grid", [pts.astype(F)], [qs.astype(F)], res, ks=(3, 8), balls=((0.5, 16),), note={"rows": 400})


# -- hints --

def _hints():
    rng = np.random.default_rng(81)
    res = F(0.25)
    pts = [rng.uniform(0, 1, (300, 3)).astype(F), np.array([[0.3, 0.3, 0.3]], F)]
    pts[0][:3] = pts[0][3]                                                 # four coincident candidates
    qs = [np.concatenate([pts[0][3:4], rng.uniform(0, 1, (31, 3)).astype(F)]), rng.uniform(0, 1, (4, 3)).astype(F)]
    c = assemble("hints_planted", "hints", pts, qs, res, ks=(1, 2))
    k1, k2 = kth_d2(c.x, c.ptr_x, c.q, c.ptr_q, 1), kth_d2(c.x, c.ptr_x, c.q, c.ptr_q, 2)
    nine = (F(9) * res) * res
    assert k2[0] == 0 and k2.max() < nine

    def put(h, i, v):
        h = h.copy()
        h[i] = v
        return h
    c.hints = {
        "exact_k1": (1, k1), "exact_k2": (2, k2),                                                      # query 0 lies on four coincident points: hint 0
        "below_k1": (1, put(k1, 7, below(k1[7]))), "below_k2": (2, put(k2, 7, below(k2[7]))),          # bogus for query 7: a rescan
        "one_inf_k2": (2, put(k2, 20, INF)),
        "hmax_9res2_k2": (2, put(k2, 9, nine)), "hmax_above_9res2_k2": (2, put(k2, 9, above(nine))),
        "all_inf_k2": (2, np.full(len(k2), INF, F)),
    }
    c.note = {"k1": k1, "k2": k2, "nine": nine, "one_candidate_voxel": 1}
    return c


SEARCH = {
    **_predicate_cases(),
    "knn_fma_swap_at_k": lambda: _swap_cloud("knn_fma_swap_at_k", 7, 8),
    "knn_fma_swap_inside": lambda: _swap_cloud("knn_fma_swap_inside", 3, 8),
    "knn_tie_lower_index_later": _tie_later,
    "knn_fourfold_duplicates_reversed": _fourfold,
    "box_face_tie_needs_le": _box_face_tie,
    "ball_box_gap_eq_r2": lambda: _ball_box("ball_box_gap_eq_r2", 0.25),
    "ball_box_gap_below_r2": lambda: _ball_box("ball_box_gap_below_r2", radius_above_quarter()),
    "sizes_queries_per_voxel_B300": _sizes_queries,
    **{f"sizes_cands_{w}_{'one_cell' if o else 'spread'}": (lambda w=w, o=o: _sizes_cands(w, o)) for w in C_COUNTS for o in (False, True)},
    "sizes_k_and_cap_sweep": _k_sweep,
    "grid_candidates_on_cell_faces": _on_faces,
    "grid_offset_plus_100": lambda: _on_faces(100.0, "grid_offset_plus_100"),
    "grid_offset_minus_3": lambda: _on_faces(-3.0, "grid_offset_minus_3"),
    "grid_roundtrip_moves_kth_across_face": _roundtrip_face,
    "grid_growth_one_more_pass": lambda: _growth("once"),
    "grid_growth_into_the_face_clamp": lambda: _growth("clamp"),
    "grid_give_up_after_8_passes": lambda: _growth("give_up"),
    "grid_fallback_over_128_layers_forgets": _fallback,
    **{f"grid_one_cell_thick_{'xyz'[a]}": (lambda a=a: _thin(a)) for a in range(3)},
    "grid_probe_region_over_128_layers": _tall,
    "grid_box_more_than_256_runs": _box_rows,
    "hints_planted": _hints,
}


@functools.lru_cache(maxsize=None)
def search_case(name):
    return SEARCH[name]()


# ---- cases: the sampler ----------------------------------------------------------------------------------------------------------------

@dataclass
class Sampling:
    name: str
    xyzr: np.ndarray              # [n, 4]
    ptr: np.ndarray               # [B + 1]
    res: float
    table_cells: tuple = ()       # capacities to call the table sampler with; () = the grid's own size
    note: dict = field(default_factory=dict)


def _sampling(name, pts, res, table_cells=(), note=None, seed=0):
    pts = [np.asarray(v, F).reshape(-1, 3) for v in pts]
    P = np.concatenate(pts)
    refl = np.random.default_rng(seed).uniform(0, 1, len(P)).astype(F)
    x = np.column_stack([P, refl]).astype(F)
    return Sampling(name, x, _ptr([len(v) for v in pts]), float(res), tuple(table_cells), dict(note or {}))


@functools.lru_cache(maxsize=None)
def planted_cells(res=0.04):
    """(on_face [..], split [..]): float32 coordinates (lo = 0) p = fl(c * res) whose float32 quotient p / res is exactly c while the true
    quotient is below c; and coordinates whose cell differs between division by res and multiplication by float32(1 / res)."""
    r = F(res)
    c = np.arange(1, 100, dtype=np.int64)
    p = c.astype(F) * r
    exact = (p / r == c.astype(F)) & (p.astype(np.float64) / np.float64(r) < c)
    rng = np.random.default_rng(20260314)
    v = rng.uniform(0, 4, 2000000).astype(F)
    split = v[(v / r).astype(np.int64) != (v * (F(1) / r)).astype(np.int64)]
    return p[exact][:12], split[:12]


def _planted_sampling(which):
    on_face, split = planted_cells()
    rng = np.random.default_rng(91)
    chosen = on_face if which == "face" else split
    pts = np.concatenate([[[0, 0, 0]], np.column_stack([chosen, chosen[::-1], np.roll(chosen, 3)]), rng.uniform(0, 4, (300, 3))])
    return _sampling(f"sampler_{'points_on_faces_quotient_exact' if which == 'face' else 'div_and_mul_cells_differ'}", [pts[:150], pts[150:]], 0.04,
                     note={"planted": chosen})


def _extent_multiple():
    rng = np.random.default_rng(92)
    pts = np.concatenate([[[0, 0, 0], [1, 1, 1]], rng.uniform(0, 0.999, (500, 3))])
    return _sampling("sampler_extent_exact_multiple", [pts[:200], [], pts[200:]], 0.25, note={"dims": 5})


def _one_cell(n=5000):
    rng = np.random.default_rng(93)
    return _sampling("sampler_all_in_one_cell_n5000", [rng.uniform(0, 0.01, (n, 3))], 0.04, note={"n": n})


def _own_cells():
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.1 + 0.02
    g = g[np.random.default_rng(94).permutation(len(g))]
    return _sampling("sampler_every_point_own_cell", [g[:100], g[100:]], 0.05, note={"n": len(g)})


def _size_n(n):
    rng = np.random.default_rng(95 + n)
    counts = [n] if n < 3 else [n // 3, 0, n - n // 3]
    pts = [rng.uniform(0, 1, (m, 3)) for m in counts]
    return _sampling(f"sampler_n_{n}", pts, 0.04, note={"n": n})


def _empty_voxels():
    rng = np.random.default_rng(96)
    counts = [0, 0, 40, 0, 0, 0, 1, 300, 0, 25, 0, 0]
    return _sampling("sampler_empty_voxels_first_last_inside", [rng.uniform(0, 1, (m, 3)) for m in counts], 0.1, note={"counts": counts})


def _huge_grid():
    rng = np.random.default_rng(97)
    a, b = rng.uniform(0, 0.5, (300, 3)), rng.uniform(60, 60.5, (300, 3))
    return _sampling("sampler_grid_over_2_32_cells", [np.concatenate([a[:100], b[:100]]), np.concatenate([b[100:], a[100:]])], 0.01,
                     table_cells=(1 << 16,), note={"cells_at_least": 1 << 32})


def _capacity():
    rng = np.random.default_rng(98)
    pts = [np.concatenate([[[0, 0, 0], [1, 1, 1]], rng.uniform(0, 1, (200, 3))]), rng.uniform(0, 1, (150, 3))]
    return _sampling("sampler_table_cells_at_and_below_the_grid", pts, 0.1, table_cells=(2 * 11 ** 3, 2 * 11 ** 3 - 1, 2 * 11 ** 3 + 4097),
                     note={"T": 2 * 11 ** 3})


SAMPLER = {
    "sampler_points_on_faces_quotient_exact": lambda: _planted_sampling("face"),
    "sampler_div_and_mul_cells_differ": lambda: _planted_sampling("split"),
    "sampler_extent_exact_multiple": _extent_multiple,
    "sampler_all_in_one_cell_n5000": _one_cell,
    "sampler_every_point_own_cell": _own_cells,
    **{f"sampler_n_{n}": (lambda n=n: _size_n(n)) for n in (1, 4095, 4096, 4097, 8192)},
    "sampler_empty_voxels_first_last_inside": _empty_voxels,
    "sampler_grid_over_2_32_cells": _huge_grid,
    "sampler_table_cells_at_and_below_the_grid": _capacity,
}


@functools.lru_cache(maxsize=None)
def sampler_case(name):
    return SAMPLER[name]()


@functools.lru_cache(maxsize=None)
def sampled(name):
    c = sampler_case(name)
    return sample(c.xyzr, c.ptr, c.res)


# ---- the engine's chain ---------------------------------------------------------------------------------------------------------------

CHAIN_RES = (0.04, 0.08, 0.16)
CHAIN_K = 8


@functools.lru_cache(maxsize=None)
def chain_input():
    """Two voxels of about 600 and 200 points and their scale factors.  The origin is a point (so lo = 0) and 90 coordinates are float32
    multiples of the first cell size: they sit on or one ulp beside a cell face, and the scale factors are the first pair of SF_LIST
    whose round trip moves at least three sampled points into another cell than the one their key names."""
    rng = np.random.default_rng(20260315)
    a = rng.uniform(0, 0.6, (600, 3)) * np.array([1, 1, 2.0])
    b = rng.uniform(0, 0.5, (200, 3)) + 0.05
    a[0] = 0
    for i in range(1, 61):
        a[i, i % 3] = float(F(rng.integers(1, 15)) * F(CHAIN_RES[0]))
    for i in range(30):
        b[i, i % 3] = float(F(rng.integers(2, 12)) * F(CHAIN_RES[0]))
    x = np.column_stack([np.concatenate([a, b]), rng.uniform(0, 1, 800)]).astype(F)
    ptr = np.array([0, 600, 800], np.int32)
    S = sample(x, ptr, CHAIN_RES[0])
    pre = x[S.idx]
    for s0 in SF_LIST:
        for s1 in SF_LIST:
            sf = np.array([s0, s1], F)
            post = gather(x, S.idx, S.batch, sf)
            crossed = (cells_of(pre, S.lo, CHAIN_RES[0]) != cells_of(post, S.lo, CHAIN_RES[0])).any(1)
            if crossed[S.batch == 0].sum() >= 3 and crossed[S.batch == 1].sum() >= 3:
                return x, ptr, sf
    raise AssertionError("no scale factors move a point across a face")


def cells_of(xyz, grid_lo, res):
    """Per-axis cell of float32 coordinates in a grid (float32 subtract, divide, truncate), as the sampler computes them."""
    return ((np.asarray(xyz, F)[:, :3] - np.asarray(grid_lo, F)) / F(res)).astype(np.int64)


def chain(x, ptr, sf, order0=None):
    """The forward engine's geometry chain on the records x: per level the sampler (table form: cell-start tables), the round-trip
    gather, then the three SA searches and the three hinted k = 2 interpolation searches, arguments and flags as engine.py passes them.
    order0: the cell-sorted order of level 0 to use (the table sampler's order inside a cell is free); default the stable one."""
    T = {"xyzr": [np.asarray(x, F)], "ptr": [np.asarray(ptr, np.int32)], "S": []}
    for l, res in enumerate(CHAIN_RES):
        S = sample(T["xyzr"][l], T["ptr"][l], res)
        T["S"].append(S)
        T["xyzr"].append(gather(T["xyzr"][l], S.idx, S.batch, sf))
        T["ptr"].append(S.ptr)
    S0 = T["S"][0]
    order = S0.order if order0 is None else np.asarray(order0, np.int32)
    T["order"], T["sorted0"] = order, records(T["xyzr"][0][order][:, :3], order)
    n0 = len(T["xyzr"][0])
    T["sa"] = [ball(T["sorted0"], T["ptr"][0], T["xyzr"][0], T["ptr"][1], CHAIN_RES[0] * 2, CHAIN_K, X_INDEX_IN_W, qidx=S0.idx, rows=n0)]
    for l in (1, 2):
        T["sa"].append(knn(T["xyzr"][l], T["ptr"][l], T["xyzr"][l], T["ptr"][l + 1], CHAIN_K, 0, qidx=T["S"][l].idx, rows=n0))
    T["hint"], T["fp"] = {}, {}
    for f in (2, 1, 0):
        q, fl, rank = (T["sorted0"], Q_ROW_IN_W, S0.inv[order]) if f == 0 else (T["xyzr"][f], 0, T["S"][f].inv)
        T["hint"][f] = knn_hint2(q, rank, T["ptr"][f], T["xyzr"][f + 1])
        T["fp"][f] = knn(T["xyzr"][f + 1], T["ptr"][f + 1], q, T["ptr"][f], 2, fl, rows=n0)
    return T


# ---- cases: p2w_knn_hint2 -------------------------------------------------------------------------------------------------------------

def _hint2_case(pts, res=0.25, sorted_queries=False):
    """(q, rank, ptr_q, xc, ptr_c, keys_c, grid, cell_start_c): a fine level and its sampled level (no round trip), queries in their own or
    in cell-sorted order."""
    pts = [np.asarray(v, F).reshape(-1, 3) for v in pts]
    P, ptr = np.concatenate(pts), _ptr([len(v) for v in pts])
    x = records(P, np.arange(len(P)))
    S = sample(x, ptr, res)
    xc = x[S.idx]
    return ((x[S.order], S.rank_sorted) if sorted_queries else (x, S.inv)) + (ptr, xc, S.ptr, S.cell_keys, S.grid, S.cell_start())


def _hint2_ends(sorted_queries):
    rng = np.random.default_rng(85)
    return _hint2_case([rng.uniform(0, 1, (1, 3)), rng.uniform(0.3, 0.45, (30, 3)), rng.uniform(0, 1, (50, 3)), rng.uniform(0.5, 0.7, (9, 3)),
                        rng.uniform(0, 1, (40, 3)), rng.uniform(0, 1, (1, 3))], sorted_queries=sorted_queries)


HINT2 = {
    "hint2_voxel_ends_own_order": lambda: _hint2_ends(False),       # voxels of 1, 30 (one cell), 50, 9 (one cell), 40, 1 points: the +-8 windows
    "hint2_voxel_ends_sorted_order": lambda: _hint2_ends(True),     # of the first and last queries of a voxel reach into the neighbours' ranks
    "hint2_one_point": lambda: _hint2_case([[[0.5, 0.5, 0.5]]]),
    "hint2_single_cell": lambda: _hint2_case([np.random.default_rng(86).uniform(0.3, 0.45, (70, 3))]),
}


@functools.lru_cache(maxsize=None)
def hint2_case(name):
    return HINT2[name]()
