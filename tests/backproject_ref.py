"""A plain reference of the three back-projection entry points of ``csrc/p2w_geom.hip`` (``p2w_knn_refine_f64``, ``p2w_vote``,
``p2w_morton_order``): numpy and the standard library only, written from the comments of ``include/p2w.h`` and from nothing of the
package under test.

    dist2 / refine       ((dx*dx + dy*dy) + dz*dz) in float64, brute-force rows ascending by (d2, index): a total order
    within               T of a refinement input: how many candidates lie within the largest d2 of the row handed in
    vote                 np.median + the any-wood rule / the two vote sums (math.fsum) over the first min(deg, k) slots
    morton               float32 cell per axis, clamped to 21 bits, NaN -> 0, 3 x 21-bit interleave, stable argsort
    case generators      the seeded inputs of tests/test_gpu_backproject_kernels.py

``tests/test_backproject_ref_cpu.py`` holds it to ``oracle/backproject.py`` and scipy's KD-tree and asserts that every generated
case meets the condition it is named for."""
from __future__ import annotations

import functools
import math

import numpy as np

INT_MAX = 2 ** 31 - 1
SENTINEL = -77                      # what the GPU tests fill the slots with that a call must leave alone
SURVEY_OFFSET = (5.0e5, 6.2e6, 100.0)


# ---- refine -----------------------------------------------------------------------------------------------------------------------------

def dist2(cand64, q64):
    """[m, nc] float64: ((dx*dx + dy*dy) + dz*dz) of every (query, candidate) pair, every operation rounded on its own."""
    c, q = np.asarray(cand64, dtype=np.float64).reshape(-1, 3), np.asarray(q64, dtype=np.float64).reshape(-1, 3)
    dx = q[:, None, 0] - c[None, :, 0]
    dy = q[:, None, 1] - c[None, :, 1]
    dz = q[:, None, 2] - c[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def ranking(cand64, q64):
    """(d2 [m, nc], full [m, nc] int64): every query's candidates ascending by (d2, index)."""
    d2 = dist2(cand64, q64)
    index = np.broadcast_to(np.arange(d2.shape[1]), d2.shape)
    return d2, np.lexsort((index, d2), axis=1)


def refine(cand64, q64, k):
    """[m, min(k, nc)] int64: the min(k, nc) nearest candidates of every query, ascending by (d2, index)."""
    return ranking(cand64, q64)[1][:, :k]


def within(cand64, q64, rows, deg=None):
    """[m] int: the number of candidates with d2 <= R2, R2 = the largest d2 among the first deg[i] (default: all) entries of rows[i]."""
    d2 = dist2(cand64, q64)
    rows = np.asarray(rows)
    out = np.zeros(len(rows), dtype=np.int64)
    for i in range(len(rows)):
        r = rows[i] if deg is None else rows[i][:deg[i]]
        out[i] = int((d2[i] <= d2[i, r].max()).sum()) if len(r) else 0
    return out


# ---- vote -------------------------------------------------------------------------------------------------------------------------------

def vote(nbr, deg, k, pred, prob, any_wood):
    """(label [n] float32, pwood [n] float32, undecided [n] bool) of the first min(deg[i], k) slots of every row of nbr [n, k].

    PointCloudClassifier.compute_labels (predicter.py:112-127): pwood = np.median of the neighbours' probabilities (as float64, cast
    to float32); any_wood != 1: label = 1 if any neighbour's prediction > any_wood; any_wood == 1: the argmax over the classes {0, 1}
    of the summed probabilities, first maximum, sums exact (include/p2w.h; compute_labels takes its class count from the row length,
    which is the same for two slots and more).  No valid slot: label = 0, pwood = 0.  ``undecided``: the two sums differ
    by no more than 64 * 2^-52 * (v0 + v1) - an order of summation could then decide otherwise."""
    nbr = np.asarray(nbr).reshape(-1, k)
    pred, prob = np.asarray(pred, dtype=np.float64), np.asarray(prob, dtype=np.float64)
    n = nbr.shape[0]
    label, pwood, undecided = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=bool)
    for i in range(n):
        c = max(min(int(deg[i]), k), 0)
        if c == 0:
            continue
        j = nbr[i, :c]
        pr, pd = prob[j], pred[j]
        pwood[i] = np.float32(np.median(pr))
        if any_wood != 1:
            label[i] = 1.0 if np.any(pd > any_wood) else 0.0
        else:
            v0, v1 = math.fsum(pr[pd == 0]), math.fsum(pr[pd == 1])
            label[i] = 1.0 if v1 > v0 else 0.0
            undecided[i] = v1 != v0 and abs(v1 - v0) <= 64 * 2.0 ** -52 * (v0 + v1)
    return label, pwood, undecided


# ---- morton -----------------------------------------------------------------------------------------------------------------------------

MORTON_BITS = 21


def morton_cells(xyz32, lo, res):
    """[n, 3] uint64: floor((v - lo) / res) in float32, fmax(., 0) then fmin(., 2^21 - 1) (C's fmax / fmin: a NaN gives way), per axis."""
    x = np.asarray(xyz32, dtype=np.float32).reshape(-1, 3)
    lo, res = np.asarray(lo, dtype=np.float32).reshape(3), np.float32(res)
    with np.errstate(all="ignore"):
        f = np.floor((x - lo[None, :]) / res)
        assert f.dtype == np.float32
        c = np.fmin(np.fmax(f, np.float32(0.0)), np.float32(2 ** MORTON_BITS - 1))
    return c.astype(np.uint64)


def morton(xyz32, lo, res):
    """(keys [n] uint64, order [n] int64): bit b of axis a of the cell goes to bit 3 b + a of the key (x lowest); the order is the
    stable argsort of the keys."""
    c = morton_cells(xyz32, lo, res)
    keys = np.zeros(len(c), dtype=np.uint64)
    for b in range(MORTON_BITS):
        for a in range(3):
            keys |= ((c[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return keys, np.argsort(keys, kind="stable")


# ---- cases: refine ----------------------------------------------------------------------------------------------------------------------

CELL = 0.1
NC, M = 3000, 203
CELL32 = float(np.float32(CELL))    # the value the grid divides by


def uniform_cloud(shift=(0.0, 0.0, 0.0)):
    """(cand [3000, 3], q [203, 3]) float64: candidates uniform in a 2 m cube; queries inside it (80), up to 1 m (the first of each
    kind exactly 1 m) outside each of its 26 faces / edges / corners (52), and on cell boundaries of the 0.1 m grid that starts at
    the cloud's minimum (71: on one, two or all three axes).  ``shift`` is added to both before anything is derived."""
    g = np.random.default_rng(20)
    cand = g.random((NC, 3)) * 2.0
    lo, hi = cand.min(0), cand.max(0)
    q = [g.random((80, 3)) * 2.0]
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) == (0, 0, 0):
                    continue
                for u in (1.0, None):
                    p = lo + g.random(3) * (hi - lo)
                    for a, s in enumerate((sx, sy, sz)):
                        d = u if u is not None else 1.0 - g.random()          # (0, 1]
                        if s:
                            p[a] = lo[a] - d if s < 0 else hi[a] + d
                    q.append(p[None])
    b = lo + g.random((71, 3)) * (hi - lo)
    cells = g.integers(0, 21, (71, 3))
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 1, 1], [1, 0, 1]], dtype=bool)[np.arange(71) % 7]
    b[axes] = (lo + cells * CELL32)[axes]
    q.append(b)
    q = np.concatenate(q)
    assert q.shape == (M, 3)
    s = np.asarray(shift, dtype=np.float64)
    return cand + s, q + s


@functools.lru_cache(maxsize=None)
def uniform_ranked(shifted=False):
    """(cand, q, d2, full) of uniform_cloud, computed once."""
    cand, q = uniform_cloud(SURVEY_OFFSET if shifted else (0.0, 0.0, 0.0))
    d2, full = ranking(cand, q)
    for a in (cand, q, d2, full):
        a.setflags(write=False)
    return cand, q, d2, full


def rows_for_target(full, k, t, seed):
    """[m, k] int32 input rows: per query a random k-subset, in random order, of its t nearest that contains the t-th nearest."""
    g = np.random.default_rng(seed)
    rows = np.empty((len(full), k), dtype=np.int32)
    for i in range(len(full)):
        pick = np.concatenate([g.choice(t - 1, k - 1, replace=False), [t - 1]]).astype(np.int64)
        rows[i] = full[i, g.permutation(pick)]
    return rows


def farthest_rows(full, k, seed):
    """[m, k] int32: the k farthest candidates of every query, in random order."""
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(r[-k:]) for r in full]).astype(np.int32)


# (k, t): t nearest handed in as a k-subset -> T = t candidates within the bound.  t <= 128: the list, t >= 129: the extraction.
REFINE_TARGETS = [(64, t) for t in (64, 65, 127, 128, 129, 200, NC)] + \
                 [(k, t) for k in (1, 2, 31, 32) for t in (k, 128, 129)]

STAR_PAIRS = 70
TIE_CENTRES = {"star_odd": (0.5, 0.5, 0.5), "star_even": (1.5, 1.5, 0.5), "pile128": (0.5, 1.5, 1.5), "pile129": (1.5, 0.5, 1.5)}
TIE_KS = (1, 2, 31, 32, 64)


@functools.lru_cache(maxsize=None)
def tie_cloud():
    """(cand [3000, 3] float64, members: name -> int64 indices of the planted points).

    Uniform background in the 2 m cube with nothing within 0.45 m of four centres, where (at random indices of the cloud) stand:
      star_odd    70 pairs (c + (r, 0, 0), c + (0, r, 0)), r = j / 256: the places (1, 2), (3, 4), ... of the query c hold bit-equal d2
      star_even   the same behind one nearer point c + (0, 0, 1 / 512): the places (2, 3), (4, 5), ... tie
      pile128 / pile129   that many copies of the centre.
    The centres and offsets are dyadic, so every planted d2 is exact."""
    g = np.random.default_rng(21)
    cand = g.random((NC, 3)) * 2.0
    centres = np.array(list(TIE_CENTRES.values()))
    while True:
        near = (dist2(centres, cand) < 0.45 ** 2).any(1)
        if not near.any():
            break
        cand[near] = g.random((int(near.sum()), 3)) * 2.0
    r = np.arange(1, STAR_PAIRS + 1) / 256.0
    star = np.zeros((2 * STAR_PAIRS, 3))
    star[0::2, 0], star[1::2, 1] = r, r
    planted = {"star_odd": np.asarray(TIE_CENTRES["star_odd"]) + star,
               "star_even": np.asarray(TIE_CENTRES["star_even"]) + np.concatenate([[[0.0, 0.0, 1.0 / 512]], star]),
               "pile128": np.tile(TIE_CENTRES["pile128"], (128, 1)), "pile129": np.tile(TIE_CENTRES["pile129"], (129, 1))}
    slots = g.choice(NC, sum(len(p) for p in planted.values()), replace=False)
    members, s = {}, 0
    for name, p in planted.items():
        idx = slots[s:s + len(p)]
        s += len(p)
        cand[idx] = p[g.permutation(len(p))]
        members[name] = np.sort(idx).astype(np.int64)
    cand.setflags(write=False)
    return cand, members


def tie_case(k):
    """(q [6, 3], rows [6, k] int32, T [6]) of the tie cloud at k:
      0  a star's centre (star_odd for odd k, star_even for even k), handed its k + 1 nearest WITHOUT the k-th: T = k + 1, the k-th
         and (k + 1)-th d2 are bit-equal and the lower index must take the k-th place (the list);
      1  the same centre, handed the k farthest points of the star: T = the whole star > 128 (the extraction);
      2  beside pile128, handed the pile's k HIGHEST indices: T = 128, the answer is its k lowest (the list, full);
      3  beside pile129 likewise: T = 129 (the extraction);
      4  beside pile129, handed its k lowest indices in descending order;
      5  beside pile128, handed its k lowest indices in random order."""
    cand, members = tie_cloud()
    g = np.random.default_rng(22 + k)
    star = "star_odd" if k % 2 else "star_even"
    beside = np.array([2.0 ** -10, 0.0, 0.0])
    q = np.array([TIE_CENTRES[star], TIE_CENTRES[star], TIE_CENTRES["pile128"] + beside, TIE_CENTRES["pile129"] + beside,
                  TIE_CENTRES["pile129"] + beside, TIE_CENTRES["pile128"] + beside])
    full = ranking(cand, q[:1])[1][0]
    n_star = len(members[star])
    rows = np.stack([g.permutation(np.concatenate([full[:k - 1], full[k:k + 1]])),
                     g.permutation(full[n_star - k:n_star]),
                     g.permutation(members["pile128"][-k:]),
                     g.permutation(members["pile129"][-k:]),
                     members["pile129"][:k][::-1],
                     g.permutation(members["pile128"][:k])]).astype(np.int32)
    return q, rows, np.array([k + 1, n_star, 128, 129, 129, 128])


def few_cloud(nc):
    """(cand [nc, 3], q [37, 3], rows [37, 64] int32, deg [37] int32) for nc < k = 64: every query is handed all nc candidates in
    random order, the slots behind them hold SENTINEL.  The queries lie in and up to 1 m around the unit cube of the candidates."""
    g = np.random.default_rng(23 + nc)
    cand = g.random((nc, 3))
    q = g.random((37, 3)) * 3.0 - 1.0
    rows = np.full((37, 64), SENTINEL, dtype=np.int32)
    for i in range(37):
        rows[i, :nc] = g.permutation(nc)
    return cand, q, rows, np.full(37, nc, dtype=np.int32)


# ---- cases: vote ------------------------------------------------------------------------------------------------------------------------

VOTE_NC = 500
VOTE_NS = (1, 3, 4, 5, 257)
VOTE_KS = (1, 2, 31, 32, 33, 63, 64)
VOTE_ANY_WOOD = (1.0, 0.5, 0.9, 0.0)
GARBAGE = (-1, VOTE_NC + 7, INT_MAX)


@functools.lru_cache(maxsize=None)
def vote_table(rare=False):
    """(pred, prob) float32 [500]: half the probabilities are multiples of 1/16 (many repeated values), the rest uniform float32.
    The predictions are drawn apart from them (were they prob >= 0.5, the wood sum would win nearly every vote): half wood, or with
    ``rare`` one in thirty (the any-wood rule then gives both labels at every row length)."""
    g = np.random.default_rng(24)
    prob = g.random(VOTE_NC).astype(np.float32)
    coarse = g.random(VOTE_NC) < 0.5
    prob[coarse] = (g.integers(0, 17, int(coarse.sum())) / 16.0).astype(np.float32)
    pred = (g.random(VOTE_NC) < (1.0 / 30 if rare else 0.5)).astype(np.float32)
    pred.setflags(write=False)
    prob.setflags(write=False)
    return pred, prob


def vote_case(n, k, variant=0):
    """(nbr [n, k] int32, deg [n] int32): deg over 0 .. k; the rows 0 .. 4 (as far as n reaches, rotated by ``variant``) have deg 0,
    1, k + 5 (clamped by the call), k and k - 1.  The slots from deg[i] on hold GARBAGE, which no call may follow."""
    g = np.random.default_rng(1000 * k + 10 * n + variant)
    nbr = g.integers(0, VOTE_NC, (n, k)).astype(np.int32)
    deg = (g.permutation(np.arange(n) % (k + 1)) if n > k + 1 else g.integers(0, k + 1, n)).astype(np.int32)   # every count
    forced = [0, 1, k + 5, k, k - 1]
    forced = forced[variant % 5:] + forced[:variant % 5]
    deg[:min(n, 5)] = forced[:min(n, 5)]
    for i in range(n):
        for s in range(max(int(deg[i]), 0), k):
            nbr[i, s] = GARBAGE[(i + s) % 3]
    return nbr, deg


def vote_planted(k):
    """(nbr [r, k] int32, deg [r] int32, pred, prob, any_wood, label [r]) for any_wood = 1.0 and 0.5 at k in {2, 32, 64}: rows whose
    label the construction fixes.  Probabilities are multiples of 2^-10, so every sum is exact.

    any_wood = 1 (h = k / 2 wood points w_i and h others with the same probabilities in another order):
      all of them                        v1 == v0                -> 0 (argmax keeps the first maximum)
      one wood point 2^-10 heavier       v1 == v0 + 2^-10        -> 1
      one other point 2^-10 heavier      v0 == v1 + 2^-10        -> 0
      deg = 2: one of each, equal        v1 == v0                -> 0
      deg = 0                                                    -> 0
    any_wood = 0.5 (k slots of non-wood points, one wood point):
      the wood point in the last valid slot, deg = k and deg = k / 2     -> 1
      the wood point in slot deg[i], just outside, deg = k / 2 and 0     -> 0"""
    g = np.random.default_rng(25 + k)
    h = k // 2
    w = (g.integers(1, 1024, h) / 1024.0).astype(np.float32)
    e = np.float32(2.0 ** -10)
    # 0 .. h-1 wood, h .. 2h-1 others (the same values, reversed), 2h: wood w0 + e, 2h + 1: other w[h-1] + e, 2h + 2: other = w0
    prob = np.concatenate([w, w[::-1], [w[0] + e, w[h - 1] + e, w[0]]]).astype(np.float32)
    pred = np.concatenate([np.ones(h), np.zeros(h), [1.0, 0.0, 0.0]]).astype(np.float32)
    every = np.arange(2 * h)
    pad = np.full(k, GARBAGE[1], dtype=np.int64)

    def row(valid):
        r = pad.copy()
        r[:len(valid)] = valid
        return r
    heavy_wood, heavy_other = every.copy(), every.copy()
    heavy_wood[0], heavy_other[h] = 2 * h, 2 * h + 1
    tie = [(row(g.permutation(every)), k, 0.0), (row(g.permutation(heavy_wood)), k, 1.0), (row(g.permutation(heavy_other)), k, 0.0),
           (row([0, 2 * h + 2]), 2, 0.0), (row([]), 0, 0.0)]
    others = np.arange(h, 2 * h)
    last = np.concatenate([others, others])[:k]
    full, half, outside, none = last.copy(), last.copy(), last.copy(), last.copy()
    full[k - 1], half[h - 1], outside[h], none[0] = 0, 0, 0, 0                   # (point 0 is wood; h = k / 2 < k)
    any_ = [(full, k, 1.0), (half, h, 1.0), (outside, h, 0.0), (none, 0, 0.0)]
    out = []
    for rows, aw in ((tie, 1.0), (any_, 0.5)):
        out.append((np.stack([r for r, _, _ in rows]).astype(np.int32), np.array([d for _, d, _ in rows], dtype=np.int32), pred, prob,
                    aw, np.array([lab for _, _, lab in rows], dtype=np.float32)))
    return out


VOTE_PLANTED_KS = (2, 32, 64)


# ---- cases: morton ----------------------------------------------------------------------------------------------------------------------

MORTON_NS = (1, 255, 256, 257, 4097)
MORTON_LO = (0.25, -1.0, 3.0)
# cell sizes: 5 bits per axis in the 2 m box (two radix passes), 9 bits (four), and 2^-20: every one of the 21 bits (eight)
MORTON_RES = (0.1, 2.0 ** -8, 2.0 ** -20)


def morton_records(n, beyond=True, seed=26):
    """[n, 4] float32 records (x, y, z, w): uniform in the 2 m box above MORTON_LO, with (as far as n reaches) records below lo on
    one or all axes, NaN coordinates on one or all axes, runs of up to 300 records in one cell (equal keys: the order among them is
    the input order) and, with ``beyond``, records far beyond the 2^21-cell clamp of every MORTON_RES (1e7, 1e30, +inf; -inf below).
    Without them the widest key - the radix sort's pass count - follows the cell size."""
    g = np.random.default_rng(seed + n)
    lo = np.asarray(MORTON_LO, dtype=np.float32)
    rec = np.zeros((n, 4), dtype=np.float32)
    rec[:, :3] = lo + (g.random((n, 3)) * 2.0).astype(np.float32)
    rec[:, 3] = g.random(n).astype(np.float32)
    special = np.array([[-5.0, 0.5, 3.5], [-5.0, -7.0, -2.0], [np.nan, 0.0, 4.0], [np.nan, np.nan, np.nan], [1.0, np.nan, 3.0],
                        [0.25, -1.0, 3.0], [2.25, 1.0, 5.0], [4.0, 4.0, 7.0]], dtype=np.float32)
    if beyond:
        special = np.concatenate([special, np.array([[1e7, 0.0, 4.0], [1e30, 1e30, 1e30], [np.inf, 0.0, 4.0], [-np.inf, 0.0, np.inf],
                                                     [1.0, np.nan, 1e7]], dtype=np.float32)])
    if n >= 255:
        at = g.permutation(n)                                   # disjoint groups
        n_run, n_tiny = min(300, n // 3), n // 8
        rec[at[:n_run], :3] = lo + np.float32(1.03125)          # one position: one cell at every MORTON_RES
        # several records per cell of the finest grid too
        rec[at[n_run:n_run + n_tiny], :3] = lo + (g.integers(0, 3, (n_tiny, 3)) * 2.0 ** -20).astype(np.float32)
        rec[at[n_run + n_tiny:n_run + n_tiny + 3 * len(special)], :3] = np.tile(special, (3, 1))
    return rec
