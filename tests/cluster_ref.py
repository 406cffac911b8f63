"""A plain reference of ``csrc/p2w_cluster.hip`` and of the grid it is handed: numpy and the standard library only, written from the
comments of ``include/p2w.h`` and ``pointstowood_amd/plotgrid.py`` and from nothing of the package under test.

    safe_cell / grid     the arithmetic of plotgrid.safe_cell and plotgrid.build written out: origin = per-axis minimum, local coordinates
                         rounded once to float32, float32 key division, stable sort by key, the cell table, the 56-byte p2w_grid
    joined / edges       ((dx*dx + dy*dy) + dz*dz) <= r*r in float64 on the caller's coordinates, every pair i < j, blocked O(n^2)
    roots / number       union-find whose root is the smallest index; components of min_size <= size <= max_size numbered in ascending
                         order of their smallest index, -1 elsewhere; the two counts
    pairs                unordered pairs of distinct points in equal or adjacent cells = what the link stage measures
    CASES                named, seeded clouds of tests/test_gpu_cluster_kernels.py: name -> () -> (xyz, r, min_size, max_size, cell)

``tests/test_cluster_ref_cpu.py`` pins it to the seven fixtures recorded from the reference project (tests/golden/cluster) and to
scipy, and asserts that every case meets the condition it is named for and that the cases tell a list of wrong kernels apart."""
from __future__ import annotations

import itertools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

BIG = 1 << 62                                                              # "no upper bound" as the int64 the C ABI takes
_EPS32 = 2.0 ** -23


# ---- the grid --------------------------------------------------------------------------------------------------------------------------

def safe_cell(r, extent):
    """The smallest legal cell (a float32 value, as float) for tolerance r and largest per-axis extent `extent`: r (1 + 2^-20) plus four
    float32 roundings of the extent, at least 2^-20 of the extent, 1 where that is not positive, rounded up to float32."""
    c = max(r * (1.0 + 2.0 ** -20) + 4.0 * _EPS32 * extent, extent * 2.0 ** -20)
    if not c > 0.0:
        c = 1.0
    c32 = np.float32(c)
    if float(c32) < c:
        c32 = np.nextafter(c32, np.float32(np.inf))
    return float(c32)


def extent(xyz):
    """The largest float64 coordinate local to the per-axis minimum: what the host layer hands safe_cell."""
    x = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return float((x - x.min(0)).max())


Grid = namedtuple("Grid", "cell origin dims n_cells cells keys order keys_sorted xyz_sorted cell_start image")


def grid(xyz, cell):
    """The cell grid of the float64 points xyz [n >= 1, 3] at cell size `cell` (rounded once to float32).

    cell        float: the float32 value every quotient is divided by
    origin      [3] float64: the per-axis minimum
    dims        [3] int64: trunc(fl32((hi - lo) / cell)) + 1 of the float32 local coordinates (lo = 0: the minimum's own)
    cells       [n, 3] int64: trunc(fl32((u - lo) / cell)) per point and axis;  keys [n] int64 = (cz * d1 + cy) * d0 + cx
    order       [n] int32: sorted position -> point index, the stable argsort of the keys;  keys_sorted uint64, xyz_sorted float64
    cell_start  [n_cells + 1] int32: the number of keys below every cell id
    image       [56] uint8: the p2w_grid {float lo[3], res, hi[3]; int32 b_lo = 0; int64 dims[3]}"""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    c = np.float32(cell)
    origin = x.min(0)
    u = (x - origin).astype(np.float32)
    lo, hi = u.min(0), u.max(0)
    dims = np.trunc((hi - lo) / c).astype(np.int64) + 1
    cells = np.trunc((u - lo) / c).astype(np.int64)
    keys = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
    order = np.argsort(keys, kind="stable").astype(np.int32)
    keys_sorted = keys[order].astype(np.uint64)
    n_cells = int(dims[0] * dims[1] * dims[2])
    assert n_cells <= 1 << 24, "a reference grid is small enough for its table"
    cell_start = np.searchsorted(keys[order], np.arange(n_cells + 1), side="left").astype(np.int32)
    image = np.zeros(56, dtype=np.uint8)
    image[0:12] = lo.view(np.uint8)
    image[12:16] = np.array([c], dtype=np.float32).view(np.uint8)
    image[16:28] = hi.view(np.uint8)
    image[32:56] = dims.view(np.uint8)
    return Grid(float(c), origin, dims, n_cells, cells, keys, order, keys_sorted, np.ascontiguousarray(x[order]), cell_start, image)


def pairs(g):
    """The number of unordered pairs of distinct points whose cells are equal or differ by at most 1 on every axis, each counted
    once: every point counts the other points of the 27 cells around it, and every pair is met from both of its ends."""
    count = {}
    for c in map(tuple, g.cells.tolist()):
        count[c] = count.get(c, 0) + 1
    total = 0
    for (cx, cy, cz), m in count.items():
        around = sum(count.get((cx + ox, cy + oy, cz + oz), 0) for ox in (-1, 0, 1) for oy in (-1, 0, 1) for oz in (-1, 0, 1))
        total += m * (around - 1)
    assert total % 2 == 0
    return total // 2


# ---- the clustering --------------------------------------------------------------------------------------------------------------------

def joined(dx, dy, dz, r):
    """The predicate of include/p2w.h: every operation rounded on its own, no fused multiply-add."""
    return (dx * dx + dy * dy) + dz * dz <= r * r


def edges(xyz, r, pred=joined, block=128):
    """[E, 2] int64: every pair i < j that `pred` joins, by rows of `block` points against all later points."""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    out = [np.zeros((0, 2), dtype=np.int64)]
    for s in range(0, n, block):
        e = min(s + block, n)
        dx, dy, dz = (x[s:e, None, a] - x[None, s:, a] for a in range(3))
        m = pred(dx, dy, dz, r)
        m &= np.arange(s, n)[None, :] > np.arange(s, e)[:, None]
        i, j = np.nonzero(m)
        out.append(np.stack([i + s, j + s], axis=1))
    return np.concatenate(out)


def roots(n, e):
    """[n] int64: the smallest index of every point's component under the edges e, by a union-find that hooks the larger root under
    the smaller."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in np.asarray(e).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    return np.array([find(i) for i in range(n)], dtype=np.int64).reshape(n)


def number(root, min_size, max_size):
    """(labels [n] int64, n_kept, n_noise): the components of min_size <= size <= max_size numbered 0, 1, ... in ascending order of
    their smallest index (= their root); every other point -1."""
    root = np.asarray(root, dtype=np.int64)
    n = len(root)
    size = np.bincount(root, minlength=n)
    kept_root = (root == np.arange(n)) & (size >= min_size) & (size <= max_size)
    cid = np.cumsum(kept_root) - kept_root
    lab = np.where(kept_root[root], cid[root], -1).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    return lab, int(kept_root.sum()), int((lab == -1).sum())


def labels(xyz, r, min_size, max_size):
    """(labels, n_kept, n_noise) of the float64 points xyz [n, 3]."""
    x = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return number(roots(len(x), edges(x, r)), min_size, max_size)


# ---- the predicate's edge cases --------------------------------------------------------------------------------------------------------

def sums(dx, dy, dz):
    """The squared distance as the kernel must form it and as a contracting compiler could: (separate, fma(dz, dz, dx*dx + dy*dy),
    and the same with the inner sum fused either way), the fused ones by exact rational arithmetic rounded once."""
    F = Fraction
    sep = (dx * dx + dy * dy) + dz * dz
    outer = float(F(dx * dx + dy * dy) + F(dz) ** 2)
    full_x = float(F(float(F(dx) ** 2 + F(dy * dy))) + F(dz) ** 2)
    full_y = float(F(float(F(dy) ** 2 + F(dx * dx))) + F(dz) ** 2)
    return sep, outer, full_x, full_y


def exact_root(v):
    """A double r with r*r == v exactly, or None."""
    r = math.sqrt(v)
    for c in (r, math.nextafter(r, 0.0), math.nextafter(r, math.inf)):
        if c * c == v:
            return c
    return None


def fma_flip_search(seed, draws):
    """{"sep_joins": (dx, dy, dz, r), "fma_joins": (...)}: the first draw of each kind among `draws` uniform triples in [0.01, 0.08] for
    which the separately rounded sum and every contracted one fall on opposite sides of r*r, r*r being the lower of the two exactly.
    How FMA_SEP_JOINS and FMA_FMA_JOINS below were found (seed 0)."""
    g = np.random.default_rng(seed)
    found = {}
    for _ in range(draws):
        dx, dy, dz = (float(v) for v in g.uniform(0.01, 0.08, 3))
        sep, outer, full_x, full_y = sums(dx, dy, dz)
        r = exact_root(min(sep, outer))
        if sep == outer or r is None or len({v <= r * r for v in (outer, full_x, full_y)}) != 1:
            continue
        found.setdefault("sep_joins" if sep < outer else "fma_joins", (dx, dy, dz, r))
    return found


FMA_SEP_JOINS = tuple(float.fromhex(h) for h in ("0x1.6d97265f64e72p-7", "0x1.12240e4928034p-4", "0x1.2eaa4fbb72854p-4", "0x1.9ae93797815f9p-4"))
FMA_FMA_JOINS = tuple(float.fromhex(h) for h in ("0x1.39e7fd2f09799p-5", "0x1.8782b955beb61p-6", "0x1.0bec401770c01p-6", "0x1.89733452fe4b8p-5"))
PLOT = np.array([512345.25, 6012345.5, 80.0])                               # a plot's easting, northing and height: exact in float32


def _two(dx, dy, dz, r, at=(0.0, 0.0, 0.0)):
    return np.array([at, (at[0] + dx, at[1] + dy, at[2] + dz)], dtype=np.float64), r, 1, BIG, None


def _pred_equal():
    return _two(0.1, 0.0, 0.0, 0.1)                                        # d2 = r*r + 0 + 0


def _pred_next_above():
    """dy*dy = one unit in the last place of r*r (to a rounding), so dx*dx + dy*dy is the next double above r*r."""
    r = 0.1
    up = math.nextafter(r * r, math.inf)
    dy = math.sqrt(up - r * r)
    assert r * r + dy * dy == up
    return _two(r, dy, 0.0, r)


# ---- the stencil cases -----------------------------------------------------------------------------------------------------------------

OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
HALF = [o for o in OFFSETS if o[::-1] > (0, 0, 0)]                         # the 13 of them that lead to a higher key: z, then y, then x
STENCIL_R, STENCIL_E = 0.25, 3.25


def stencil(o, where, rev, far, safe):
    """Two points alone in the cells A and A + o of a cubic grid over [0, 3.25]^3 and two far anchors (0, E, 0), (E, 0, E) that fix the
    grid's extent and are joined to nothing.  `where`: "in" = A in the middle, "lo" / "hi" = the lower / upper of the two cells is the
    first / last of the grid on every axis.  On the axes o steps along the pair straddles the shared cell boundary at +-0.05 (near:
    within r = 0.25) or +-0.2 (far: apart, in the same two cells); on the others both sit 0.4 cells into A.  `rev`: the point of the
    higher key has the lower index.  `safe`: the safe cell (13 cells per axis), else cell = 2 r (7 per axis)."""
    r, E = STENCIL_R, STENCIL_E
    cell = safe_cell(r, E) if safe else 2.0 * r
    d = int(np.trunc(np.float32(E) / np.float32(cell))) + 1
    delta = 0.2 if far else (0.1 if safe else 0.05)
    pa, pb = np.zeros(3), np.zeros(3)
    for ax in range(3):
        a = {"in": d // 2, "lo": 1 if o[ax] < 0 else 0, "hi": d - 2 if o[ax] > 0 else d - 1}[where]
        if o[ax] == 0:
            pa[ax] = pb[ax] = a * cell + 0.4 * cell
        else:
            bound = max(a, a + o[ax]) * cell
            pa[ax], pb[ax] = bound - o[ax] * delta, bound + o[ax] * delta
    low_first = o[::-1] > (0, 0, 0)                                        # the key order of the two cells: z, then y, then x
    first, second = (pa, pb) if low_first != rev else (pb, pa)
    xyz = np.array([first, second, (0.0, E, 0.0), (E, 0.0, E)])
    return xyz, r, 1, BIG, (None if safe else cell)


def _stencil_cases():
    out = {}
    for safe in (False, True):
        for o in OFFSETS:
            if safe and sum(v != 0 for v in o) != 1:
                continue
            for where, rev, far in itertools.product(("in", "lo", "hi"), (False, True), (False, True)):
                name = "stencil%s_%+d%+d%+d_%s_%s_%s" % ("safe" if safe else "", *o, where, "rev" if rev else "fwd", "far" if far else "near")
                out[name] = (o, where, rev, far, safe)
    return out


STENCIL = _stencil_cases()                                                 # name -> (o, where, rev, far, safe)


def _face_wrap():
    """Six singletons at cell centres of the 7^3 grid of the stencil cases, no two in adjacent cells: pairs = 0.  (6,1,1) and (0,2,1)
    are neighbours in key order only (an x run that is not clamped at the face), (2,0,1) and (2,6,1) are a y - 1 row apart only when
    the row index wraps."""
    cell = 2.0 * STENCIL_R
    c = np.array([(6, 1, 1), (0, 2, 1), (2, 0, 1), (2, 6, 1), (0, 6, 0), (6, 0, 6)], dtype=np.float64)
    xyz = c * cell + 0.5 * cell
    xyz[4], xyz[5] = (0.0, STENCIL_E, 0.0), (STENCIL_E, 0.0, STENCIL_E)
    return xyz, STENCIL_R, 1, BIG, cell


# ---- numbering, sizes, union-find shapes, grid shapes ----------------------------------------------------------------------------------

def _arranged(comps, g):
    """The points of the components `comps` (a list of [m, 3] arrays) indexed so that component k's smallest index is k and the rest
    of the indices are shuffled among all of them."""
    first = np.array([c[0] for c in comps])
    rest = np.concatenate([c[1:] for c in comps])
    return np.concatenate([first, rest[g.permutation(len(rest))]])


def _chains(sizes, r):
    """One straight chain of spacing 0.6 r per size, the chains 5 r apart in y and z."""
    return [np.array([0.0, 5.0 * r * (k % 4), 5.0 * r * (k // 4)]) + np.arange(m)[:, None] * np.array([0.6 * r, 0.0, 0.0])
            for k, m in enumerate(sizes)]


SIZES_AT_BOUNDS = [2, 3, 6, 5, 2, 3, 4, 6, 5, 1]                           # min_size 3, max_size 5: kept are 3, 5, 3, 4, 5


def _sizes_at_bounds(mn=3, mx=5):
    return _arranged(_chains(SIZES_AT_BOUNDS, 0.1), np.random.default_rng(41)) + PLOT, 0.1, mn, mx, None


def _cloud(n, seed, r=0.1, mean_neighbours=1.5):
    """n uniform points in a cube in which a ball of radius r holds `mean_neighbours` others on average: components of many sizes."""
    side = (n * 4.0 / 3.0 * math.pi * r ** 3 / mean_neighbours) ** (1.0 / 3.0)
    return np.random.default_rng(seed).uniform(0.0, side, (n, 3))


def _n_points(n):
    if n == 1:
        return np.array([[1.5, -2.25, 3.0]]), 0.1, 1, BIG, None
    if n == 2:
        return np.array([[1.5, -2.25, 3.0], [1.5, -2.25, 3.0625]]), 0.1, 2, BIG, None
    return _cloud(n, n), 0.1, 2, BIG, None


def _with_tail(n_cloud, seed, tail, mn):
    """A cloud and, behind it in index order, a chain of `tail` points far from it."""
    x = _cloud(n_cloud, seed)
    t = np.array([x[:, 0].max() + 1.0, 0.0, 0.0]) + np.arange(tail)[:, None] * np.array([0.06, 0.0, 0.0])
    return np.concatenate([x, t]), 0.1, mn, BIG, None


def zigzag(n, r):
    """n points along x at spacing 0.7 r, alternately 0.01 r below and above the first cell boundary in y, and the safe cell of the
    cloud they form with an anchor at the origin, 1 to the left of the line: consecutive points are joined, every point has a cell of
    its own.  Returns ([n, 3] in the order along the line, the anchor, the cell)."""
    E = 1.0 + (n - 1) * 0.7 * r
    c = safe_cell(r, E)
    k = np.arange(n)
    line = np.stack([1.0 + k * 0.7 * r, c + np.where(k % 2 == 0, -0.01 * r, 0.01 * r), np.zeros(n)], axis=1)
    return line, np.zeros((1, 3)), c


def bit_reversed(n):
    bits = n.bit_length() - 1
    assert 1 << bits == n
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)])


def _line(n, how):
    """The zigzag line with point index -> position along the line given by `how`; the anchor is the last point."""
    r = 0.05
    line, anchor, _ = zigzag(n, r)
    pos = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "bit_reversed": bit_reversed(n) if n & (n - 1) == 0 else None,
           "shuffled": np.random.default_rng(43).permutation(n)}[how]
    return np.concatenate([line[pos], anchor]), r, 1, BIG, None


def _one_cell():
    """A 10 x 10 x 15 lattice of spacing 0.09 (axis neighbours joined at r = 0.1, diagonals not) in one cell of size 2, shuffled."""
    idx = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(15), indexing="ij"), -1).reshape(-1, 3)
    return (idx * 0.09)[np.random.default_rng(44).permutation(len(idx))] + PLOT, 0.1, 1, BIG, 2.0


def _comb():
    """A spine of 400 points along x at spacing 0.08 and a tooth of 12 points along y on every fourth of them (a diagonal step is
    0.113 > r), shuffled: one component, a tree."""
    s = 0.08
    spine = np.stack([np.arange(400) * s, np.zeros(400), np.zeros(400)], axis=1)
    kx, ky = np.meshgrid(np.arange(0, 400, 4), np.arange(1, 13), indexing="ij")
    teeth = np.stack([kx.ravel() * s, ky.ravel() * s, np.zeros(kx.size)], axis=1)
    x = np.concatenate([spine, teeth])
    return x[np.random.default_rng(45).permutation(len(x))], 0.1, 1, BIG, None


LINES_MIN = LINES_MAX = 1000


def _interleaved_lines():
    """Line B (1001 points, y = 0, even indices) and line A (1000 points, y = 0.12, odd indices) along x at spacing 0.07, r = 0.1, in
    cells of 0.4: the lines are 0.12 apart and share every cell.  min_size = max_size = 1000: A is kept, B is one too large."""
    kb, ka = np.arange(LINES_MAX + 1), np.arange(LINES_MIN)
    x = np.zeros((len(kb) + len(ka), 3))
    x[0::2, 0] = kb * 0.07
    x[1::2, 0], x[1::2, 1] = ka * 0.07, 0.12
    return x, 0.1, LINES_MIN, LINES_MAX, 0.4


def _on_axes(axes, n, seed, span):
    """n uniform points of [0, span] on the given axes, the other coordinates constant: a grid one cell thick there."""
    x = np.tile(np.array([3.0, -7.5, 11.25]), (n, 1))
    x[:, list(axes)] += np.random.default_rng(seed).uniform(0.0, span, (n, len(axes)))
    return x, 0.1, 2, BIG, None


def _duplicates():
    """Tolerance 0: ten positions held by 1 to 6 identical points each, shuffled; min_size 2, so the single ones are noise."""
    g = np.random.default_rng(46)
    pos = g.uniform(0.0, 2.0, (10, 3))
    x = np.repeat(pos, [1, 2, 3, 4, 5, 6, 1, 2, 3, 1], axis=0)
    return x[g.permutation(len(x))] + PLOT, 0.0, 2, BIG, 0.25


CASES = {
    **{name: (lambda a=a: stencil(*a)) for name, a in STENCIL.items()},
    "face_wrap": _face_wrap,
    "pred_equal": _pred_equal,
    "pred_next_above": _pred_next_above,
    "pred_fma_sep_joins": lambda: _two(*FMA_SEP_JOINS),
    "pred_fma_fma_joins": lambda: _two(*FMA_FMA_JOINS),
    "pred_f64_joins_f32_not": lambda: _two(0.1095, 0.0, 0.0, 0.11, at=tuple(PLOT)),
    "pred_f32_joins_f64_not": lambda: _two(0.105, 0.0, 0.0, 0.1, at=tuple(PLOT)),
    "tol0_duplicates": _duplicates,
    "sizes_at_bounds": _sizes_at_bounds,
    "sizes_min_above_max": lambda: _sizes_at_bounds(5, 3),
    **{"n_%d" % n: (lambda n=n: _n_points(n)) for n in (1, 2, 255, 256, 257, 4096, 4097)},
    "n_8192": lambda: (_cloud(8192, 8192), 0.1, 2, BIG, None),
    "n4097_kept_roots_both_sides": lambda: _with_tail(4096, 47, 1, 1),
    "root_above_4096": lambda: _with_tail(4500, 48, 100, 2),
    "last_kept_singleton": lambda: _with_tail(300, 49, 1, 1),
    "last_noise_singleton": lambda: _with_tail(300, 49, 1, 2),
    "last_kept_member": lambda: _with_tail(300, 49, 5, 2),
    "line_ascending": lambda: _line(2048, "ascending"),
    "line_descending": lambda: _line(2048, "descending"),
    "line_bit_reversed": lambda: _line(4096, "bit_reversed"),
    "line_shuffled": lambda: _line(8191, "shuffled"),
    "one_cell": _one_cell,
    "comb": _comb,
    "interleaved_lines": _interleaved_lines,
    "dims_d11": lambda: _on_axes((0,), 400, 50, 20.0),
    "dims_1d1": lambda: _on_axes((1,), 400, 51, 20.0),
    "dims_11d": lambda: _on_axes((2,), 400, 52, 20.0),
    "plane_xy": lambda: _on_axes((0, 1), 600, 53, 3.0),
    "plane_xz": lambda: _on_axes((0, 2), 600, 54, 3.0),
    "plane_yz": lambda: _on_axes((1, 2), 600, 55, 3.0),
    "dims_111": lambda: (np.tile(PLOT, (5, 1)), 0.1, 1, BIG, None),
}

Solved = namedtuple("Solved", "xyz r min_size max_size cell grid edges root labels n_kept n_noise pairs")
_solved = {}


def solved(name):
    """The case `name`, its cell (the safe cell where the case leaves it open), its grid and its answers - worked out once and shared
    by every test of a run; nothing in it is written to afterwards."""
    if name not in _solved:
        xyz, r, mn, mx, cell = CASES[name]()
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        g = grid(xyz, safe_cell(r, extent(xyz)) if cell is None else cell)
        e = edges(xyz, r)
        root = roots(len(xyz), e)
        lab, n_kept, n_noise = number(root, mn, mx)
        for a in (xyz, e, root, lab, *[f for f in g if isinstance(f, np.ndarray)]):
            a.setflags(write=False)
        _solved[name] = Solved(xyz, r, mn, mx, cell, g, e, root, lab, n_kept, n_noise, pairs(g))
    return _solved[name]
