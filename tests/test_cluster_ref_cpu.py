"""tests/cluster_ref.py without a GPU: the plain reference reproduces the seven fixtures recorded from the reference project
(tests/golden/cluster) and agrees with scipy, every case of tests/test_gpu_cluster_kernels.py meets the condition it is named for,
and a list of wrong kernels - written here as variants of the reference - each change the answer of a named case, so no GPU test
can pass by being vacuous."""
import math
import os

import numpy as np
import pytest

from pointstowood_amd import plotgrid
from tests import cluster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster")
FIXTURES = ["blobs_noise", "lattice_tie", "lattice_easting", "duplicates_tol0", "filter_minmax", "single_point", "empty"]
ALL = sorted(R.CASES)


# ---- the reference against the recorded labels and against scipy -----------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_reference_reproduces_the_recorded_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    lab, n_kept, n_noise = R.labels(z["xyz"], float(z["tolerance"]), float(z["min_size"]), float(z["max_size"]))
    want = z["labels"]
    assert lab.dtype == np.int64 and np.array_equal(lab, want)
    assert n_kept == (int(want.max()) + 1 if want.size else 0) and n_noise == int((want == -1).sum())


@pytest.mark.parametrize("n,seed,offset,r,mn,mx", [(3000, 0, (0.0, 0.0, 0.0), 0.1, 1, R.BIG), (4000, 1, tuple(R.PLOT), 0.12, 3, 40)])
def test_reference_agrees_with_scipy(n, seed, offset, r, mn, mx):
    pytest.importorskip("scipy")
    from tests.test_gpu_cluster import _scipy_labels
    x = R._cloud(n, seed, r, 2.0) + np.asarray(offset)
    x[n // 2:n // 2 + 50] = x[:50]                                         # exact duplicates among them
    lab, n_kept, _ = R.labels(x, r, mn, mx)
    want = _scipy_labels(x, r, mn, mx)
    assert n_kept == int(want.max()) + 1 > 50 and np.array_equal(lab, want)
    assert len(set(np.bincount(R.roots(n, R.edges(x, r))).tolist())) > 6    # components of many sizes


def test_grid_image_has_the_layout_of_p2w_grid():
    g = R.solved("n_255").grid
    f = g.image[:32].view(np.float32)
    assert np.array_equal(f[0:3], np.zeros(3, dtype=np.float32)) and float(f[3]) == g.cell
    u = (R.solved("n_255").xyz - g.origin).astype(np.float32)
    assert np.array_equal(f[4:7], u.max(0)) and int(g.image[28:32].view(np.int32)[0]) == 0
    assert np.array_equal(g.image[32:56].view(np.int64), g.dims)
    assert np.array_equal(g.keys_sorted, np.sort(g.keys).astype(np.uint64)) and np.array_equal(g.xyz_sorted, R.solved("n_255").xyz[g.order])
    counts = np.bincount(g.keys, minlength=g.n_cells)
    assert np.array_equal(np.diff(g.cell_start), counts) and g.cell_start[0] == 0 and g.cell_start[-1] == len(g.keys)


# ---- every case: legal, and what the kernel's header presupposes -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_cell_is_legal_and_every_joined_pair_lies_in_adjacent_cells(name):
    s = R.solved(name)
    n = len(s.xyz)
    assert 1 <= n <= 8192 and s.xyz.dtype == np.float64 and np.isfinite(s.xyz).all()
    safe = plotgrid.safe_cell(s.r, R.extent(s.xyz))
    assert R.safe_cell(s.r, R.extent(s.xyz)) == safe
    assert s.grid.cell == (safe if s.cell is None else float(np.float32(s.cell))) and s.grid.cell >= safe
    c = s.grid.cells
    assert np.all(c >= 0) and np.all(c < s.grid.dims)
    assert np.all(np.abs(c[s.edges[:, 0]] - c[s.edges[:, 1]]).max(axis=1, initial=0) <= 1)
    assert s.n_kept == int(s.labels.max()) + 1 and s.n_noise == int((s.labels == -1).sum())


# ---- the named conditions --------------------------------------------------------------------------------------------------------------

def _d2(s, i=0, j=1):
    dx, dy, dz = s.xyz[j] - s.xyz[i]
    return (dx * dx + dy * dy) + dz * dz


def test_stencil_group_has_every_offset_position_order_and_twin():
    got = set(R.STENCIL.values())
    for o in R.OFFSETS:
        for where in ("in", "lo", "hi"):
            for rev in (False, True):
                for far in (False, True):
                    assert (o, where, rev, far, False) in got
                    assert ((o, where, rev, far, True) in got) == (sum(v != 0 for v in o) == 1)
    assert len(R.OFFSETS) == 26 and len(R.HALF) == 13 and all(tuple(-v for v in o) not in R.HALF for o in R.HALF)


@pytest.mark.parametrize("name", sorted(R.STENCIL))
def test_stencil_pair_sits_in_the_stated_cells(name):
    o, where, rev, far, safe = R.STENCIL[name]
    s = R.solved(name)
    g = s.grid
    d = 13 if safe else 7
    assert len(s.xyz) == 4 and tuple(g.dims) == (d, d, d)
    assert (s.cell is None) == safe and (safe or s.cell == 2.0 * s.r)
    c = g.cells
    assert tuple(c[1] - c[0]) == (o if (o[::-1] > (0, 0, 0)) != rev else tuple(-v for v in o))
    assert (g.keys[0] < g.keys[1]) != rev
    if where == "in":
        assert np.all(c[:2] >= 1) and np.all(c[:2] <= d - 2)
    elif where == "lo":
        assert np.all(c[:2].min(0) == 0)
    else:
        assert np.all(c[:2].max(0) == d - 1)
    assert len(set(g.keys.tolist())) == 4                                   # each point alone in its cell
    assert np.all(np.abs(c[2:, None, :] - c[None, :2, :]).max(-1) >= 2)      # the anchors: not even in a neighbouring cell
    if far:
        assert _d2(s) > s.r * s.r and len(s.edges) == 0 and s.labels.tolist() == [0, 1, 2, 3]
    else:
        assert _d2(s) <= s.r * s.r and s.edges.tolist() == [[0, 1]] and s.labels.tolist() == [0, 0, 1, 2]
    assert s.pairs == 1


def test_predicate_pairs_sit_on_the_stated_side():
    s = R.solved("pred_equal")
    assert _d2(s) == s.r * s.r and s.labels.tolist() == [0, 0]
    s = R.solved("pred_next_above")
    assert _d2(s) == math.nextafter(s.r * s.r, math.inf) and s.labels.tolist() == [0, 1]
    assert float(np.float32(s.r)) ** 2 >= _d2(s)                            # and float32(r) would join it


@pytest.mark.parametrize("name,sep_joins", [("pred_fma_sep_joins", True), ("pred_fma_fma_joins", False)])
def test_fma_pairs_flip_under_a_single_rounding_sum(name, sep_joins):
    """The origin makes the differences the coordinates themselves; r*r is exactly the lower of the two sums; the separately rounded
    sum and all three contracted ones (fma(dz, dz, dx*dx + dy*dy), and the inner sum fused either way) lie on opposite sides."""
    s = R.solved(name)
    dx, dy, dz = s.xyz[1]
    assert np.all(s.xyz[0] == 0.0) and tuple(s.xyz[1] - s.xyz[0]) == (dx, dy, dz)
    sep, outer, full_x, full_y = R.sums(float(dx), float(dy), float(dz))
    assert sep == _d2(s) and s.r * s.r == min(sep, outer) and sep != outer
    assert (sep <= s.r * s.r) == sep_joins
    assert all((v <= s.r * s.r) != sep_joins for v in (outer, full_x, full_y))
    assert s.labels.tolist() == ([0, 0] if sep_joins else [0, 1])


def test_fma_pairs_can_be_found_again():
    found = R.fma_flip_search(0, 200)
    assert set(found) == {"sep_joins", "fma_joins"}
    for kind, (dx, dy, dz, r) in found.items():
        sep, outer, full_x, full_y = R.sums(dx, dy, dz)
        assert r * r == min(sep, outer) and (sep <= r * r) == (kind == "sep_joins") and (outer <= r * r) != (sep <= r * r)


@pytest.mark.parametrize("name,f64_joins", [("pred_f64_joins_f32_not", True), ("pred_f32_joins_f64_not", False)])
def test_plot_coordinate_pairs_flip_after_rounding_to_float32(name, f64_joins):
    s = R.solved(name)
    assert np.array_equal(s.xyz[0], R.PLOT)
    x32 = s.xyz.astype(np.float32).astype(np.float64)
    dx, dy, dz = x32[1] - x32[0]
    assert (_d2(s) <= s.r * s.r) == f64_joins and ((dx * dx + dy * dy) + dz * dz <= s.r * s.r) != f64_joins
    assert s.labels.tolist() == ([0, 0] if f64_joins else [0, 1])


def test_duplicates_are_joined_at_tolerance_zero_and_nothing_else_is():
    s = R.solved("tol0_duplicates")
    assert s.r == 0.0 and len(s.edges) > 10 and np.all(s.xyz[s.edges[:, 0]] == s.xyz[s.edges[:, 1]])
    assert sorted(np.bincount(s.root)[np.unique(s.root)].tolist()) == [1, 1, 1, 2, 2, 3, 3, 4, 5, 6] and s.n_noise == 3 and s.n_kept == 7


def _sizes(s):
    return np.bincount(s.root, minlength=len(s.root))


def test_sizes_sit_exactly_at_the_bounds_and_the_filtered_take_no_number():
    s = R.solved("sizes_at_bounds")
    size = _sizes(s)
    assert np.flatnonzero(size).tolist() == list(range(10)) and size[:10].tolist() == R.SIZES_AT_BOUNDS
    assert {s.min_size - 1, s.min_size, s.max_size, s.max_size + 1} <= set(R.SIZES_AT_BOUNDS)
    assert s.labels[:10].tolist() == [-1, 0, -1, 1, -1, 2, 3, -1, 4, -1] and s.n_kept == 5
    t = R.solved("sizes_min_above_max")
    assert t.min_size > t.max_size and np.array_equal(t.xyz, s.xyz) and np.all(t.labels == -1) and t.n_kept == 0 and t.n_noise == 37


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4096, 4097, 8192])
def test_n_cases_have_n_points_kept_and_noise(n):
    s = R.solved("n_%d" % n)
    assert len(s.xyz) == n
    if n > 2:
        assert s.n_kept > 10 and s.n_noise > 10 and _sizes(s).max() > 5
        kept_roots = np.flatnonzero((s.root == np.arange(n)) & (s.labels >= 0))
        assert n < 8192 or (kept_roots.min() < 4096 < kept_roots.max())


def test_kept_roots_lie_on_both_sides_of_the_scan_tile():
    s = R.solved("n4097_kept_roots_both_sides")
    kept_roots = np.flatnonzero((s.root == np.arange(4097)) & (s.labels >= 0))
    assert len(s.xyz) == 4097 and kept_roots[0] < 4096 and kept_roots[-1] == 4096 and s.labels[4096] == s.n_kept - 1
    s = R.solved("root_above_4096")
    assert len(s.xyz) == 4600 and np.all(s.root[4500:] == 4500) and np.all(s.root[:4500] < 4500) and s.labels[4500] == s.n_kept - 1 > 0


def test_last_point_cases():
    a, b, c = R.solved("last_kept_singleton"), R.solved("last_noise_singleton"), R.solved("last_kept_member")
    n = len(a.xyz)
    assert a.root[-1] == n - 1 and _sizes(a)[-1] == 1 and a.labels[-1] == a.n_kept - 1 >= 0
    assert np.array_equal(a.xyz, b.xyz) and b.root[-1] == n - 1 and b.labels[-1] == -1 and b.n_kept > 0
    assert c.root[-1] == len(c.xyz) - 5 and c.labels[-1] == c.n_kept - 1 >= 0


@pytest.mark.parametrize("how,n", [("ascending", 2048), ("descending", 2048), ("bit_reversed", 4096), ("shuffled", 8191)])
def test_line_has_one_point_per_cell_and_the_stated_index_order(how, n):
    s = R.solved("line_" + how)
    assert len(s.xyz) == n + 1 and s.cell is None
    assert np.bincount(s.grid.keys).max() == 1
    assert np.all(s.labels[:n] == 0) and s.labels[n] == 1 and len(s.edges) == n - 1
    rank = np.argsort(np.argsort(s.xyz[:n, 0]))                              # position along the line of every index
    want = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "bit_reversed": R.bit_reversed(n) if how == "bit_reversed" else None,
            "shuffled": np.random.default_rng(43).permutation(n)}[how]
    assert np.array_equal(rank, want)
    if how == "shuffled":
        assert np.abs(np.diff(rank)).min() >= 1 and np.mean(np.abs(np.diff(rank)) > 64) > 0.9


def test_union_find_shapes():
    s = R.solved("one_cell")
    assert tuple(s.grid.dims) == (1, 1, 1) and len(s.xyz) == 1500 and np.all(s.labels == 0) and s.pairs == 1500 * 1499 // 2
    s = R.solved("comb")
    deg = np.bincount(s.edges.ravel(), minlength=len(s.xyz))
    assert np.all(s.labels == 0) and (deg == 3).sum() == 99 and (deg == 1).sum() == 101 and len(s.edges) == len(s.xyz) - 1


def test_interleaved_lines_alternate_in_every_wave_and_sit_at_the_bounds():
    s = R.solved("interleaved_lines")
    n = len(s.xyz)
    sorted_root = s.root[s.grid.order]
    assert np.array_equal(sorted_root, np.arange(n) % 2)                    # B (root 0), A (root 1), B, A, ... in the sorted order
    for w in range(0, n, 64):
        assert set(sorted_root[w:w + 64].tolist()) == {0, 1}
    size = _sizes(s)
    assert size[0] == s.max_size + 1 and size[1] == s.min_size == s.max_size
    assert np.all(s.labels[1::2] == 0) and np.all(s.labels[0::2] == -1) and (s.n_kept, s.n_noise) == (1, 1001)
    a_cells, b_cells = set(s.grid.keys[1::2].tolist()), set(s.grid.keys[0::2].tolist())
    assert a_cells <= b_cells and len(b_cells - a_cells) <= 1
    assert abs(s.xyz[0, 1] - s.xyz[1, 1]) > s.r


@pytest.mark.parametrize("name,thin", [("dims_d11", (1, 2)), ("dims_1d1", (0, 2)), ("dims_11d", (0, 1)), ("plane_xy", (2,)),
                                       ("plane_xz", (1,)), ("plane_yz", (0,)), ("dims_111", (0, 1, 2)), ("one_cell", (0, 1, 2))])
def test_grid_shapes(name, thin):
    s = R.solved(name)
    for a in range(3):
        assert (s.grid.dims[a] == 1) == (a in thin) and (a in thin or s.grid.dims[a] >= 30)
    assert s.n_kept >= 1 and len(s.edges) > 0


def test_face_wrap_case_has_no_pair_to_measure():
    s = R.solved("face_wrap")
    assert s.pairs == 0 and s.labels.tolist() == list(range(6))
    assert s.grid.cells[:4].tolist() == [[6, 1, 1], [0, 2, 1], [2, 0, 1], [2, 6, 1]] and tuple(s.grid.dims) == (7, 7, 7)


# ---- mutants: wrong kernels as variants of the reference, and the case each one changes --------------------------------------------------

def _stencil_candidates(g, offsets=R.HALF, clip=(0, 1, 2), own_twice=False):
    """The link stage as a candidate list: sorted position p -> the sorted positions it measures, i.e. the rest of its own cell and the
    cells key + ox + oy d0 + oz d0 d1 of `offsets`; an offset that leaves the grid on an axis of `clip` is skipped, on another axis
    the key arithmetic runs on into whatever row it lands in (a key outside the table: nothing)."""
    d0, d1, d2 = (int(v) for v in g.dims)
    cs = g.cell_start
    sc = g.cells[g.order]
    out = []
    for p in range(len(sc)):
        key = int(g.keys_sorted[p])
        runs = [np.arange(cs[key], cs[key + 1])] if own_twice else [np.arange(p + 1, cs[key + 1])]
        for o in offsets:
            if any(not 0 <= sc[p, a] + o[a] < g.dims[a] for a in clip):
                continue
            k = key + o[0] + o[1] * d0 + o[2] * d0 * d1
            if 0 <= k < g.n_cells:
                runs.append(np.arange(cs[k], cs[k + 1]))
        q = np.concatenate(runs)
        out.append(q[q != p])
    return out


def _stencil_answers(s, **how):
    cand = _stencil_candidates(s.grid, **how)
    xs, order = s.grid.xyz_sorted, s.grid.order
    e = []
    for p, q in enumerate(cand):
        d = xs[p] - xs[q]
        hit = q[R.joined(d[:, 0], d[:, 1], d[:, 2], s.r)]
        e.extend((int(order[p]), int(order[j])) for j in hit)
    lab, n_kept, n_noise = R.number(R.roots(len(xs), np.array(e, dtype=np.int64).reshape(-1, 2)), s.min_size, s.max_size)
    return lab, n_kept, n_noise, sum(len(q) for q in cand)


@pytest.mark.parametrize("name", ALL)
def test_half_stencil_over_the_grid_gives_the_brute_force_answers(name):
    """The kernel's plan - own cell from p + 1, 13 neighbour cells, clipped at the faces - reaches the O(n^2) labels and measures
    every pair of adjacent cells once, on every case: the unmutated form of the mutants below."""
    s = R.solved(name)
    lab, n_kept, n_noise, measured = _stencil_answers(s)
    assert np.array_equal(lab, s.labels) and (n_kept, n_noise) == (s.n_kept, s.n_noise) and measured == s.pairs


def _changed(name, pred=R.joined, coords=lambda x: x):
    s = R.solved(name)
    x = coords(s.xyz)
    lab, _, _ = R.number(R.roots(len(x), R.edges(x, s.r, pred)), s.min_size, s.max_size)
    return not np.array_equal(lab, s.labels)


def test_mutant_strict_inequality():
    assert _changed("pred_equal", lambda dx, dy, dz, r: (dx * dx + dy * dy) + dz * dz < r * r)
    assert _changed("tol0_duplicates", lambda dx, dy, dz, r: (dx * dx + dy * dy) + dz * dz < r * r)


def test_mutant_single_rounding_sum():
    def fused(dx, dy, dz, r):
        return np.vectorize(lambda a, b, c: R.sums(float(a), float(b), float(c))[1] <= r * r)(dx, dy, dz)
    assert _changed("pred_fma_sep_joins", fused) and _changed("pred_fma_fma_joins", fused)
    assert not _changed("pred_equal", fused) and not _changed("pred_next_above", fused)


def test_mutant_float32_coordinates():
    def f32(x):
        return x.astype(np.float32).astype(np.float64)
    assert _changed("pred_f64_joins_f32_not", coords=f32) and _changed("pred_f32_joins_f64_not", coords=f32)


def test_mutant_float32_tolerance():
    def pred(dx, dy, dz, r):
        return (dx * dx + dy * dy) + dz * dz <= float(np.float32(r)) ** 2
    assert _changed("pred_next_above", pred) and not _changed("pred_equal", pred)


@pytest.mark.parametrize("drop", range(13))
def test_mutant_stencil_without_one_direction(drop):
    """Dropping direction o loses the pair of every near case with offset o or -o, at every position and in both index orders, and of
    no other stencil case."""
    o = R.HALF[drop]
    rest = [h for h in R.HALF if h != o]
    for name, (oo, where, rev, far, safe) in R.STENCIL.items():
        s = R.solved(name)
        lab, n_kept, _, measured = _stencil_answers(s, offsets=rest)
        hit = oo in (o, tuple(-v for v in o))
        assert (measured != s.pairs) == hit, name
        assert (not np.array_equal(lab, s.labels)) == (hit and not far), name
        assert not (hit and not far) or lab.tolist() == [0, 1, 2, 3]


def test_mutant_no_clipping_at_a_face():
    """Without the x clamps or the y test the key arithmetic runs into the next row: labels stay (those cells are far away), the pair
    count does not.  (Without the z test the run starts beyond the table: not a wrong answer but a read out of bounds, which no
    case can show.)"""
    s = R.solved("face_wrap")
    for axis in (0, 1):
        lab, _, _, measured = _stencil_answers(s, clip=tuple(a for a in (0, 1, 2) if a != axis))
        assert np.array_equal(lab, s.labels) and measured > s.pairs == 0, axis


def test_mutant_numbering_that_counts_filtered_components():
    s = R.solved("sizes_at_bounds")
    is_root = s.root == np.arange(len(s.root))
    cid = np.cumsum(is_root) - is_root
    lab = np.where(s.labels >= 0, cid[s.root], -1)
    assert not np.array_equal(lab, s.labels) and np.array_equal(lab >= 0, s.labels >= 0)


def _wave_sizes(s, short):
    """Sizes as ec_compress_kernel counts them, wave by wave of the sorted order: the leader's root by one add of its lane count, every
    other root lane by lane - `short`: one too few per wave for those."""
    size = np.zeros(len(s.root), dtype=np.int64)
    sr = s.root[s.grid.order]
    for w in range(0, len(sr), 64):
        roots_here, counts = np.unique(sr[w:w + 64], return_counts=True)
        for x, c in zip(roots_here.tolist(), counts.tolist()):
            size[x] += c - (1 if short and x != sr[w] else 0)
    return size


@pytest.mark.parametrize("name", ["interleaved_lines", "sizes_at_bounds"])
def test_mutant_sizes_short_by_one_for_the_non_leader_roots_of_a_wave(name):
    s = R.solved(name)
    assert np.array_equal(_wave_sizes(s, False), _sizes(s))
    size = _wave_sizes(s, True)
    kept = (size[s.root] >= s.min_size) & (size[s.root] <= s.max_size)
    assert not np.array_equal(kept, s.labels >= 0)


def test_mutant_count_that_ignores_a_kept_last_root():
    for name, differs in (("last_kept_singleton", True), ("n4097_kept_roots_both_sides", True), ("n_1", True),
                          ("last_noise_singleton", False), ("last_kept_member", False)):
        s = R.solved(name)
        n = len(s.root)
        kept_root = (s.root == np.arange(n)) & (s.labels >= 0)
        cid_last = int(kept_root[:n - 1].sum())                             # the exclusive scan at the last point
        assert (cid_last != s.n_kept) == differs, name


def test_mutant_pair_count_that_visits_own_cell_pairs_twice():
    for name in ("one_cell", "dims_111", "pred_equal", "interleaved_lines"):
        s = R.solved(name)
        lab, _, _, measured = _stencil_answers(s, own_twice=True)
        assert np.array_equal(lab, s.labels) and measured > s.pairs, name
    s = R.solved("line_ascending")                                          # one point per cell: this one cannot tell
    assert _stencil_answers(s, own_twice=True)[3] == s.pairs
