"""The four entry points of csrc/p2w_pathlen.hip on the MI355X, each alone, against the plain reference tests/pathlen_ref.py (pinned
to the recorded fixtures by tests/test_pathlen_ref_cpu.py, which also asserts that every case below meets the condition it is
named for).  Every stage is fed the REFERENCE's output of the stage before it, and every comparison is exact: integers equal,
float64 by bit pattern."""
import ctypes

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from pointstowood_amd import pathlength as PL
from tests import pathlen_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


# ---- kNN -------------------------------------------------------------------------------------------------------------------------------

def _three_of_each():
    return R.duplicated(150, 3)


KNN = {
    "coincident_k10": (lambda: R.coincident(50), 10),
    "collinear_k4": (R.collinear, 4),
    "collinear_k65": (R.collinear, 65),
    "planar_k16": (R.planar, 16),
    "lattice_k20": (R.lattice, 20),
    "lattice_offset_k20": (lambda: R.lattice(offset=R.LATTICE_OFFSET), 20),
    "duplicated_k12": (_three_of_each, 12),
    "n_equals_k_100": (lambda: R.uniform(100, 27), 100),
    "two_k1": (lambda: np.array([[0.0, 0.0, 0.0], [0.1, 0.2, 0.3]]), 1),
    "two_k2": (lambda: np.array([[0.0, 0.0, 0.0], [0.1, 0.2, 0.3]]), 2),
    "one_point": (lambda: np.array([[1.5, -2.25, 3.0]]), 1),
}


@pytest.mark.parametrize("name", sorted(KNN))
def test_knn_rows_equal_the_brute_force_rows(name):
    """collinear_k65 caught the ring walk of pl_knn_kernel: its rows were right, but the grid of a line is one cell thick and every
    ring stepped through the (2 s + 1)^2 rows outside it - 11.6 s for these 400 points before the offsets were clipped to the grid."""
    make, k = KNN[name]
    x = make()
    got = PL.knn_rows(_dev(x), k).cpu().numpy()
    assert got.shape == (len(x), k) and got.dtype == np.int32
    assert np.array_equal(got, R.knn_rows(x, k))


# ---- growth ----------------------------------------------------------------------------------------------------------------------------

GROWTH = sorted(R.growth_cases())


def kernel_stop(g):
    """info_out[1] as include/p2w.h states it, from the reference's run: the last step with a non-empty frontier or a threshold
    raise.  The reference's loop ends right after the step that processed the last point; the kernel still runs the frontier step
    after it (every row entry is processed, nothing is added) and stops at the empty frontier behind that, so it reports
    max(step) + 1 - the reference's stop step + 1, and the same step for one point, whose only (empty-handed) step both take.
    Where points stay unreached the reference's stop step is the one that found so, which the kernel does not count: one less."""
    if g.unreached:
        return g.stop - 1
    return int(g.step.max()) + 1


def _grow(name):
    (x, k, base, kp, thr, stp, gthr), rows, g = R.grown(name)
    step, edges, info = PL._grow(_dev(x), _dev(rows, torch.int32), base, kp, thr, stp, gthr)
    return g, step.cpu().numpy(), edges.cpu().numpy().astype(np.int64), info


@pytest.mark.parametrize("name", GROWTH)
def test_growth_equals_the_reference_loop(name):
    """Steps, the raw ordered edge list (duplicates and self-loops as emitted), gap steps, raises, the unreached flag, the bits
    of the repeatedly raised threshold, the edge count and the stop step."""
    g, step, edges, info = _grow(name)
    assert step.dtype == np.int32 and np.array_equal(step, g.step)
    assert edges.shape == g.edges.shape and np.array_equal(R.sort_pairs(edges), R.sort_pairs(g.edges))
    assert (info["gap_steps"], info["threshold_raises"], info["stopped_unreached"]) == (g.gap_steps, g.raises, g.unreached)
    assert np.array_equal(_bits([info["final_threshold"]]), _bits([g.threshold]))
    assert info["edges"] == len(g.edges)
    assert info["stop_step"] == kernel_stop(g)
    n = len(step)
    if not g.unreached:
        assert info["stop_step"] == g.stop + (1 if n > 1 else 0)


def test_unreached_island_leaves_the_main_blob_as_grown_alone():
    (x, k, base, kp, thr, stp, gthr), rows, g = R.grown("unreached")
    alone = R.grow(x[:120], rows[:120], base, kp, thr, stp, gthr)
    _, step, edges, info = _grow("unreached")
    assert info["stopped_unreached"] and np.all(step[120:] == -1)
    assert np.array_equal(step[:120], alone.step) and np.array_equal(R.sort_pairs(edges), R.sort_pairs(alone.edges))


def test_growth_twice_gives_the_same_steps_and_edges():
    a, b = _grow("duplicated"), _grow("duplicated")
    assert np.array_equal(a[1], b[1]) and np.array_equal(R.sort_pairs(a[2]), R.sort_pairs(b[2]))
    assert {k: v for k, v in a[3].items() if k != "grow_launches"} == {k: v for k, v in b[3].items() if k != "grow_launches"}


def _grow_direct(x, rows, base, kp, thr, stp, gthr, cap, tail):
    """p2w_pathlen_grow with an edge buffer of `cap` pairs and `tail` int32 words of canary directly behind it."""
    L = _lib.lib()
    xd, nd = _dev(x), _dev(rows, torch.int32)
    n, k = rows.shape
    buf = torch.full((2 * cap + tail,), -7, dtype=torch.int32, device="cuda")
    step = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.p2w_pathlen_grow_ws_bytes(n)), dtype=torch.uint8, device="cuda")
    info = (ctypes.c_int64 * 6)(*([-1] * 6))
    out = ctypes.c_double(-1.0)
    code = L.p2w_pathlen_grow(xd.data_ptr(), nd.data_ptr(), n, k, base, kp, thr, stp, gthr, step.data_ptr(), buf.data_ptr(), cap,
                              ctypes.addressof(info), ctypes.addressof(out), ws.data_ptr(), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    return code, buf.cpu().numpy(), step.cpu().numpy(), list(info), out.value


def test_edge_buffer_of_exactly_the_edge_count_is_enough_and_one_less_is_refused_without_a_stray_store():
    (x, k, base, kp, thr, stp, gthr), rows, g = R.grown("island_0.3")
    m = len(g.edges)
    code, buf, step, info, out = _grow_direct(x, rows, base, kp, thr, stp, gthr, m, 64)
    assert code == 0 and info[0] == m and np.all(buf[2 * m:] == -7)
    assert np.array_equal(R.sort_pairs(buf[:2 * m].reshape(-1, 2)), R.sort_pairs(g.edges)) and np.array_equal(step, g.step)
    code, buf, step, info, out = _grow_direct(x, rows, base, kp, thr, stp, gthr, m - 1, 64)
    assert code == -4                                                      # P2W_EWORKSPACE
    assert np.all(buf[2 * (m - 1):] == -7)
    kept = buf[:2 * (m - 1)].reshape(-1, 2)
    kept = kept[kept[:, 0] != -7]
    want = {tuple(p) for p in g.edges.tolist()}
    assert len(kept) == m - 1 and all(tuple(p) in want for p in kept.tolist())


# ---- SSSP ------------------------------------------------------------------------------------------------------------------------------

def _graphs():
    out = {}
    for name in R.growth_cases():
        (x, _, base, *_), _, g = R.grown(name)
        out["grow_" + name] = (x, g.edges, base)
    out.update(R.sssp_cases())
    return out


GRAPHS = sorted(_graphs())
_solved = {}


def _solve(name):
    if name not in _solved:
        x, e, base = _graphs()[name]
        n = len(x)
        w = R.dist(x, e[:, 0], e[:, 1]) if len(e) else np.zeros(0)
        d = R.dijkstra(n, e, w, base)
        _solved[name] = (x, e, base, d, R.parents(n, e, w, d, base), R.hops(n, e, w, d, base)[0])
    return _solved[name]


def _sssp(x, e, base):
    dist, parent, info = PL._sssp(_dev(x), _dev(np.asarray(e, dtype=np.int64).reshape(-1, 2), torch.int32), base, parents=True)
    return dist.cpu().numpy(), parent.cpu().numpy(), info


def _assert_sssp(got, d, par, hop, n):
    """info_out: the round count depends on which relaxations win the race, so only 1 <= rounds <= n is asserted; the hop levels
    are those of the level-synchronous search over tight edges: the first level with an empty frontier, 1 + the reference's largest
    hop count."""
    dist, parent, info = got
    assert np.array_equal(np.isnan(dist), np.isnan(d))
    assert np.array_equal(_bits(dist), _bits(np.where(np.isnan(d), dist, d)))
    assert np.array_equal(parent.astype(np.int64), par)
    assert 1 <= info["sssp_rounds"] <= n
    assert info["hop_levels"] == int(hop.max()) + 1


@pytest.mark.parametrize("name", GRAPHS)
def test_sssp_distances_and_parents_equal_dijkstra_and_the_parent_rule(name):
    """The raw list (duplicates, both orientations and self-loops left in) and the de-duplicated (min, max) list give the same bits."""
    x, e, base, d, par, hop = _solve(name)
    n = len(x)
    _assert_sssp(_sssp(x, e, base), d, par, hop, n)
    _assert_sssp(_sssp(x, R.graph(x, e)[0], base), d, par, hop, n)


@pytest.mark.parametrize("name", ["lattice_graph", "multigraph", "zero_cluster", "grow_duplicated", "grow_lattice_kp3"])
def test_sssp_does_not_depend_on_edge_order_or_orientation(name):
    x, e, base, d, par, hop = _solve(name)
    _assert_sssp(_sssp(x, R.flipped(e), base), d, par, hop, len(x))


def test_sssp_without_edges_and_with_an_isolated_base():
    for name in ("no_edges", "isolated_base"):
        x, e, base, d, par, hop = _solve(name)
        dist, parent, info = _sssp(x, e, base)
        assert dist[base] == 0.0 and np.all(np.isnan(np.delete(dist, base))) and np.all(parent == -1)
        assert info["sssp_rounds"] == 1 and info["hop_levels"] == 1


def test_sssp_grid_stride_loops_on_600000_nodes():
    """More nodes and more edges than the 2048 x 256 threads of a launch; distances against the numpy Bellman-Ford."""
    x, e, base = R.big_shallow()
    n = len(x)
    d = R.bellman_ford_np(n, e, R.dist(x, e[:, 0], e[:, 1]), base)
    dist, _, info = PL._sssp(_dev(x), _dev(e, torch.int32), base, parents=False)
    dist = dist.cpu().numpy()
    assert np.array_equal(np.isnan(dist), np.isnan(d)) and np.array_equal(_bits(dist[~np.isnan(d)]), _bits(d[~np.isnan(d)]))
    assert 1 <= info["sssp_rounds"] <= n and info["hop_levels"] == 0


# ---- weights ---------------------------------------------------------------------------------------------------------------------------

def test_weights_of_600000_int64_pairs_equal_dist():
    g = np.random.default_rng(28)
    x = g.uniform(-50, 50, (5000, 3))
    e = g.integers(0, 5000, (600_000, 2))
    e[::1000, 1] = e[::1000, 0]                                            # self-loops
    xd, ed = _dev(x), _dev(e)
    w = torch.full((len(e) + 8,), -1.0, dtype=torch.float64, device="cuda")
    L = _lib.lib()
    assert L.p2w_pathlen_weights(xd.data_ptr(), ed.data_ptr(), len(e), w.data_ptr(), _lib.stream()) == 0
    w = w.cpu().numpy()
    assert np.array_equal(_bits(w[:len(e)]), _bits(R.dist(x, e[:, 0], e[:, 1]))) and np.all(w[len(e):] == -1.0)
    assert np.all(w[:len(e):1000] == 0.0)
    assert L.p2w_pathlen_weights(xd.data_ptr(), None, 0, None, _lib.stream()) == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

def test_path_graph_and_paths_on_duplicate_points():
    """PathGraph from the raw reference edges of the duplicate-point case (zero weights, self-loops, ties), and the paths of
    extract_path_info: the check of test_parent_chains_are_shortest_acyclic_and_end_at_the_base on data with equal distances."""
    (x, k, base, *_), rows, g = R.grown("duplicated")
    G = PL.PathGraph(_dev(x), _dev(g.edges, torch.int32), _dev(g.step))
    ue, uw = R.graph(x, g.edges)
    assert G.edges.dtype == np.int64 and np.array_equal(G.edges, ue) and np.array_equal(_bits(G.weights), _bits(uw))
    assert np.array_equal(np.where(np.isnan(G.step_register), -1, G.step_register).astype(np.int32), g.step)
    ids, dist, paths = PL.extract_path_info(G, base, return_path=True)
    d = R.dijkstra(len(x), ue, uw, base)
    reached = np.flatnonzero(~np.isnan(d))
    want = reached[np.lexsort((reached, d[reached]))]
    assert ids == want.tolist() and np.array_equal(_bits(dist), _bits(d[want]))
    assert len(set(dist)) < len(dist)                                      # equal distances: the index decides the order
    w = {(int(a), int(b)): float(ww) for (a, b), ww in zip(ue, uw)}
    dd = dict(zip(ids, dist))
    assert set(paths) == set(ids)
    for v in ids:
        p = paths[v]
        assert p[0] == base and p[-1] == v and len(set(p)) == len(p)
        acc = 0.0
        for a, b in zip(p[:-1], p[1:]):
            acc = acc + w[(min(a, b), max(a, b))]
            assert acc == dd[b]
