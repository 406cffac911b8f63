"""tests/pathlen_ref.py without a GPU: the plain reference reproduces the seven fixtures recorded from the reference project
(tests/golden/pathlength), its parts agree with one another, and every generated case of tests/test_gpu_pathlen_kernels.py meets
the condition it is there for - so no GPU test can pass by being vacuous."""
import os

import numpy as np
import pytest

from tests import pathlen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pathlength")
CASES = ["tree_defaults", "tree_gaps", "tree_k16", "tree_graph_threshold", "tree_easting", "single_point", "knn_equals_n"]
# sklearn measured knn_equals_n by its dot-product expansion (tests/test_gpu_pathlength.py): lengths to 1e-12 there, bits elsewhere
APPROX = {"knn_equals_n"}


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, name):
    if name in APPROX:
        return np.allclose(got, want, rtol=1e-12, atol=1e-15)
    return np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", CASES)
def test_reference_reproduces_the_recorded_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    x, base = z["xyz"], int(z["base_id"])
    rows = R.knn_rows(x, int(z["knn"]))
    g = R.grow(x, rows, base, int(z["kpairs"]), float(z["nbrs_threshold"]), float(z["nbrs_threshold_step"]), float(z["graph_threshold"]))
    assert np.array_equal(g.step, z["step"])
    e, w = R.graph(x, g.edges)
    assert np.array_equal(e, z["edges"].astype(np.int64))
    assert _same(w, z["weights"], name)
    if name == "single_point":
        assert len(e) == 0 and int(z["no_source"]) == 1 and g.stop == 1 and not g.unreached
        return
    d = R.dijkstra(len(x), e, w, base)
    ids = np.flatnonzero(~np.isnan(d))
    assert np.array_equal(ids, z["node_ids"])
    assert _same(d[ids], z["distance"], name)
    assert not g.unreached and g.stop == int(g.step.max())


def _sssp_inputs():
    """name -> (n, edges, weights, base) of every small SSSP case: the growth cases' raw edge lists and the hand-built graphs."""
    out = {}
    for name in R.growth_cases():
        (x, _, base, *_), _, g = R.grown(name)
        out["grow_" + name] = (x, g.edges, base)
    out.update(R.sssp_cases())
    return out


SSSP = sorted(_sssp_inputs())


@pytest.fixture(scope="module")
def solved():
    res = {}
    for name, (x, e, base) in _sssp_inputs().items():
        n = len(x)
        w = R.dist(x, e[:, 0], e[:, 1]) if len(e) else np.zeros(0)
        d = R.dijkstra(n, e, w, base)
        res[name] = (n, e, w, base, d, R.parents(n, e, w, d, base), R.hops(n, e, w, d, base)[0])
    return res


@pytest.mark.parametrize("name", SSSP)
def test_bellman_ford_bit_equals_dijkstra_and_ignores_duplicates(name, solved):
    n, e, w, base, d, _, _ = solved[name]
    assert np.array_equal(_bits(R.bellman_ford_np(n, e, w, base)), _bits(d))
    x = _sssp_inputs()[name][0]
    ue, uw = R.graph(x, e)
    assert np.array_equal(_bits(R.dijkstra(n, ue, uw, base)), _bits(d))
    assert d[base] == 0.0


@pytest.mark.parametrize("name", SSSP)
def test_parent_chains_fall_one_hop_per_step_and_sum_to_the_distance(name, solved):
    n, e, w, base, d, par, hop = solved[name]
    wmin = {}
    for (a, b), ww in zip(e.tolist(), w.tolist()):
        wmin.setdefault((a, b), set()).add(ww)
        wmin.setdefault((b, a), set()).add(ww)
    reached = ~np.isnan(d)
    assert np.array_equal(hop >= 0, reached)
    assert par[base] == -1 and np.all(par[~reached] == -1) and np.all(par[reached & (np.arange(n) != base)] >= 0)
    for v in np.flatnonzero(reached).tolist():
        path = [v]
        while path[-1] != base:
            u = int(par[path[-1]])
            assert hop[u] == hop[path[-1]] - 1
            path.append(u)
        assert len(path) == hop[v] + 1
        acc = 0.0
        for a, b in zip(path[::-1][:-1], path[::-1][1:]):                 # from the base outwards: the left-fold sum
            (ww,) = wmin[(a, b)]
            acc = acc + ww
            assert acc == d[b]


# ---- the cases exercise what they claim ----------------------------------------------------------------------------------------------

def test_long_chains_cross_every_read_back_batch():
    assert R.grown("chain_k4_kp1")[2].stop > 4 + 8 + 16 + 32 + 64 + 64
    assert R.grown("chain_k4_kp0")[2].stop > 4 + 8 + 16 + 32 + 64 + 64
    assert R.grown("chain_k8_kp3_mid")[2].stop > 4 + 8 + 16
    for name in ("chain_k4_kp1", "chain_k4_kp0", "chain_k8_kp3_mid"):
        g = R.grown(name)[2]
        assert not g.unreached and np.all(g.step >= 0)


def test_island_cases_cover_the_raise_counts():
    """The threshold raises before the island's gap step move the step counter, and with it the counter rotation, by 0, 1, 2, ..."""
    raises = []
    for off in R.ISLAND_OFFSETS:
        g = R.grown(f"island_{off}")[2]
        assert not g.unreached and np.all(g.step >= 0) and g.gap_steps >= 1
        thr = 0.15
        for _ in range(g.raises):
            thr = thr + 0.05
        assert thr == g.threshold
        raises.append(g.raises)
    assert 0 in raises and {r % 3 for r in raises} == {0, 1, 2} and max(raises) >= 15


def test_duplicate_point_case_has_zero_weights_self_loops_and_a_gap_step():
    (x, *_), rows, g = R.grown("duplicated")
    w = R.dist(x, g.edges[:, 0], g.edges[:, 1])
    loops = g.edges[:, 0] == g.edges[:, 1]
    assert np.any(loops) and np.any((w == 0.0) & ~loops) and g.gap_steps >= 1
    assert len(R.sort_pairs(g.edges)) > len(R.graph(x, g.edges)[0])      # the raw list holds duplicates


def test_unreached_case_leaves_the_island_and_the_blob_is_grown_as_if_alone():
    (x, k, base, kp, thr, stp, gthr), rows, g = R.grown("unreached")
    assert g.unreached and np.all(g.step[120:] == -1) and np.all(g.step[:120] >= 0)
    assert rows[:120].max() < 120 and rows[120:].min() >= 120
    alone = R.grow(x[:120], rows[:120], base, kp, thr, stp, gthr)
    assert not alone.unreached
    assert np.array_equal(alone.step, g.step[:120]) and np.array_equal(R.sort_pairs(alone.edges), R.sort_pairs(g.edges))
    assert g.stop == alone.stop + 2           # one frontier step that finds nothing new, then the step that finds no row to join


def test_graph_threshold_cases():
    full = R.grown("gthr_0.05")[2]
    assert 0 < len(full.edges)
    (x, k, base, kp, thr, stp, _), rows, _ = R.grown("gthr_0")
    wide = R.grow(x, rows, base, kp, thr, stp, np.inf)
    assert len(full.edges) < len(wide.edges) and np.array_equal(full.step, wide.step)
    for name in ("gthr_0", "gthr_neg"):
        g = R.grown(name)[2]
        assert len(g.edges) == 0 and np.all(g.step >= 0) and np.array_equal(g.step, wide.step)


def test_lattice_rows_are_decided_by_the_index_rule():
    for x in (R.lattice(), R.lattice(offset=R.LATTICE_OFFSET)):
        every = np.arange(len(x))
        d = np.sort(R.dist(x, every[:, None], every[None, :]), axis=1)
        assert np.sum(d[:, 19] == d[:, 20]) >= 125                        # k = 20: the k-th and the (k + 1)-th are equally far in
        #                                                                   every interior row (1 + 6 + 12 nearer, 8 at pitch * sqrt(3))
    a, b = R.lattice(), R.lattice(offset=R.LATTICE_OFFSET)
    assert np.array_equal(b - np.asarray(R.LATTICE_OFFSET), a)            # the offset coordinates are exact
    assert np.array_equal(R.knn_rows(a, 20), R.knn_rows(b, 20))
    g = R.grown("lattice_kp30")[2]
    assert not g.unreached and np.all(g.step >= 0)


def test_small_and_degenerate_growth_cases():
    g = R.grown("two_k1")[2]
    assert g.unreached and g.step.tolist() == [0, -1] and g.stop == 2
    g = R.grown("one_point")[2]
    assert not g.unreached and g.step.tolist() == [0] and g.stop == 1 and len(g.edges) == 0      # the loop runs its one step
    g = R.grown("two_k2")[2]
    assert not g.unreached and g.step.tolist() == [0, 1] and g.stop == 1 and g.edges.tolist() == [[0, 1]]
    g = R.grown("coincident")[2]
    assert np.all(g.step >= 0) and g.gap_steps >= 1
    g = R.grown("threshold_tie")[2]
    assert g.step[8] == 9 and g.step[9] == 12 and g.raises == 1 and g.gap_steps == 2 and g.threshold == 0.25 + 0.05
    g = R.grown("saturating")[2]
    assert g.unreached and g.raises == 2 and g.threshold == 2.0 ** 53 and g.stop == 5 and g.step.tolist() == [0, 1, -1, -1]


def test_sssp_tie_graphs_have_several_candidate_parents(solved):
    for name, least in (("lattice_graph", 100), ("zero_cluster", 10), ("grow_lattice_kp3", 50), ("grow_duplicated", 20)):
        n, e, w, base, d, par, hop = solved[name]
        cand = [set() for _ in range(n)]
        for (a, b), ww in zip(e.tolist(), w.tolist()):
            for u, v in ((a, b), (b, a)):
                if hop[u] >= 0 and hop[v] == hop[u] + 1 and d[u] + ww == d[v]:
                    cand[v].add(u)
        many = [v for v in range(n) if len(cand[v]) >= 2]
        assert len(many) >= least, (name, len(many))
        assert all(par[v] == min(cand[v]) for v in many)
        # and the smallest index is not simply the first or the last neighbour in edge-list order for all of them
        assert any(par[v] != max(cand[v]) for v in many)


def test_sssp_case_shapes():
    x, e, base = R.multigraph()
    assert len(x) == 2000 and len(e) == 7000 and int(np.sum(e[:, 0] == e[:, 1])) >= 200
    d = R.dijkstra(len(x), e, R.dist(x, e[:, 0], e[:, 1]), base)
    assert 2 <= int(np.sum(~np.isnan(d))) <= 100                          # the base's component is the smallest
    x, e, base = R.star()
    assert np.bincount(e.ravel())[0] == len(x) - 1 == 4095
    x, e, base = R.shuffled_path()
    assert int(np.nanargmax(R.dijkstra(300, e, R.dist(x, e[:, 0], e[:, 1]), base))) == 299
    x, e, base = R.isolated_base()
    assert base not in e
    x, e, base = R.zero_cluster()
    w = R.dist(x, e[:, 0], e[:, 1])
    assert int(np.sum(w == 0.0)) == 20 * 19 // 2


def test_big_shallow_graph_needs_few_rounds():
    x, e, base = R.big_shallow()
    assert len(x) > 2048 * 256 and len(e) > 2048 * 256
    rounds = []
    d = R.bellman_ford_np(len(x), e, R.dist(x, e[:, 0], e[:, 1]), base, rounds)
    assert rounds[0] < 64 and np.sum(~np.isnan(d)) > len(x) // 2
