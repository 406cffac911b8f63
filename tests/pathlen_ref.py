"""A plain reference of the path-length stages of ``csrc/p2w_pathlen.hip``: numpy and the standard library only, written from the
comments of ``include/p2w.h`` and from nothing of the package under test.

    dist / knn_rows      sqrt((dx*dx + dy*dy) + dz*dz) in float64, brute-force rows ascending by (distance, index)
    grow                 the growth loop of p2w_pathlen_grow's header comment, one Python step per step
    graph                the (min, max) de-duplication of pathlength.PathGraph and its weights
    dijkstra             heapq; bellman_ford_np: the same fixed point by np.minimum.at (for the one large case)
    parents              hop counts over tight edges, then the smallest-index tight neighbour one hop nearer
    case generators      seeded float64 clouds and edge lists of tests/test_gpu_pathlen_kernels.py

``tests/test_pathlen_ref_cpu.py`` pins it to the seven fixtures recorded from the reference project (tests/golden/pathlength) and
asserts that every generated case exercises what it is named for."""
from __future__ import annotations

import heapq
from collections import namedtuple

import numpy as np


def dist(x, a, b):
    """Float64 distance of the points a and b of x (indices or index arrays), every operation rounded on its own."""
    x = np.asarray(x, dtype=np.float64)
    a, b = np.asarray(a), np.asarray(b)
    dx = x[a, 0] - x[b, 0]
    dy = x[a, 1] - x[b, 1]
    dz = x[a, 2] - x[b, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def knn_rows(x, k):
    """[n, k] int64: row i = the k nearest points of i (itself included), ascending by (dist, index), by brute force."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    rows = np.empty((n, k), dtype=np.int64)
    every = np.arange(n)
    for s in range(0, n, 512):
        q = np.arange(s, min(s + 512, n))
        d = dist(x, q[:, None], every[None, :])
        rows[q] = np.argsort(d, axis=1, kind="stable")[:, :k]        # stable: equal distances stay in index order
    return rows


Growth = namedtuple("Growth", "step edges gap_steps raises threshold unreached stop")


def grow(x, nbr, base, kpairs, thr, step, gthr):
    """The growth loop.  Returns Growth(step [n] int32 (-1 never), edges [E, 2] int64 = the ordered pairs (g, e) as emitted, duplicates
    and self-loops included, gap steps, threshold raises, final threshold, unreached flag, stop step).

    Step t = 1, 2, ...; "processed" inside step t means 0 <= step < t.
      frontier step  every frontier node g takes the first min(kpairs + 1, k) entries e of its row that are not processed, adds the
                     edge (g, e) where dist <= gthr and claims every taken entry that has no step yet; the claimed form the next
                     frontier.
      empty frontier the remaining points whose FIRST processed row entry lies at dist < thr each take the first kp1 processed and
                     the first kp1 unprocessed entries of their row (a gap step; they form the next frontier).  If there is none,
                     thr += step and the step is spent.
    The loop ends after the step that processed the last point (it runs at least once: ``stop`` = that step).  Where no remaining row
    holds a processed point, or the addition leaves thr unchanged, it ends with ``unreached`` set, ``stop`` = the step that found so."""
    x = np.asarray(x, dtype=np.float64)
    nbr = np.asarray(nbr)
    n, k = nbr.shape
    kp1 = min(kpairs + 1, k)
    thr, step, gthr = float(thr), float(step), float(gthr)
    rows = nbr.tolist()
    D = dist(x, np.arange(n)[:, None], nbr).tolist()
    st = [-1] * n
    st[base] = 0
    left = n - 1
    edges = []
    frontier = [base]
    t = gaps = raises = 0
    unreached = False
    while True:
        t += 1
        if frontier:
            claimed = []
            for g in frontier:
                row, drow, taken = rows[g], D[g], 0
                for j in range(k):
                    if taken == kp1:
                        break
                    e = row[j]
                    s = st[e]
                    if 0 <= s < t:
                        continue
                    taken += 1
                    if drow[j] <= gthr:
                        edges.append((g, e))
                    if s == -1:
                        st[e] = t
                        claimed.append(e)
            frontier = claimed
        else:
            found, holds = [], False
            for i in range(n):
                if st[i] != -1:
                    continue
                for j in range(k):
                    if st[rows[i][j]] >= 0:
                        holds = True
                        if D[i][j] < thr:
                            found.append(i)
                        break
            if not holds:
                unreached = True
                break
            if not found:
                nt = thr + step
                if nt == thr:
                    unreached = True
                    break
                thr = nt
                raises += 1
                continue
            for i in found:
                row, drow = rows[i], D[i]
                for side in (True, False):
                    taken = 0
                    for j in range(k):
                        if taken == kp1:
                            break
                        if (0 <= st[row[j]] < t) != side:
                            continue
                        taken += 1
                        if drow[j] <= gthr:
                            edges.append((i, row[j]))
            for i in found:                      # after every row was read: a point found in this step is unprocessed during it
                st[i] = t
            frontier = found
            gaps += 1
        left -= len(frontier)
        if left == 0:
            break
    return Growth(np.asarray(st, dtype=np.int32), np.asarray(edges, dtype=np.int64).reshape(-1, 2), gaps, raises, thr, unreached, t)


def sort_pairs(e):
    """The rows of an [E, 2] edge list in ascending (first, second) order, duplicates kept."""
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def graph(x, edges):
    """(edges [E, 2] int64 = the unique (min, max) pairs in ascending order, weights [E] float64)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    n = len(x)
    code = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))
    u = np.stack([code // n, code % n], 1)
    return u, dist(x, u[:, 0], u[:, 1])


def dijkstra(n, edges, w, base):
    """dist [n] float64 from base over the undirected edges (self-loops ignored, duplicates allowed), NaN where unreached."""
    adj = [[] for _ in range(n)]
    for (a, b), ww in zip(np.asarray(edges).reshape(-1, 2).tolist(), np.asarray(w, dtype=np.float64).tolist()):
        if a != b:
            adj[a].append((b, ww))
            adj[b].append((a, ww))
    d = [float("inf")] * n
    d[base] = 0.0
    done = [False] * n
    heap = [(0.0, base)]
    while heap:
        du, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v, ww in adj[u]:
            nd = du + ww
            if nd < d[v]:
                d[v] = nd
                heapq.heappush(heap, (nd, v))
    out = np.asarray(d, dtype=np.float64)
    out[np.isinf(out)] = np.nan
    return out


def bellman_ford_np(n, edges, w, base, rounds_out=None):
    """The same distances as the fixed point of d[v] = min(d[v], d[u] + w) over both directions of every edge."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64)
    d = np.full(n, np.inf)
    d[base] = 0.0
    rounds = 0
    while True:
        nd = d.copy()
        np.minimum.at(nd, e[:, 1], d[e[:, 0]] + w)
        np.minimum.at(nd, e[:, 0], d[e[:, 1]] + w)
        rounds += 1
        if np.array_equal(nd, d):
            break
        d = nd
    if rounds_out is not None:
        rounds_out.append(rounds)
    d[np.isinf(d)] = np.nan
    return d


def hops(n, edges, w, d, base):
    """hop [n] int64: breadth-first level from base over the tight edges u -> v (d[u] + w == d[v], bitwise), -1 where unreached."""
    adj = [[] for _ in range(n)]
    dl = np.asarray(d, dtype=np.float64).tolist()
    for (a, b), ww in zip(np.asarray(edges).reshape(-1, 2).tolist(), np.asarray(w, dtype=np.float64).tolist()):
        if dl[a] + ww == dl[b]:              # NaN (unreached) compares unequal
            adj[a].append(b)
        if dl[b] + ww == dl[a]:
            adj[b].append(a)
    hop = [-1] * n
    hop[base] = 0
    level = [base]
    while level:
        nxt = []
        for u in level:
            for v in adj[u]:
                if hop[v] == -1:
                    hop[v] = hop[u] + 1
                    nxt.append(v)
        level = nxt
    return np.asarray(hop, dtype=np.int64), adj


def parents(n, edges, w, d, base):
    """parent [n] int64: for every reached v != base the smallest-index tight neighbour u with hop[u] == hop[v] - 1; -1 for the base
    and for unreached nodes."""
    hop, adj = hops(n, edges, w, d, base)
    par = [-1] * n
    for u in range(n):                        # u ascending: the first one written is the smallest
        if hop[u] < 0:
            continue
        for v in adj[u]:
            if v != base and hop[v] == hop[u] + 1 and par[v] == -1:
                par[v] = u
    return np.asarray(par, dtype=np.int64)


# ---- case generators (seeded, float64) -----------------------------------------------------------------------------------------------

def coincident(n=50):
    return np.tile(np.array([[0.3, -1.25, 2.0]]), (n, 1))


def collinear(n=400, seed=11):
    """n points along z, about 1 cm apart with 1 mm jitter, x = y = 0 exactly."""
    g = np.random.default_rng(seed)
    x = np.zeros((n, 3))
    x[:, 2] = np.arange(n) * 0.01 + g.normal(0, 0.001, n)
    return x[g.permutation(n)]


def planar(n=1500, seed=12):
    g = np.random.default_rng(seed)
    x = g.uniform(0, 2, (n, 3))
    x[:, 2] = 0.75
    return x


def lattice(m=7, pitch=0.125, offset=(0.0, 0.0, 0.0), seed=13):
    """An m x m x m lattice in shuffled order; pitch and offset are chosen so that every coordinate is exact in float64."""
    g = np.random.default_rng(seed)
    i = np.arange(m, dtype=np.float64) * pitch
    x = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    x = x[g.permutation(len(x))] + np.asarray(offset, dtype=np.float64)
    return x


LATTICE_OFFSET = (5.0e5, 1.0e6, 0.0)


def duplicated(m=150, times=3, seed=14):
    """m points of a 0.6 m cube, each repeated `times` times, shuffled."""
    g = np.random.default_rng(seed)
    x = np.repeat(g.uniform(0, 0.6, (m, 3)), times, axis=0)
    return x[g.permutation(len(x))]


def uniform(n, seed, box=1.0):
    return np.random.default_rng(seed).uniform(0, box, (n, 3))


def chain(n=400, seed=15):
    """n points along x about 5 cm apart (2 mm jitter on every axis), in order: index i is the i-th point of the chain."""
    g = np.random.default_rng(seed)
    x = g.normal(0, 0.002, (n, 3))
    x[:, 0] += np.arange(n) * 0.05
    return x


def blob_island(offset, island=12, main=120, seed=16):
    """A blob of `main` points (sigma 5 cm) and an island of `island` points (sigma 1 cm) `offset` metres along x.  The base is the
    point of least z of the blob (index < main)."""
    g = np.random.default_rng(seed)
    a = g.normal(0, 0.05, (main, 3))
    b = g.normal(0, 0.01, (island, 3)) + np.array([offset, 0.0, 0.0])
    return np.concatenate([a, b])


ISLAND_OFFSETS = (0.25, 0.3, 0.45, 0.5, 0.55, 1.2)          # 0, 1, 4, 5, 6 and 19 threshold raises


def threshold_tie():
    """A chain of 8 points of pitch 0.125 along z and two side points, one 0.125 and one exactly 0.25 beside it, in exact
    coordinates: with nbrs_threshold = 0.25 the first joins at the first gap step and the second (0.25 < 0.25 is false) only after
    a raise.  Returns (xyz, k, kpairs, nbrs_threshold)."""
    x = np.zeros((10, 3))
    x[:8, 2] = np.arange(8) * 0.125
    x[8] = (0.125, 0.0, 0.25)
    x[9] = (0.25, 0.0, 0.75)
    return x, 3, 0, 0.25


def saturating():
    """Four points on a line, two of them 1e18 and 3e18 away: with nbrs_threshold = 2^53 - 2 and step 1 the threshold is raised
    twice and then no longer changes.  Returns (xyz, k, kpairs, nbrs_threshold, step)."""
    x = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0e18], [0.0, 0.0, -3.0e18]])
    return x, 2, 0, 9007199254740990.0, 1.0


def lattice_graph(a=12, b=12, c=3, seed=17):
    """(xyz, edges): an a x b x c unit lattice in shuffled order with an edge between every two points one unit apart."""
    g = np.random.default_rng(seed)
    ijk = np.stack(np.meshgrid(np.arange(a), np.arange(b), np.arange(c), indexing="ij"), -1).reshape(-1, 3)
    perm = g.permutation(len(ijk))
    ijk = ijk[perm]
    where = {tuple(p): i for i, p in enumerate(ijk.tolist())}
    edges = []
    for i, p in enumerate(ijk.tolist()):
        for ax in range(3):
            q = list(p)
            q[ax] += 1
            j = where.get(tuple(q))
            if j is not None:
                edges.append((i, j))
    e = np.asarray(edges, dtype=np.int64)
    return ijk.astype(np.float64), e[g.permutation(len(e))]


def multigraph(n=2000, seed=18):
    """(xyz, edges, base): three components of 1200 / 700 / 100 points (the base in the smallest), 6 000 random edges inside the
    components + 500 exact duplicates + 300 reversed duplicates + 200 self-loops, shuffled."""
    g = np.random.default_rng(seed)
    x = g.uniform(0, 10, (n, 3))
    comp = np.concatenate([np.zeros(1200, int), np.ones(700, int), np.full(100, 2)])[g.permutation(n)]
    members = [np.flatnonzero(comp == c) for c in range(3)]
    parts = []
    for m, cnt in zip(members, (3600, 2100, 300)):
        parts.append(np.stack([g.choice(m, cnt), g.choice(m, cnt)], 1))
    e = np.concatenate(parts)
    loops = np.repeat(g.choice(n, 200)[:, None], 2, axis=1)
    e = np.concatenate([e, e[g.choice(len(e), 500, replace=False)], e[g.choice(len(e), 300, replace=False)][:, ::-1], loops])
    return x, e[g.permutation(len(e))], int(members[2][0])


def star(n=4096, seed=19):
    """(xyz, edges, base): hub 0 joined to every other point; the base is a leaf."""
    x = uniform(n, seed)
    e = np.stack([np.zeros(n - 1, np.int64), np.arange(1, n)], 1)
    e[::2] = e[::2, ::-1].copy()
    return x, e, n - 1


def shuffled_path(n=300, seed=20):
    """(xyz, edges, base): the path 0 - 1 - ... - n-1 over random points, its edge list shuffled."""
    g = np.random.default_rng(seed)
    x = g.uniform(0, 1, (n, 3))
    e = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    return x, e[g.permutation(n - 1)], 0


def zero_cluster(m=20, tail=10, seed=21):
    """(xyz, edges, base): a chain of `tail` points from the base (index 0) whose last point is joined to two members of a cluster
    of m coincident points; the cluster is fully connected (zero-weight edges)."""
    g = np.random.default_rng(seed)
    t = np.zeros((tail, 3))
    t[:, 2] = np.arange(tail) * 0.25
    x = np.concatenate([t, np.tile(np.array([[0.5, 0.0, t[-1, 2]]]), (m, 1))])
    e = [(i, i + 1) for i in range(tail - 1)] + [(tail - 1, tail + 7), (tail + 3, tail - 1)]
    e += [(tail + i, tail + j) for i in range(m) for j in range(i + 1, m)]
    e = np.asarray(e, dtype=np.int64)
    return x, e[g.permutation(len(e))], 0


def isolated_base(n=30, seed=22):
    """(xyz, edges, base): random edges among the points 1 .. n-1; the base 0 has none."""
    g = np.random.default_rng(seed)
    return uniform(n, seed), g.integers(1, n, (60, 2)), 0


def big_shallow(n=600_000, random_edges=1_200_000, seed=23):
    """(xyz, edges, base): edges (i, i + 1) inside blocks of 64 and `random_edges` random ones: above the 2048 x 256 threads of a
    launch in nodes and in edges, and shallow."""
    g = np.random.default_rng(seed)
    x = g.uniform(0, 100, (n, 3))
    i = np.arange(n - 1)
    i = i[(i % 64) != 63]
    e = np.concatenate([np.stack([i, i + 1], 1), g.integers(0, n, (random_edges, 2))])
    return x, e, 0


def flipped(edges, seed=24):
    """The same undirected edges permuted, every orientation flipped."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return e[np.random.default_rng(seed).permutation(len(e))][:, ::-1].copy()


# ---- the growth cases of tests/test_gpu_pathlen_kernels.py: name -> (xyz, k, base, kpairs, thr, step, gthr) -------------------------

def _low(x, upto=None):
    return int(np.argmin(x[:upto, 2]))


def growth_cases():
    inf = float("inf")
    c = {}
    ch = chain()
    c["chain_k4_kp1"] = (ch, 4, 0, 1, 0.15, 0.05, inf)
    c["chain_k4_kp0"] = (ch, 4, 0, 0, 0.15, 0.05, inf)
    c["chain_k8_kp3_mid"] = (ch, 8, 200, 3, 0.15, 0.05, inf)
    du = duplicated()
    c["duplicated"] = (du, 12, _low(du), 1, 0.05, 0.02, inf)
    la = lattice()
    c["lattice_kp3"] = (la, 20, _low(la), 3, 0.15, 0.05, inf)
    c["lattice_kp30"] = (la, 20, _low(la), 30, 0.15, 0.05, inf)
    for off in ISLAND_OFFSETS:
        x = blob_island(off)
        c[f"island_{off}"] = (x, 20, _low(x, 120), 3, 0.15, 0.05, inf)
    x = blob_island(2.0, island=40)
    c["unreached"] = (x, 20, _low(x, 120), 3, 0.15, 0.05, inf)
    u = uniform(300, 25, 0.3)
    for name, g in (("gthr_0.05", 0.05), ("gthr_0", 0.0), ("gthr_neg", -1.0)):
        c[name] = (u, 10, _low(u), 3, 0.15, 0.05, g)
    two = np.array([[0.0, 0.0, 0.0], [0.1, 0.2, 0.3]])
    c["two_k1"] = (two, 1, 0, 3, 0.15, 0.05, inf)
    c["two_k2"] = (two, 2, 0, 3, 0.15, 0.05, inf)
    c["one_point"] = (np.array([[1.5, -2.25, 3.0]]), 1, 0, 3, 0.15, 0.05, inf)
    c["coincident"] = (coincident(), 10, 7, 3, 0.15, 0.05, inf)
    x, k, kp, thr = threshold_tie()
    c["threshold_tie"] = (x, k, 0, kp, thr, 0.05, inf)
    x, k, kp, thr, stp = saturating()
    c["saturating"] = (x, k, 0, kp, thr, stp, inf)
    return c


_grown = {}


def grown(name):
    """(case tuple, rows, Growth) of a growth case, computed once."""
    if name not in _grown:
        case = growth_cases()[name]
        x, k, base, kp, thr, stp, gthr = case
        rows = knn_rows(x, k)
        _grown[name] = (case, rows, grow(x, rows, base, kp, thr, stp, gthr))
    return _grown[name]


def sssp_cases():
    """name -> (xyz, edges, base): the small SSSP cases that are not growth outputs."""
    c = {}
    x, e = lattice_graph()
    c["lattice_graph"] = (x, e, 5)
    c["multigraph"] = multigraph()
    c["star"] = star()
    c["shuffled_path"] = shuffled_path()
    c["zero_cluster"] = zero_cluster()
    c["isolated_base"] = isolated_base()
    c["no_edges"] = (uniform(17, 26), np.zeros((0, 2), dtype=np.int64), 4)
    return c
