"""Path length from the stem base on the GPU: ``array_to_graph`` + ``extract_path_info`` (``pointstowood/utils/shortest_path.py``).

The reference grows a graph over every point's ``knn`` nearest neighbours (sklearn, itself included in its row) one step at a time
from ``base_id``: a frontier step (:86-112) links every frontier point to the first ``kpairs + 1`` entries of its row that were not
processed before the step, and those entries form the next frontier; when the frontier is empty a gap step (:115-176) picks every
remaining point with a processed row entry closer than ``nbrs_threshold`` and links it to the first ``kpairs + 1`` processed and the
first ``kpairs + 1`` unprocessed entries of its row, or, when there is none, raises the threshold by ``nbrs_threshold_step``.  Edges
longer than ``graph_threshold`` are left out.  The path length of a point is its networkx Dijkstra distance from the base (:225).

Here the same steps run in ``csrc/p2w_pathlen.hip``: the rows come from ``p2w_knn_wide_f64`` (exact float64 distances on the plot grid
of ``plotgrid.build``, ordered by (distance, index)), the growth from ``p2w_pathlen_grow`` and the distances from ``p2w_pathlen_sssp`` (Bellman-Ford to the
fixed point, which is Dijkstra's result bit for bit).  Where no remaining row holds a processed point the reference raises its
threshold for ever; here those points are reported unreached (distance NaN, step -1).
"""
from __future__ import annotations

import math
import operator

import numpy as np
import torch

from . import _lib, plotgrid
from ._lib import check, lib, ptr
from .plotgrid import knn_slack  # noqa: F401  (a statement about the grid's construction, kept beside it)

_NONFINITE = "Input contains NaN or infinity."          # what sklearn raises
_TABLE_CELLS = 1 << 27                                  # largest grid of the kNN whose cell table is built


class NodeNotFound(ValueError):
    """The source of ``extract_path_info`` has no edge in the graph (networkx raises its NodeNotFound there)."""


def _index(v, name):
    try:
        return operator.index(v)
    except TypeError:
        raise ValueError(f"{name} must be an integer, got {v!r}") from None


def _check_args(n, base_id, kpairs, knn, nbrs_threshold, nbrs_threshold_step, graph_threshold):
    knn = _index(knn, "knn")
    kpairs = _index(kpairs, "kpairs")
    if not 1 <= knn <= _lib.MAX_K_WIDE:
        raise ValueError(f"knn must be in 1 .. {_lib.MAX_K_WIDE}, got {knn}")
    if n < 1:
        raise ValueError("the cloud has no points")
    if knn > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {knn}, n_samples_fit = {n}")
    if kpairs < 0:
        raise ValueError(f"kpairs must be >= 0, got {kpairs}")
    if base_id is not None:
        base_id = _index(base_id, "base_id")
        if not 0 <= base_id < n:
            raise ValueError(f"base_id {base_id} is not a point index of a cloud of {n} points")
    thr, stp, gthr = float(nbrs_threshold), float(nbrs_threshold_step), float(graph_threshold)
    if math.isnan(thr):
        raise ValueError("nbrs_threshold must not be NaN")
    if not (stp > 0.0) or math.isinf(stp):
        raise ValueError(f"nbrs_threshold_step must be finite and > 0, got {nbrs_threshold_step!r}")
    if math.isnan(gthr):
        raise ValueError("graph_threshold must not be NaN")
    return base_id, kpairs, knn, thr, stp, gthr


def _prepare(xyz, need_base, base_id, kpairs, knn, nbrs_threshold, nbrs_threshold_step, graph_threshold):
    """(float64 CUDA tensor [n, 3], True when the caller passed numpy, the checked arguments).  A numpy cloud is checked on the host
    (shape, finiteness) and uploaded only after every argument has been checked."""
    host = not isinstance(xyz, torch.Tensor)
    pts = np.asarray(xyz) if host else xyz
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be an [n, 3] array, got shape {tuple(pts.shape)}")
    if host:
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        if not np.isfinite(pts).all():
            raise ValueError(_NONFINITE)
    else:
        if not pts.dtype.is_floating_point:
            raise ValueError(f"points must be float32 or float64, got {pts.dtype}")
        _lib.require_cuda(pts)
        pts = pts.to(torch.float64).contiguous()
    args = _check_args(pts.shape[0], base_id, kpairs, knn, nbrs_threshold, nbrs_threshold_step, graph_threshold)
    if need_base and args[0] is None:
        raise ValueError("base_id must be a point index")
    if host:
        return torch.from_numpy(pts).to("cuda"), True, args
    if not bool(torch.isfinite(pts).all()):
        raise ValueError(_NONFINITE)
    return pts, False, args


def knn_rows(x64: torch.Tensor, k: int, stats: dict | None = None) -> torch.Tensor:
    """nbr [n, k] int32: row i = the k nearest points of point i (itself included) ascending by (float64 distance, index).

    Any grid cell gives the same rows; the cell only sets how many cells a search visits.  It is chosen so that an occupied cell
    holds about k / 2 points: a first grid at the cell of a uniform cloud in the bounding box, then one correction by the square
    root of the occupancy ratio (tree surfaces fill cells in two dimensions rather than three)."""
    L = lib()
    n = x64.shape[0]
    ext = (x64.max(0).values - x64.min(0).values).cpu().tolist()
    extent = max(ext)
    floor = extent * 2.0 ** -20
    vol = max(ext[0], floor) * max(ext[1], floor) * max(ext[2], floor)
    cell = max((vol / n * k / 2.0) ** (1.0 / 3.0), floor, 1e-9)
    g = plotgrid.build(x64, cell, _TABLE_CELLS)
    occ = int(g.occupied.item())
    per = n / max(occ, 1)
    better = max(cell * min(max(math.sqrt((k / 2.0) / per), 0.125), 8.0), floor, 1e-9)
    if abs(better / cell - 1.0) > 0.25:
        del g
        g = plotgrid.build(x64, better, _TABLE_CELLS)
        occ = int(g.occupied.item())
    nbr = torch.empty((n, k), dtype=torch.int32, device=x64.device)
    check(L.p2w_knn_wide_f64(ptr(g.xyz_sorted), ptr(g.order), ptr(g.keys), ptr(g.cell_start), ptr(g.grid), n, k, knn_slack(extent),
                             ptr(nbr), _lib.stream()), "knn_wide_f64")
    if stats is not None:
        stats.update(knn_cell=g.cell, knn_occupied_cells=occ, knn_table=g.cell_start is not None)
    return nbr


def _grow(x64, nbr, base, kpairs, thr, stp, gthr):
    """(step [n] int32, edges [E, 2] int32, info dict) of the reference's growth loop."""
    L = lib()
    n, k = nbr.shape
    dev = x64.device
    cap = n * 3 * min(kpairs + 1, k) + 16
    step = torch.empty(n, dtype=torch.int32, device=dev)
    edges = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.p2w_pathlen_grow_ws_bytes(n)), dtype=torch.uint8, device=dev)
    info = (_lib.C.c_int64 * 6)()
    thr_out = _lib.C.c_double()
    check(L.p2w_pathlen_grow(ptr(x64), ptr(nbr), n, k, base, kpairs, thr, stp, gthr, ptr(step), ptr(edges), cap,
                             _lib.C.addressof(info), _lib.C.addressof(thr_out), ptr(ws), ws.numel(), _lib.stream()), "pathlen_grow")
    m = int(info[0])
    return step, edges[:m], dict(edges=m, stop_step=int(info[1]), gap_steps=int(info[2]), threshold_raises=int(info[3]),
                                 grow_launches=int(info[4]), stopped_unreached=bool(info[5]), final_threshold=thr_out.value)


def _sssp(x64, edges, base, parents=False):
    """(dist [n] float64 with NaN where unreached, parent [n] int32 or None, info dict)."""
    L = lib()
    n, dev = x64.shape[0], x64.device
    m = edges.shape[0]
    dist = torch.empty(n, dtype=torch.float64, device=dev)
    parent = torch.empty(n, dtype=torch.int32, device=dev) if parents else None
    ws = torch.empty(int(L.p2w_pathlen_sssp_ws_bytes(n, m)), dtype=torch.uint8, device=dev)
    info = (_lib.C.c_int64 * 3)()
    check(L.p2w_pathlen_sssp(ptr(x64), ptr(edges) if m else None, m, n, base, ptr(dist), ptr(parent), _lib.C.addressof(info),
                             ptr(ws), ws.numel(), _lib.stream()), "pathlen_sssp")
    return dist, parent, dict(sssp_rounds=int(info[0]), hop_levels=int(info[1]), sssp_launches=int(info[2]))


def path_length(xyz, base_id=None, kpairs=3, knn=100, nbrs_threshold=0.15, nbrs_threshold_step=0.05, graph_threshold=np.inf,
                stats: dict | None = None):
    """(dist [n] float64, NaN where unreached; step [n] int32, -1 where never processed) of the points ``xyz`` [n, 3].

    ``xyz``: a numpy array (results: numpy) or a CUDA tensor (results: CUDA tensors).  ``base_id=None``: the first point of least z.
    The arguments are the reference's ``array_to_graph`` ones (shortest_path.py:6-8); the base has distance 0 and step 0 even when
    it has no edge.  ``stats`` (a dict, optional) receives the GPU time of the stages in ms (knn / grow / sssp, one after the other,
    each timed by events) and the counts of the growth (steps, edges, gap steps, threshold raises, launches)."""
    x64, host, (base_id, kpairs, knn, thr, stp, gthr) = _prepare(xyz, False, base_id, kpairs, knn, nbrs_threshold, nbrs_threshold_step,
                                                                 graph_threshold)
    n = x64.shape[0]
    if base_id is None:
        base_id = int(torch.argmin(x64[:, 2]).item())
    mark, elapsed_ms = _lib.stage_timer(stats is not None)
    mark()
    nbr = knn_rows(x64, knn, stats)
    mark()
    step, edges, ginfo = _grow(x64, nbr, base_id, kpairs, thr, stp, gthr)
    del nbr
    mark()
    dist, _, sinfo = _sssp(x64, edges, base_id)
    mark()
    if stats is not None:
        ms = elapsed_ms()
        stats.update(knn_ms=ms[0], grow_ms=ms[1], sssp_ms=ms[2], steps=int(step.max().item()), n=n, base_id=base_id, **ginfo, **sinfo)
    if host:
        return dist.cpu().numpy(), step.cpu().numpy()
    return dist, step


class PathGraph:
    """The graph ``array_to_graph`` returns: ``edges`` [E, 2] int64 (undirected, each once as (min, max), ascending, self-loops
    kept), ``weights`` [E] float64 (the endpoints' distance, shortest_path.py:241-266) and ``step_register`` (float64, NaN where
    never processed).  ``to_networkx()`` builds the equivalent networkx Graph (networkx is imported only then)."""

    def __init__(self, xyz: torch.Tensor, edges: torch.Tensor, step: torch.Tensor):
        self._xyz = xyz
        n = xyz.shape[0]
        e = edges.long()
        lo, hi = torch.minimum(e[:, 0], e[:, 1]), torch.maximum(e[:, 0], e[:, 1])
        code = torch.unique(lo * n + hi)
        self._edges_dev = torch.stack([code // n, code % n], 1).contiguous()
        w = torch.empty(code.numel(), dtype=torch.float64, device=xyz.device)
        check(lib().p2w_pathlen_weights(ptr(xyz), ptr(self._edges_dev), code.numel(), ptr(w), _lib.stream()), "pathlen_weights")
        self.n_points = n
        self.edges = self._edges_dev.cpu().numpy()
        self.weights = w.cpu().numpy()
        s = step.cpu().numpy()
        self.step_register = np.where(s < 0, np.nan, s.astype(np.float64))

    @property
    def nodes(self) -> np.ndarray:
        return np.unique(self.edges)

    def number_of_nodes(self) -> int:
        return int(self.nodes.size)

    def number_of_edges(self) -> int:
        return int(self.edges.shape[0])

    def __contains__(self, node) -> bool:
        return bool(np.any(self.edges == node))

    def to_networkx(self):
        import networkx as nx
        G = nx.Graph()
        G.add_weighted_edges_from((int(a), int(b), float(w)) for (a, b), w in zip(self.edges, self.weights))
        return G


def array_to_graph(arr, base_id, kpairs, knn, nbrs_threshold, nbrs_threshold_step, graph_threshold=np.inf, return_step=False):
    """``array_to_graph`` of shortest_path.py:6-192 on the GPU: a ``PathGraph`` (and the step register when ``return_step``)."""
    x64, _, (base_id, kpairs, knn, thr, stp, gthr) = _prepare(arr, True, base_id, kpairs, knn, nbrs_threshold, nbrs_threshold_step,
                                                              graph_threshold)
    nbr = knn_rows(x64, knn)
    step, edges, _ = _grow(x64, nbr, base_id, kpairs, thr, stp, gthr)
    G = PathGraph(x64, edges, step)
    return (G, G.step_register) if return_step else G


def extract_path_info(G: PathGraph, base_id, return_path=True):
    """``extract_path_info`` of shortest_path.py:195-238: (nodes_ids, distance[, path_list]) of every node reachable from
    ``base_id``, in ascending (distance, index) order; ``path_list[v]`` = [base_id, ..., v] along the parents of
    ``p2w_pathlen_sssp`` (every step a shortest-path edge)."""
    base_id = _index(base_id, "base_id")
    if not (0 <= base_id < G.n_points) or base_id not in G:
        raise NodeNotFound(f"Node {base_id} not found in graph")
    dist, parent, _ = _sssp(G._xyz, G._edges_dev.int().contiguous(), base_id, parents=bool(return_path))
    d = dist.cpu().numpy()
    ids = np.flatnonzero(~np.isnan(d))
    ids = ids[np.lexsort((ids, d[ids]))]
    nodes_ids, distance = ids.tolist(), d[ids].tolist()
    if not return_path:
        return nodes_ids, distance
    par = parent.cpu().numpy()
    paths = {base_id: [base_id]}
    for v in nodes_ids:                      # ascending distance: with fewest-hop parents a parent's path may still be missing
        chain = []
        u = v
        while u not in paths:
            chain.append(u)
            u = int(par[u])
        p = paths[u]
        for x in reversed(chain):
            p = p + [x]
            paths[x] = p
    return nodes_ids, distance, {v: paths[v] for v in nodes_ids}


def downsample(x64: torch.Tensor, size: float):
    """(reps [m] int64 ascending, owner [n] int64) of the CLI's downsampling: the ``p2w_voxel_sample`` grid of cell ``size`` over the
    fp32 coordinates local to the cloud's minimum, each occupied cell represented by its largest point index (as
    ``consecutive_cluster`` does), the representatives in ascending index order; owner[i] = the position in ``reps`` of point i's
    representative.  The reference script's ``downsample_cloud`` is not part of its tree, so this is the project's own rule."""
    n, dev = x64.shape[0], x64.device
    inv = torch.empty(n, dtype=torch.int32, device=dev)
    # (not a plotgrid.build: the representatives and the inverse map, no sorted order or keys)
    idx, ptr_out = plotgrid.voxel_sample(plotgrid.records(plotgrid.local(x64)[1]), size, inverse=inv)
    m = int(ptr_out[1].item())
    reps, perm = torch.sort(idx[:m].long())
    rank = torch.empty(m, dtype=torch.int64, device=dev)
    rank[perm] = torch.arange(m, device=dev)
    return reps, rank[inv.long()]
