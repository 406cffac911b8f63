"""Path length on the MI355X (pointstowood_amd.pathlength, csrc/p2w_pathlen.hip) against the reference's array_to_graph +
extract_path_info (tests/golden/pathlength, written by make_golden_pathlength.py) and against brute-force numpy kNN rows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pointstowood_amd import io
from pointstowood_amd import pathlength as PL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pathlength")
CASES = ["tree_defaults", "tree_gaps", "tree_k16", "tree_graph_threshold", "tree_easting", "single_point", "knn_equals_n"]
# sklearn's "auto" picks its brute-force search when knn >= n / 2 and measures by the dot-product expansion there, so in that case
# the reference's weights are a few ulps from the exact distance: graph and steps are compared exactly, lengths to 1e-12
APPROX = {"knn_equals_n"}


def _same(got, want, name):
    if name in APPROX:
        return np.allclose(got, want, rtol=1e-12, atol=1e-15)
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def _case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def _args(c):
    return (int(c["kpairs"]), int(c["knn"]), float(c["nbrs_threshold"]), float(c["nbrs_threshold_step"]), float(c["graph_threshold"]))


def _expected_dist(c):
    d = np.full(len(c["xyz"]), np.nan)
    d[c["node_ids"]] = c["distance"]
    d[int(c["base_id"])] = 0.0
    return d


@pytest.mark.parametrize("name", CASES)
def test_fixture_graph_steps_and_distances_equal_the_reference(name):
    c = _case(name)
    base = int(c["base_id"])
    kp, knn, thr, stp, gthr = _args(c)
    G, steps = PL.array_to_graph(c["xyz"], base, kp, knn, thr, stp, gthr, return_step=True)
    assert np.array_equal(G.edges, c["edges"].astype(np.int64))
    assert _same(G.weights, c["weights"], name)
    assert np.array_equal(np.where(np.isnan(steps), -1, steps).astype(np.int32), c["step"])
    if int(c["no_source"]):
        with pytest.raises(PL.NodeNotFound):
            PL.extract_path_info(G, base, return_path=False)
    else:
        ids, dist = PL.extract_path_info(G, base, return_path=False)
        o = np.argsort(ids)
        assert np.array_equal(np.asarray(ids)[o], c["node_ids"])
        assert _same(np.asarray(dist)[o], c["distance"], name)
    dist, step = PL.path_length(c["xyz"], base, kp, knn, thr, stp, gthr)
    assert dist.dtype == np.float64 and step.dtype == np.int32
    assert np.array_equal(step, c["step"])
    want = _expected_dist(c)
    assert np.array_equal(np.isnan(dist), np.isnan(want))
    assert _same(dist[~np.isnan(want)], want[~np.isnan(want)], name)


def test_cuda_tensor_input_gives_cuda_results_equal_to_numpy():
    c = _case("tree_gaps")
    t = torch.from_numpy(c["xyz"]).cuda()
    dist, step = PL.path_length(t)                       # base_id None = the first point of least z
    assert dist.is_cuda and step.is_cuda and dist.dtype == torch.float64 and step.dtype == torch.int32
    assert np.array_equal(step.cpu().numpy(), c["step"])
    want = _expected_dist(c)
    assert np.array_equal(dist.cpu().numpy().view(np.uint64), want.view(np.uint64))


def _brute_rows(x, k):
    n = len(x)
    rows = np.empty((n, k), dtype=np.int64)
    for s in range(0, n, 512):
        q = x[s:s + 512]
        d = np.sqrt(((q[:, None, 0] - x[None, :, 0]) ** 2 + (q[:, None, 1] - x[None, :, 1]) ** 2) + (q[:, None, 2] - x[None, :, 2]) ** 2)
        idx = np.broadcast_to(np.arange(n), d.shape)
        o = np.lexsort((idx, d), axis=1)[:, :k]
        rows[s:s + 512] = o
    return rows


@pytest.mark.parametrize("k", [1, 64, 65, 100])
@pytest.mark.parametrize("offset", [0.0, 5.0e5])
def test_knn_rows_equal_brute_force_fp64_order(k, offset):
    g = np.random.default_rng(k)
    x = np.concatenate([g.uniform(0, 3, (3000, 3)), g.normal(1.5, 0.05, (1500, 3)), np.round(g.uniform(0, 3, (500, 3)), 2)])
    x = x + np.array([offset, 2 * offset, 0.0])
    got = PL.knn_rows(torch.from_numpy(x).cuda(), k).cpu().numpy()
    assert np.array_equal(got, _brute_rows(x, k))


def test_far_blob_is_left_unreached_and_the_tree_is_unchanged():
    c = _case("tree_defaults")
    g = np.random.default_rng(3)
    blob = g.normal(0, 0.05, (150, 3)) + c["xyz"].mean(0) + np.array([3.0, 0.0, 0.0]) + np.array([0.5, 0.0, 0.0])
    x = np.concatenate([c["xyz"], blob])
    st = {}
    dist, step = PL.path_length(x, int(c["base_id"]), *_args(c), stats=st)
    n = len(c["xyz"])
    assert st["stopped_unreached"] and np.all(np.isnan(dist[n:])) and np.all(step[n:] == -1)
    assert np.array_equal(step[:n], c["step"])
    assert np.array_equal(dist[:n].view(np.uint64), _expected_dist(c).view(np.uint64))


def test_parent_chains_are_shortest_acyclic_and_end_at_the_base():
    c = _case("tree_gaps")
    base = int(c["base_id"])
    G = PL.array_to_graph(c["xyz"], base, *_args(c))
    ids, dist, paths = PL.extract_path_info(G, base, return_path=True)
    d = dict(zip(ids, dist))
    w = {(int(a), int(b)): float(x) for (a, b), x in zip(G.edges, G.weights)}
    assert set(paths) == set(ids)
    for v in ids:
        p = paths[v]
        assert p[0] == base and p[-1] == v and len(set(p)) == len(p)
        acc = 0.0
        for a, b in zip(p[:-1], p[1:]):
            acc = acc + w[(min(a, b), max(a, b))]
            assert acc == d[b]
    assert d[base] == 0.0 and ids[0] == base


def test_two_runs_are_bit_equal():
    c = _case("tree_gaps")
    a = PL.path_length(c["xyz"])
    b = PL.path_length(c["xyz"])
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def test_cli_end_to_end(tmp_path):
    c = _case("tree_gaps")
    g = np.random.default_rng(5)
    x = np.concatenate([c["xyz"], c["xyz"][:2000] + g.normal(0, 0.01, (2000, 3))]) + np.array([300000.0, 5000000.0, 50.0])
    refl = g.uniform(-20, 0, len(x))
    path = str(tmp_path / "tree.ply")
    io.write_ply(path, {"x": x[:, 0], "y": x[:, 1], "z": x[:, 2], "reflectance": refl})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pathlength.py"), path, "--downsample", "0.05"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = io.read_ply(str(tmp_path / "tree_pathlength.ply"))
    # the downsample mapping restated in numpy: fp32 local coordinates, fp32 division, largest index per cell
    loc = (x - x.min(0)).astype(np.float32)
    key = np.trunc(loc / np.float32(0.05)).astype(np.int64)
    dims = key.max(0) + 1
    cell = (key[:, 2] * dims[1] + key[:, 1]) * dims[0] + key[:, 0]
    uc, inv = np.unique(cell, return_inverse=True)
    rep_of_cell = np.full(len(uc), -1)
    np.maximum.at(rep_of_cell, inv, np.arange(len(x)))
    reps = np.sort(rep_of_cell)
    owner = np.searchsorted(reps, rep_of_cell[inv])
    sub = x[reps]
    dist, _ = PL.path_length(sub, int(np.argmin(sub[:, 2])))
    d = dist[owner]
    keep = ~np.isnan(d)
    assert np.array_equal(out["x"], x[keep, 0]) and np.array_equal(out["reflectance"], refl[keep])
    assert np.array_equal(out["pathlength"].view(np.uint64), d[keep].view(np.uint64))
