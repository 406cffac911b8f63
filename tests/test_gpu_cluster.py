"""Euclidean clustering on the MI355X (pointstowood_amd.cluster, csrc/p2w_cluster.hip) against the reference's EuclideanCluster
(tests/golden/cluster, written by make_golden_cluster.py) and against scipy's KD-tree + connected components."""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from pointstowood_amd import io
from pointstowood_amd.cluster import EuclideanCluster, euclidean_cluster

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster")
CASES = ["blobs_noise", "lattice_tie", "lattice_easting", "duplicates_tol0", "filter_minmax", "single_point", "empty"]


def _case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["xyz"], float(z["tolerance"]), float(z["min_size"]), float(z["max_size"]), z["labels"]


@pytest.mark.parametrize("name", CASES)
def test_fixture_labels_equal_the_reference(name):
    xyz, tol, mn, mx, want = _case(name)
    got = EuclideanCluster(tol, mn, mx).cluster(xyz)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    t = torch.from_numpy(xyz).cuda()
    lab = EuclideanCluster(tol, mn, mx).cluster(t)
    assert lab.is_cuda and lab.dtype == torch.int64
    assert np.array_equal(lab.cpu().numpy(), want)
    labels, n_clusters = euclidean_cluster(t, tol, mn, mx)
    assert n_clusters == (int(want.max()) + 1 if want.size else 0)


def _scipy_labels(xyz, r, mn, mx):
    """scipy query_pairs + connected_components, components renumbered by their smallest index, sizes filtered."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = len(xyz)
    pr = cKDTree(xyz).query_pairs(r, output_type="ndarray")
    _, comp = connected_components(coo_matrix((np.ones(len(pr)), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
    first = np.full(comp.max() + 1, n)
    np.minimum.at(first, comp, np.arange(n))
    size = np.bincount(comp)
    keep = (size >= mn) & (size <= mx)
    order = np.argsort(first)
    kept = order[keep[order]]
    rank = np.full(len(first), -1)
    rank[kept] = np.arange(len(kept))
    return rank[comp]


def _clustered_cloud(n, seed, offset=(0.0, 0.0, 0.0)):
    g = np.random.default_rng(seed)
    n_blob = 60
    centres = g.uniform([0, 0, 0], [60, 60, 20], (n_blob, 3))
    share = g.dirichlet(np.ones(n_blob)) * n * 0.9
    pts = [c + g.standard_normal((max(int(s), 1), 3)) * g.uniform(0.2, 1.0) for c, s in zip(centres, share)]
    pts.append(g.uniform([0, 0, 0], [60, 60, 20], (n - sum(len(p) for p in pts), 3)))
    p = np.concatenate(pts)[g.permutation(n)]
    return p + np.asarray(offset)


@pytest.mark.parametrize("n,seed,offset,r,mn,mx", [
    (120_000, 0, (0.0, 0.0, 0.0), 0.08, 1, np.inf),
    (200_000, 1, (512345.25, 6012345.5, 80.0), 0.05, 5, 20000),
    (300_000, 2, (0.0, 0.0, 0.0), 0.12, 10, np.inf),
])
def test_random_clouds_against_scipy(n, seed, offset, r, mn, mx):
    pytest.importorskip("scipy")
    xyz = _clustered_cloud(n, seed, offset)
    want = _scipy_labels(xyz, r, mn, mx)
    labels, k = euclidean_cluster(torch.from_numpy(xyz).cuda(), r, mn, mx)
    got = labels.cpu().numpy()
    assert k == int(want.max()) + 1 and k > 10
    assert np.array_equal(got, want)


def test_float32_input_is_clustered_on_its_float64_values():
    pytest.importorskip("scipy")
    xyz = _clustered_cloud(100_000, 3).astype(np.float32)
    want = _scipy_labels(xyz.astype(np.float64), 0.07, 2, np.inf)
    got = EuclideanCluster(0.07, 2).cluster(xyz)
    assert np.array_equal(got, want)


def test_bisection_path_equals_the_table_path():
    xyz = torch.from_numpy(_clustered_cloud(150_000, 4, (300000.0, 0.0, 0.0))).cuda()
    st_t, st_b = {}, {}
    a, ka = euclidean_cluster(xyz, 0.06, 3, np.inf, stats=st_t)
    b, kb = euclidean_cluster(xyz, 0.06, 3, np.inf, table_cells=1, stats=st_b)
    assert st_t["table"] and not st_b["table"]
    assert st_t["pairs"] == st_b["pairs"] > 0
    assert ka == kb and torch.equal(a, b)


def test_two_runs_give_bit_equal_labels():
    xyz = torch.from_numpy(_clustered_cloud(250_000, 5)).cuda()
    a, ka = euclidean_cluster(xyz, 0.1, 1)
    b, kb = euclidean_cluster(xyz, 0.1, 1)
    assert ka == kb and torch.equal(a, b)
    st = {}
    c, kc = euclidean_cluster(xyz, 0.1, 1, stats=st)         # the stages launched one at a time: the same result
    assert kc == ka and torch.equal(a, c)


def test_one_giant_component_is_fast_and_correct():
    """A 100^3 lattice of spacing 0.25 (exact in binary: every axis neighbour at d == r exactly), visited in a random order: one
    component of 10^6 points, the worst case for the union-find's trees."""
    g = torch.Generator().manual_seed(0)
    idx = torch.stack(torch.meshgrid(*[torch.arange(100)] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = (idx[torch.randperm(idx.shape[0], generator=g)].double() * 0.25 + torch.tensor([400000.0, 10.0, 5.0],
           dtype=torch.float64)).cuda()
    euclidean_cluster(xyz[:1000], 0.25, 1)                    # warm up the library
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels, k = euclidean_cluster(xyz, 0.25, 1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert k == 1 and bool((labels == 0).all())
    labels, k = euclidean_cluster(xyz, 0.25, 1, 10**6 - 1)   # too large: every point is noise
    assert k == 0 and bool((labels == -1).all())
    labels, k = euclidean_cluster(xyz, 0.2499, 1)             # below the spacing: 10^6 singletons, numbered by index
    assert k == 10**6 and torch.equal(labels, torch.arange(10**6, device=labels.device))
    assert dt < 5.0, dt


def test_non_finite_input_and_bad_tolerance_raise():
    xyz = torch.rand(1000, 3, dtype=torch.float64).cuda()
    for v in (float("nan"), float("inf"), -float("inf")):
        bad = xyz.clone()
        bad[517, 1] = v
        with pytest.raises(ValueError, match="data must be finite, check for nan or inf values"):
            euclidean_cluster(bad, 0.1, 1)
        with pytest.raises(ValueError, match="data must be finite"):
            EuclideanCluster(0.1, 1).cluster(bad)
    for tol in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="cluster_tolerance"):
            euclidean_cluster(xyz, tol, 1)
    with pytest.raises(ValueError, match="safe cell"):
        euclidean_cluster(xyz, 0.1, 1, cell=0.05)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        euclidean_cluster(xyz[:, :2], 0.1, 1)


def test_cli_end_to_end(tmp_path):
    inp = tmp_path / "cli_input.ply"
    shutil.copy(os.path.join(GOLDEN, "cli_input.ply"), inp)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "euclidean_clustering.py"), str(inp)], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    want = json.load(open(os.path.join(GOLDEN, "cli.json")))
    lines = r.stdout.splitlines()
    assert f"Number of clusters: {want['n_clusters']}" in lines
    assert f"Number of noise points: {want['n_noise']}" in lines
    out = tmp_path / "cli_input_clustered.ply"
    ref = os.path.join(GOLDEN, "cli_input_clustered.ply")
    got_cols, ref_cols = io.read_ply(str(out)), io.read_ply(ref)
    assert list(got_cols) == list(ref_cols) == ["x", "y", "z", "reflectance", "pwood", "cluster_id"]
    for c in ref_cols:
        assert np.array_equal(got_cols[c], ref_cols[c]), c
    assert out.read_bytes() == open(ref, "rb").read()
