"""Euclidean clustering, the parts that need no GPU: the CLI's interface, the fixtures' integrity, the grid cell's safety bound and
the C entry point's argument checks (they return before any launch)."""
import ctypes
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from pointstowood_amd import cluster as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster")


def _cli():
    spec = importlib.util.spec_from_file_location("p2w_euclidean_clustering_cli", os.path.join(ROOT, "euclidean_clustering.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parser_flags_and_defaults_equal_the_reference():
    """pointstowood/src/euclidean_clustering.py:49-55: positional input_file, --cluster_tolerance 0.1 (float), --min_cluster_size 10
    and --max_cluster_size 10000 (int)."""
    p = _cli().build_parser()
    a = p.parse_args(["cloud.ply"])
    assert vars(a) == {"input_file": "cloud.ply", "cluster_tolerance": 0.1, "min_cluster_size": 10, "max_cluster_size": 10000}
    b = p.parse_args(["c.ply", "--cluster_tolerance", "0.25", "--min_cluster_size", "3", "--max_cluster_size", "7"])
    assert (b.cluster_tolerance, b.min_cluster_size, b.max_cluster_size) == (0.25, 3, 7)
    assert isinstance(b.min_cluster_size, int) and isinstance(b.max_cluster_size, int)
    with pytest.raises(SystemExit):
        p.parse_args(["c.ply", "--min_cluster_size", "2.5"])
    with pytest.raises(SystemExit):
        p.parse_args([])


def test_cli_refuses_other_formats_before_touching_the_gpu():
    with pytest.raises(SystemExit, match="only .ply"):
        _cli().main(["cloud.las"])


def test_cluster_fixture_manifest_matches_the_files():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    files = sorted(f for f in os.listdir(GOLDEN) if f != "manifest.json")
    assert sorted(man) == files
    for f in files:
        assert hashlib.sha256(open(os.path.join(GOLDEN, f), "rb").read()).hexdigest() == man[f], f


def test_safe_cell_keeps_every_joined_pair_in_adjacent_cells():
    """The bound of cluster.safe_cell, exercised the way the grid is built: pairs at exactly the tolerance along an axis, at the
    largest coordinates of the extent, float32 local coordinates and float32 key division."""
    g = np.random.default_rng(0)
    for r, E in ((0.1, 100.0), (0.05, 5.0e5), (1e-4, 3000.0), (0.0, 50.0), (2.0, 1.0)):
        origin = 512345.678
        x = origin + g.uniform(0, E, 20000)
        x[:2] = origin, origin + E
        y = x + r * (1 - g.random(x.size) * 1e-12) * np.where(g.random(x.size) < 0.5, -1, 1)
        ok = np.abs(x - y) <= r
        lo = min(x.min(), y.min())
        ext = max(x.max(), y.max()) - lo
        c = np.float32(CL.safe_cell(r, ext))
        assert float(c) >= r and c > 0 and ext / float(c) <= 2 ** 20 + 1
        ux = (x - lo).astype(np.float32)
        uy = (y - lo).astype(np.float32)
        kx, ky = np.trunc(ux / c), np.trunc(uy / c)
        assert np.all(np.abs(kx - ky)[ok] <= 1), (r, E)


def test_size_bounds_follow_the_reference_comparison():
    assert CL._size_bounds(10, 10000) == (10, 10000)
    assert CL._size_bounds(2.5, np.inf) == (3, 1 << 62)
    assert CL._size_bounds(0, 7.9) == (0, 7)
    lo, hi = CL._size_bounds(float("nan"), 5)
    assert lo > hi


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf")])
def test_bad_tolerance_is_a_value_error(bad):
    with pytest.raises(ValueError, match="cluster_tolerance"):
        CL.euclidean_cluster(torch.zeros(4, 3), bad, 1)


@pytest.mark.parametrize("shape", [(5,), (5, 2), (5, 4)])
def test_points_must_have_three_columns(shape):
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        CL.euclidean_cluster(torch.zeros(shape), 0.1, 1)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        CL.EuclideanCluster(0.1, 1).cluster(np.zeros(shape))


def test_non_finite_numpy_input_raises_the_scipy_message():
    p = np.zeros((3, 3))
    p[1, 2] = np.nan
    with pytest.raises(ValueError, match="data must be finite, check for nan or inf values"):
        CL.EuclideanCluster(0.1, 1).cluster(p)


def test_euclid_cluster_argument_errors():
    """p2w_euclid_cluster refuses bad sizes, tolerances and stages and a missing or short workspace before it launches anything."""
    L = _lib.lib()
    assert L.p2w_version() == 610
    n = 1000
    need = int(L.p2w_euclid_cluster_ws_bytes(n))
    assert need >= 4 * 4 * n
    buf = ctypes.create_string_buffer(need + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    fake = 16

    def call(n=n, tol=0.1, stages=_lib.CLUSTER_ALL, ws=ws, ws_bytes=need):
        return L.p2w_euclid_cluster(fake, fake, fake, None, fake, n, tol, 1, 10, stages, fake, fake, None, ws, ws_bytes, None)

    assert call(n=-1) == -1
    assert call(n=1 << 31) == -1
    assert call(tol=-0.5) == -1
    assert call(tol=float("nan")) == -1
    assert call(tol=float("inf")) == -1
    assert call(stages=0) == -1 and call(stages=8) == -1
    assert call(ws=None) == -2
    assert call(ws=ws + 4) == -3
    assert call(ws_bytes=need - 1) == -4
    assert L.p2w_euclid_cluster(None, fake, fake, None, fake, n, 0.1, 1, 10, _lib.CLUSTER_LINK, fake, fake, None, ws, need, None) == -2
    assert L.p2w_euclid_cluster(fake, fake, fake, None, fake, n, 0.1, 1, 10, _lib.CLUSTER_NUMBER, None, fake, None, ws, need, None) == -2
