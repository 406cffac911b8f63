"""Path length, the parts that need no GPU: the CLI's interface, the fixtures' integrity and the argument checks of the Python
API and of the C entry points (they return before any launch)."""
import ctypes
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from pointstowood_amd import _lib
from pointstowood_amd import pathlength as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pathlength")


def _cli():
    spec = importlib.util.spec_from_file_location("p2w_pathlength_cli", os.path.join(ROOT, "pathlength.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parser_flags_and_defaults_equal_the_reference_script():
    """pathlength-batch.py:29-64: downsample 0.05, kpairs 3, knn 100, nbrs_threshold 0.15, nbrs_threshold_step 0.05."""
    cli = _cli()
    p = cli.build_parser()
    a = p.parse_args(["a.ply"])
    assert vars(a) == {"files": ["a.ply"], "downsample": 0.05, "kpairs": 3, "knn": 100, "nbrs_threshold": 0.15,
                       "nbrs_threshold_step": 0.05}
    b = p.parse_args(["a.ply b.ply", "c.ply", "--downsample", "0", "--kpairs", "1", "--knn", "16", "--nbrs-threshold", "0.2",
                      "--nbrs-threshold-step", "0.1"])
    assert cli.file_list(b) == ["a.ply", "b.ply", "c.ply"]
    assert (b.downsample, b.kpairs, b.knn, b.nbrs_threshold, b.nbrs_threshold_step) == (0.0, 1, 16, 0.2, 0.1)
    with pytest.raises(SystemExit):
        p.parse_args([])
    with pytest.raises(SystemExit):
        p.parse_args(["a.ply", "--knn", "2.5"])


def test_cli_refuses_other_formats_and_wide_knn_before_touching_the_gpu():
    with pytest.raises(SystemExit, match="only .ply"):
        _cli().main(["cloud.las"])
    with pytest.raises(SystemExit, match="--knn"):
        _cli().main(["cloud.ply", "--knn", "101"])


def test_pathlength_fixture_manifest_matches_the_files():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    files = sorted(f for f in os.listdir(GOLDEN) if f != "manifest.json")
    assert sorted(man) == files and len(files) == 7
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20
        assert hashlib.sha256(open(os.path.join(GOLDEN, f), "rb").read()).hexdigest() == man[f], f


def test_fixtures_hold_what_the_gpu_tests_read():
    for f in sorted(os.listdir(GOLDEN)):
        if not f.endswith(".npz"):
            continue
        z = np.load(os.path.join(GOLDEN, f))
        n = len(z["xyz"])
        assert z["step"].shape == (n,) and z["step"][int(z["base_id"])] == 0
        assert z["edges"].shape == (len(z["weights"]), 2) and np.all(z["edges"][:, 0] <= z["edges"][:, 1])
        assert int(z["knn"]) <= n


@pytest.mark.parametrize("kw, match", [
    (dict(knn=101), "knn"), (dict(knn=0), "knn"), (dict(knn=2.0), "knn"), (dict(base_id=50), "base_id"),
    (dict(base_id=-1), "base_id"), (dict(kpairs=-1), "kpairs"), (dict(nbrs_threshold_step=0.0), "nbrs_threshold_step"),
    (dict(nbrs_threshold_step=np.inf), "nbrs_threshold_step"), (dict(nbrs_threshold=np.nan), "nbrs_threshold"),
    (dict(graph_threshold=np.nan), "graph_threshold")])
def test_bad_arguments_raise_before_any_launch(kw, match):
    x = np.random.default_rng(0).uniform(0, 1, (50, 3))
    kw = {"knn": 10, **kw}
    with pytest.raises(ValueError, match=match):
        PL.path_length(x, **kw)


def test_knn_above_n_non_finite_and_bad_shapes_raise():
    x = np.zeros((20, 3))
    x[:, 0] = np.arange(20)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        PL.path_length(x, knn=21)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        PL.array_to_graph(x, 0, 3, 21, 0.15, 0.05)
    y = x.copy()
    y[3, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        PL.path_length(y, knn=5)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        PL.path_length(np.zeros((5, 2)), knn=2)
    with pytest.raises(ValueError, match="no points"):
        PL.path_length(np.zeros((0, 3)), knn=1)


def test_knn_slack_covers_the_grid_rounding():
    """After ring s the searches assume every unseen point is at least s * cell - slack away along some axis: the fp32 local
    coordinates and the fp32 division by the cell misplace a point by less than the slack."""
    g = np.random.default_rng(1)
    for E, cell in ((10.0, 0.05), (5.0e5, 0.3), (3000.0, 0.01)):
        o = 512345.678
        x = o + g.uniform(0, E, 200000)
        x[0] = o
        c = np.float32(cell)
        k = np.trunc((x - o).astype(np.float32) / c)
        lo, hi = k * float(c), (k + 1) * float(c)
        slack = PL.knn_slack(E)
        assert np.all(x - o >= lo - slack / 2) and np.all(x - o <= hi + slack / 2)


def test_pathlen_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    assert L.p2w_version() == 610
    fake = 16
    n = 1000
    need = int(L.p2w_pathlen_grow_ws_bytes(n))
    assert need >= 2 * 4 * n
    buf = ctypes.create_string_buffer(need + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    info = (ctypes.c_int64 * 6)()
    thr = ctypes.c_double()

    def grow(n=n, k=10, base=0, kpairs=3, step=0.05, gthr=np.inf, ws=ws, ws_bytes=need, nbr=fake):
        return L.p2w_pathlen_grow(fake, nbr, n, k, base, kpairs, 0.15, step, gthr, fake, fake, 100, ctypes.addressof(info),
                                  ctypes.addressof(thr), ws, ws_bytes, None)

    assert grow(n=0) == -1 and grow(k=0) == -1 and grow(k=101) == -1 and grow(n=5, k=6) == -1
    assert grow(base=-1) == -1 and grow(base=n) == -1 and grow(kpairs=-1) == -1
    assert grow(step=0.0) == -1 and grow(step=float("inf")) == -1 and grow(gthr=float("nan")) == -1
    assert grow(nbr=None) == -2 and grow(ws=None) == -2
    assert grow(ws=ws + 4) == -3
    assert grow(ws_bytes=need - 1) == -4
    sneed = int(L.p2w_pathlen_sssp_ws_bytes(n, 500))
    sinfo = (ctypes.c_int64 * 3)()
    assert L.p2w_pathlen_sssp(fake, fake, 500, n, n, fake, None, ctypes.addressof(sinfo), ws, sneed, None) == -1
    assert L.p2w_pathlen_sssp(fake, fake, -1, n, 0, fake, None, ctypes.addressof(sinfo), ws, sneed, None) == -1
    assert L.p2w_pathlen_sssp(fake, None, 500, n, 0, fake, None, ctypes.addressof(sinfo), ws, sneed, None) == -2
    assert L.p2w_pathlen_sssp(fake, fake, 500, n, 0, fake, None, ctypes.addressof(sinfo), ws, sneed - 1, None) == -4
    assert L.p2w_knn_wide_f64(fake, fake, fake, None, fake, n, 101, 0.0, fake, None) == -1
    assert L.p2w_knn_wide_f64(fake, fake, fake, None, fake, 5, 6, 0.0, fake, None) == -1
    assert L.p2w_knn_wide_f64(fake, fake, fake, None, fake, n, 10, -1.0, fake, None) == -1
    assert L.p2w_knn_wide_f64(None, fake, fake, None, fake, n, 10, 0.0, fake, None) == -2
    assert L.p2w_pathlen_weights(fake, fake, -1, fake, None) == -1
