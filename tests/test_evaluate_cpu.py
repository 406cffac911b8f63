"""Evaluation against truth labels, the parts that need no GPU: ``binary_metrics`` against the recorded sklearn values, the fixtures'
integrity, the CLI's interface and the C entry point's argument checks (they return before any launch)."""
import ctypes
import hashlib
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from pointstowood_amd import evaluate as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "evaluate")
CASES = ("random_binary", "truth_all_0", "truth_all_1", "pred_all_0", "pred_all_1", "one_point", "weights_1024", "weights_pathlength")
SCORES = ("precision", "recall", "f1", "balanced_accuracy")
U = 2.0 ** -53


def load_case(name):
    return dict(np.load(os.path.join(GOLDEN, f"matrix_{name}.npz")))


def close_to_sklearn(got, want, n, exact):
    """The rule of every comparison with a recorded sklearn value: the same bits where every sum is exact (counts, weights that
    are multiples of 1/1024), within 4 n 2^-53 relative otherwise (n terms per sum, two sums and a division per score, and as much
    again for sklearn's own sums)."""
    if math.isnan(want):
        return math.isnan(got)
    return got == want if exact else abs(got - want) <= 4 * n * U * abs(want)


def host_matrices(t, p, w, a, b):
    idx = (t[a:b].astype(np.int64), p[a:b].astype(np.int64))
    m, mw = np.zeros((2, 2)), np.zeros((2, 2))
    np.add.at(m, idx, 1.0)
    np.add.at(mw, idx, w[a:b])
    return m, mw


def _cli():
    spec = importlib.util.spec_from_file_location("p2w_comparetofsct_cli", os.path.join(ROOT, "comparetofsct.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", CASES)
def test_binary_metrics_equal_the_recorded_sklearn_values(name):
    c = load_case(name)
    exact = bool(c["exact_weights"])
    assert exact == (name != "weights_pathlength")
    ptr = c["ptr"]
    for s in range(len(ptr) - 1):
        a, b = int(ptr[s]), int(ptr[s + 1])
        m, mw = host_matrices(c["truth"], c["pred"], c["weight"], a, b)
        assert np.array_equal(m, c["matrix"][s])
        plain, weighted = EV.binary_metrics(m), EV.binary_metrics(mw)
        assert EV.binary_metrics(m.astype(np.int64)) == plain
        for k in SCORES:
            assert close_to_sklearn(plain[k], float(c[k][s]), b - a, True), (name, s, k, plain[k], float(c[k][s]))
            assert close_to_sklearn(weighted[k], float(c["w_" + k][s]), b - a, exact), (name, s, k, weighted[k], float(c["w_" + k][s]))
        assert plain["accuracy"] == (m[0, 0] + m[1, 1]) / (b - a)


def test_binary_metrics_edge_cases():
    z = EV.binary_metrics(np.zeros((2, 2)))
    assert z["precision"] == 0.0 and z["recall"] == 0.0 and z["f1"] == 0.0 and math.isnan(z["balanced_accuracy"])
    m = EV.binary_metrics([[3, 1], [2, 4]])
    assert m == {"precision": 4 / 5, "recall": 4 / 6, "f1": 8 / 11, "balanced_accuracy": float(np.mean([3 / 4, 4 / 6])), "accuracy": 0.7}
    with pytest.raises(ValueError, match="2 x 2"):
        EV.binary_metrics(np.zeros((4, 4)))


def test_evaluate_fixture_manifest_matches_the_files():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    files = sorted(os.path.relpath(os.path.join(r, f), GOLDEN) for r, _, fs in os.walk(GOLDEN) for f in fs if f != "manifest.json")
    assert sorted(man) == files and len(files) == len(CASES) + 10
    for f in files:
        assert hashlib.sha256(open(os.path.join(GOLDEN, f), "rb").read()).hexdigest() == man[f], f
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20


def test_cli_parser():
    p = _cli().build_parser()
    assert vars(p.parse_args(["plots"])) == {"directory": "plots"}
    with pytest.raises(SystemExit):
        p.parse_args([])
    with pytest.raises(SystemExit):
        p.parse_args(["a", "b"])


def test_cli_refuses_a_missing_or_empty_directory_before_touching_the_library(tmp_path, monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(EV, "lib", no_library)
    with pytest.raises(SystemExit, match="no such directory"):
        _cli().main([str(tmp_path / "nowhere")])
    (tmp_path / "pol_a_ours.ply").write_bytes(b"")
    with pytest.raises(SystemExit, match=r"no \*_fsct.ply"):
        _cli().main([str(tmp_path)])


def test_eval_chunk_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "p2w.h")).read()
    assert int(re.search(r"#define P2W_EVAL_CHUNK (\d+)", hdr).group(1)) == _lib.EVAL_CHUNK
    assert int(re.search(r"#define P2W_EVAL_MAX_CLASSES (\d+)", hdr).group(1)) == _lib.EVAL_MAX_CLASSES
    assert _lib.EVAL_CHUNK % 4 == 0


def test_confusion_argument_errors():
    """p2w_confusion refuses bad sizes, a missing, misaligned or short workspace and weights without their output (or the reverse)
    before it launches anything; the workspace is sized for n / CHUNK + segments chunks without reading seg_ptr."""
    L = _lib.lib()
    assert L.p2w_version() == 610
    n, S, C = 100000, 3, 2
    need = int(L.p2w_confusion_ws_bytes(n, S, C))
    chunks = n // _lib.EVAL_CHUNK + S
    assert need >= 8 * (S + 1) + chunks * (4 * (C * C + 1) + 8 * C * C)
    assert int(L.p2w_confusion_ws_bytes(n, S, 8)) > need > int(L.p2w_confusion_ws_bytes(0, 1, C)) > 0
    buf = ctypes.create_string_buffer(need + 16)
    ws = (ctypes.addressof(buf) + 15) & ~15
    fake = 16

    def call(n=n, segments=S, classes=C, weight=None, wsum=None, seg_ptr=fake, ws=ws, ws_bytes=need, truth=fake):
        return L.p2w_confusion(truth, fake, weight, seg_ptr, n, segments, classes, fake, wsum, fake, ws, ws_bytes, None)

    assert call(n=-1) == -1
    assert call(classes=1) == -1 and call(classes=9) == -1
    assert call(segments=0) == -1 and call(segments=-2) == -1
    assert call(seg_ptr=None) == -1                      # no seg_ptr: one segment
    assert call(ws=None) == -2
    assert call(ws=ws + 4) == -3
    assert call(ws_bytes=need - 1) == -4
    assert call(wsum=fake) == -1 and call(weight=fake) == -1
    assert call(truth=None) == -2 and call(truth=20) == -3


def test_confusion_refuses_host_tensors_and_bad_arguments():
    t = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EV.confusion(t, t)
    with pytest.raises(ValueError, match="classes"):
        EV.confusion(t, t, classes=9)


def test_labelled_dataset_filters_the_labels_with_the_nan_rows(capsys):
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.rand(50, 3, generator=g), torch.rand(50, 1, generator=g), (torch.rand(50, 1, generator=g) < 0.5).float()], 1)
    v[7, 3] = float("nan")
    d = EV.LabelledVoxelDataset([v, v[:7]])
    a, b = d[0], d[1]
    keep = torch.ones(50, dtype=torch.bool)
    keep[7] = False
    assert a.pos.shape[0] == 49 and torch.equal(a.y, v[keep, 4]) and a.y.dtype == torch.float32
    assert torch.equal(b.y, v[:7, 4]) and "y" in b.keys()
    from pointstowood_amd.predicter import VoxelDataset
    assert not hasattr(VoxelDataset([v])[0], "y")
    capsys.readouterr()
