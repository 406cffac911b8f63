"""Evaluation against truth labels on the GPU: ``p2w_confusion`` against numpy's bincount at every size and segment layout at which
the kernel takes another path, its weighted sums against exact and correctly rounded host sums, its reproducibility, its handling
of invalid points, and the three routes built on it (``binary_metrics`` of the recorded sklearn cases, ``compare_directory`` against
the reference's ``results.csv``, ``evaluate_voxels`` against ``predicter.classify``).  Reads only tests/golden/evaluate."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from pointstowood_amd import evaluate as EV
from tests.test_evaluate_cpu import CASES, GOLDEN, SCORES, U, close_to_sklearn, load_case

pytestmark = pytest.mark.gpu

CHUNK = _lib.EVAL_CHUNK


def draw(n, classes=2, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, classes, n).astype(np.float32), g.integers(0, classes, n).astype(np.float32)


def run(t, p, w=None, ptr=None, classes=2, strict=True):
    dev = "cuda"
    out = EV.confusion(torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev), None if w is None else torch.from_numpy(w).to(dev),
                       None if ptr is None else torch.as_tensor(ptr, dtype=torch.int64, device=dev), classes=classes, strict=strict)
    return [None if o is None else o.cpu().numpy() for o in out]


def bincounts(t, p, ptr, classes):
    """[S, C, C] by numpy: bincount of classes * t + p per segment."""
    cells = classes * classes
    return np.stack([np.bincount((classes * t[a:b] + p[a:b]).astype(np.int64), minlength=cells).reshape(classes, classes)
                     for a, b in zip(ptr[:-1], ptr[1:])])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7])
def test_counts_equal_bincount_around_every_size_edge(n):
    t, p = draw(n, seed=n)
    counts, wsum, invalid = run(t, p)
    assert counts.dtype == np.int64 and counts.shape == (1, 2, 2) and wsum is None
    assert np.array_equal(counts, bincounts(t, p, [0, n], 2)) and counts.sum() == n and invalid.tolist() == [0]


SEGMENTS = {
    "five_with_the_first_and_the_last_empty": [0, 0, 700, 1200, 1900, 1900],
    "one_point_segment": [0, 500, 501, 1300],
    "boundary_on_a_chunk_multiple": [0, 2 * CHUNK, 2 * CHUNK + 900],
    "boundary_one_past_a_chunk_multiple": [0, CHUNK + 1, 3 * CHUNK],
    "more_segments_than_chunks": np.concatenate([[0], np.cumsum(np.random.default_rng(64).integers(1, 10, 64))]).tolist(),
    "long_between_two_tiny": [0, 3, 3 + 2 * CHUNK + 1, 3 + 2 * CHUNK + 1 + 5],
}


@pytest.mark.parametrize("layout", sorted(SEGMENTS))
def test_segments_equal_a_bincount_per_segment(layout):
    ptr = SEGMENTS[layout]
    n = ptr[-1]
    t, p = draw(n, seed=len(ptr))
    w = np.random.default_rng(1).integers(1, 4097, n) / 1024.0
    counts, wsum, invalid = run(t, p, w, ptr)
    want = bincounts(t, p, ptr, 2)
    assert counts.shape == (len(ptr) - 1, 2, 2) and np.array_equal(counts, want)
    assert not invalid.any()
    exact = np.zeros(want.shape)
    seg = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    np.add.at(exact, (seg, t.astype(np.int64), p.astype(np.int64)), w)
    assert np.array_equal(wsum, exact)


@pytest.mark.parametrize("classes", [4, 8])
def test_more_classes_with_every_cell_hit_and_with_empty_cells(classes):
    n = 2 * CHUNK + 321
    t, p = draw(n, classes, seed=classes)
    ptr = [0, 1000, n]
    counts, _, invalid = run(t, p, ptr=ptr, classes=classes)
    assert counts.shape == (2, classes, classes) and (counts > 0).all() and not invalid.any()
    assert np.array_equal(counts, bincounts(t, p, ptr, classes))
    t2, p2 = np.minimum(t, classes - 2), np.where(p == 1, 0, p).astype(np.float32)      # the last row and column 1 stay empty
    counts, _, invalid = run(t2, p2, ptr=ptr, classes=classes)
    assert np.array_equal(counts, bincounts(t2, p2, ptr, classes)) and not invalid.any()
    assert not counts[:, classes - 1].any() and not counts[:, :, 1].any() and counts.sum() == n


def test_weights_of_1_1024_sum_exactly_and_path_lengths_within_the_summation_bound():
    n = 3 * CHUNK + 77
    t, p = draw(n, seed=5)
    ptr = [0, CHUNK + 5, n]
    seg = np.repeat(np.arange(2), np.diff(ptr))
    idx = (seg, t.astype(np.int64), p.astype(np.int64))
    g = np.random.default_rng(6)
    w = g.integers(1, 4097, n) / 1024.0                                   # every partial sum is exact in float64
    counts, wsum, _ = run(t, p, w, ptr)
    exact = np.zeros((2, 2, 2))
    np.add.at(exact, idx, w)
    assert wsum.dtype == np.float64 and np.array_equal(wsum, exact)
    w = (g.random(n) * 30).astype(np.float32).astype(np.float64)          # float32 path lengths in [0, 30)
    counts, wsum, _ = run(t, p, w, ptr)
    for s in range(2):
        for a in range(2):
            for b in range(2):
                mask = (seg == s) & (t == a) & (p == b)
                m, want = int(mask.sum()), math.fsum(w[mask])
                assert counts[s, a, b] == m
                # any order of summing m non-negative terms is within (m - 1) 2^-53 relative of the true sum
                err = abs(wsum[s, a, b] - want)
                print(f"cell {s}{a}{b}: {m} points, relative error {err / want:.3e}, bound {(m - 1) * U:.3e}")
                assert err <= (m - 1) * U * want


def test_two_calls_give_the_same_bits_and_segments_add_up():
    n = 5 * CHUNK + 1234
    t, p = draw(n, 4, seed=9)
    w = (np.random.default_rng(10).random(n) * 30).astype(np.float32).astype(np.float64)
    ptr = [0, 1111, CHUNK * 3, n]
    a = run(t, p, w, ptr, classes=4)
    b = run(t, p, w, ptr, classes=4)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    one = run(t, p, w, classes=4)
    again = run(t, p, w, classes=4)
    assert one[1].tobytes() == again[1].tobytes()
    assert np.array_equal(one[0][0], a[0].sum(axis=0))


INVALID = {
    "truth_2_of_2_classes": ("t", 2.0), "pred_minus_1": ("p", -1.0), "truth_half": ("t", 0.5), "truth_nan": ("t", float("nan")),
    "weight_nan": ("w", float("nan")), "weight_minus_1": ("w", -1.0), "weight_inf": ("w", float("inf")),
}


@pytest.mark.parametrize("kind", sorted(INVALID))
def test_invalid_points_enter_no_cell_and_strict_raises(kind):
    n = CHUNK + 300
    ptr = [0, 200, CHUNK + 100, n]
    t, p = draw(n, seed=11)
    w = np.random.default_rng(12).integers(1, 4097, n) / 1024.0
    which, value = INVALID[kind]
    at = [250, CHUNK + 50]                                 # both in segment 1, one in each of its chunks
    {"t": t, "p": p, "w": w}[which][at] = value
    counts, wsum, invalid = run(t, p, w, ptr, strict=False)
    assert invalid.tolist() == [0, 2, 0]
    keep = np.ones(n, dtype=bool)
    keep[at] = False
    kt, kp, kw = t[keep], p[keep], w[keep]
    kptr = [0, 200, CHUNK + 98, n - 2]
    assert np.array_equal(counts, bincounts(kt, kp, kptr, 2))
    exact = np.zeros((3, 2, 2))
    np.add.at(exact, (np.repeat(np.arange(3), np.diff(kptr)), kt.astype(np.int64), kp.astype(np.int64)), kw)
    assert np.array_equal(wsum, exact)
    with pytest.raises(ValueError, match="segment 1: 2 points"):
        run(t, p, w, ptr)


def test_any_real_dtype_and_unaligned_views_are_accepted():
    n = 1001
    t, p = draw(n + 1, seed=13)
    dev = "cuda"
    tt, pp = torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev)
    counts, _, _ = EV.confusion(tt[1:].to(torch.int64), pp[1:] > 0.5)
    want = bincounts(t[1:], p[1:], [0, n], 2)
    assert np.array_equal(counts.cpu().numpy(), want)
    counts, _, _ = EV.confusion(tt[1:], pp[1:].to(torch.float64))       # float32 view that starts 4 bytes into its storage
    assert np.array_equal(counts.cpu().numpy(), want)


@pytest.mark.parametrize("name", CASES)
def test_recorded_sklearn_cases_end_to_end(name):
    c = load_case(name)
    exact = bool(c["exact_weights"])
    counts, wsum, invalid = run(c["truth"], c["pred"], c["weight"], c["ptr"])
    assert np.array_equal(counts, c["matrix"]) and not invalid.any()
    for s in range(len(c["ptr"]) - 1):
        n = int(c["ptr"][s + 1] - c["ptr"][s])
        plain, weighted = EV.binary_metrics(counts[s]), EV.binary_metrics(wsum[s])
        for k in SCORES:
            assert close_to_sklearn(plain[k], float(c[k][s]), n, True), (s, k, plain[k], float(c[k][s]))
            assert close_to_sklearn(weighted[k], float(c["w_" + k][s]), n, exact), (s, k, weighted[k], float(c["w_" + k][s]))


def test_compare_directory_writes_the_reference_results(tmp_path, capsys):
    src = os.path.join(GOLDEN, "compare")
    work = tmp_path / "compare"
    shutil.copytree(src, work)
    os.remove(work / "results.csv")
    rows = EV.compare_directory(str(work), verbose=True)
    assert open(work / "results.csv").read() == open(os.path.join(src, "results.csv")).read()
    want = json.load(open(os.path.join(src, "compare.json")))
    assert [r["File"] for r in rows] == ["fin_x", "ger_1", "pol_a", "pol_b"]
    for r in rows:
        for who in ("fsct", "ours"):
            w = want[f"{r['File']}_{who}.ply"]
            assert r[f"Precision {who}"] == w["precision"] and r[f"Recall {who}"] == w["recall"] and r[f"F1 {who}"] == w["f1"]
            assert r[f"Accuracy {who}"] == w["balanced_accuracy"]
            assert close_to_sklearn(r[f"Accuracy weighted {who}"], w["weighted_balanced_accuracy"], w["n"], not w["has_pathlength"])
    out = capsys.readouterr().out
    assert f"Accuracy fsct: {rows[0]['Accuracy fsct']}, Accuracy ours: {rows[0]['Accuracy ours']}" in out
    files = open(work / "results_files.csv").read().splitlines()
    assert files[0].startswith("File,Accuracy fsct,") and len(files) == 5
    assert files[1].split(",")[:2] == ["fin_x", repr(rows[0]["Accuracy fsct"])]


def test_compare_directory_refuses_what_the_reference_cannot_score(tmp_path):
    from pointstowood_amd.io import read_ply, write_ply
    src = os.path.join(GOLDEN, "compare")
    good = read_ply(os.path.join(src, "pol_b_fsct.ply"))

    def attempt(name, ours, fsct):
        d = tmp_path / name
        d.mkdir()
        write_ply(str(d / "pol_b_ours.ply"), ours)
        write_ply(str(d / "pol_b_fsct.ply"), fsct)
        return str(d)
    bad_truth = dict(good, truth=np.where(np.arange(len(good["truth"])) == 3, 3.0, good["truth"]), label=np.where(good["label"] == 2, 0.0, good["label"]))
    with pytest.raises(ValueError, match="pol_b_ours.ply: truth outside"):
        EV.compare_directory(attempt("truth", bad_truth, good))
    label3 = dict(good, label=np.where(good["label"] == 1, 3.0, good["label"]))        # {0, 2, 3}: two remain, no remap, 3 is left
    with pytest.raises(ValueError, match="pol_b_fsct.ply: label outside"):
        EV.compare_directory(attempt("label", good, label3))
    both = dict(good, scalar_label=good["label"])
    with pytest.raises(ValueError, match="pol_b_ours.ply: column 'label' occurs twice"):
        EV.compare_directory(attempt("both", both, good))
    with pytest.raises(ValueError, match="no pol_x_ours.ply"):
        d = tmp_path / "alone"
        d.mkdir()
        write_ply(str(d / "pol_x_fsct.ply"), good)
        EV.compare_directory(str(d))


@pytest.fixture(scope="module")
def labelled():
    """(net, raw voxels [n, 5] = xyz, reflectance, label): 10 voxels of 300 - 2000 points."""
    from pointstowood_amd import Net, synthetic_voxels as synth, synthetic_weights as weights
    g = np.random.default_rng(30)
    voxels = []
    for i, n in enumerate(g.integers(300, 2001, 10)):
        pos, refl = synth.uniform_points(2.0, int(n), 100 + i, reflectance=True)
        y = torch.from_numpy((g.random(int(n)) < 0.4).astype(np.float32))
        voxels.append(torch.cat([pos, refl[:, None], y[:, None]], 1))
    net = Net(1, C=8, k=16)
    net.load_state_dict(weights.synth_state_dict(1, 8, seed=3), strict=True)
    return net.to("cuda").eval(), voxels


@pytest.mark.parametrize("drop_last", [False, True])
def test_evaluate_voxels_scores_the_labels_classify_would_write(labelled, drop_last):
    from pointstowood_amd.predicter import VoxelDataset, classify, prefetch_batches
    net, voxels = labelled
    res = EV.evaluate_voxels(net, EV.LabelledVoxelDataset(voxels), batch_size=4, drop_last=drop_last)
    batches = [[0, 1, 2, 3], [4, 5, 6, 7]] + ([] if drop_last else [[8, 9]])
    assert len(res["batches"]) == len(batches) == (2 if drop_last else 3)
    got = []
    rows = classify(net, prefetch_batches(VoxelDataset(voxels), batches), 0.5, "cuda", counts=got)
    assert got == [sum(len(voxels[i]) for i in b) for b in batches]
    total, at = np.zeros((2, 2), dtype=np.int64), 0
    for b, r, n in zip(batches, res["batches"], got):
        y = torch.cat([voxels[i][:, 4] for i in b]).numpy()
        want = bincounts(y, rows[at:at + n, 3].astype(np.float32), [0, n], 2)[0]
        at += n
        assert np.array_equal(r["matrix"], want) and r["matrix"].dtype == np.int64
        assert {k: r[k] for k in EV.METRICS} == EV.binary_metrics(want)
        total += want
    assert 0 < total[:, 1].sum() < total.sum()              # the synthetic model predicts both classes
    for k in EV.METRICS:
        mean = 0.0
        for r in res["batches"]:
            mean += r[k]
        assert res["mean"][k] == mean / len(batches)
    assert np.array_equal(res["pooled"]["matrix"], total)
    assert {k: res["pooled"][k] for k in EV.METRICS} == EV.binary_metrics(total)


def test_evaluate_voxels_reports_invalid_labels_once_at_the_end(labelled):
    net, voxels = labelled
    bad = [v.clone() for v in voxels[:6]]
    bad[5][10, 4] = 2.0
    with pytest.raises(ValueError, match="batch 1: 1 points"):
        EV.evaluate_voxels(net, EV.LabelledVoxelDataset(bad), batch_size=4)
