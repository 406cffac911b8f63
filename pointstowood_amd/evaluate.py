"""Scoring a classification against truth labels on the GPU: the reference's ``pointstowood/comparetofsct.py`` (precision, recall,
balanced accuracy and path-length-weighted balanced accuracy of every ``*_ours.ply`` / ``*_fsct.ply`` pair of a directory) and the
held-out evaluation loop of ``pointstowood/src/trainer.py:223-267`` (the four sklearn scores per batch, averaged over the batches -
what the reference selects a checkpoint by).

Every score the reference takes from sklearn is a function of one confusion matrix, so the points are counted once, on the device,
by ``p2w_confusion`` (``csrc/p2w_eval.hip``: exact integer counts, fp64 weight sums with the same bits on every run), and the
scores are a few float64 operations on the host (``binary_metrics``).  numpy and torch only.

* ``confusion``             - the kernel's wrapper: [S, C, C] counts and weight sums of S segments, no host synchronisation.
* ``binary_metrics``        - precision / recall / f1 / balanced accuracy / accuracy of a 2 x 2 matrix, sklearn's formulas.
* ``LabelledVoxelDataset``  - ``VoxelDataset`` plus ``Data.y``: ``TrainingDataset`` without augmentation (trainer.py:46-60).
* ``evaluate_voxels``       - the held-out loop through ``Net.stream``; one device-to-host copy for the whole run.
* ``compare_directory``     - the flow of comparetofsct.py:29-165 with its ``results.csv``.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import _lib
from ._lib import aligned16 as _aligned, check, lib, ptr as _p
from .predicter import VoxelDataset, prefetch_batches

METRICS = ("precision", "recall", "f1", "balanced_accuracy", "accuracy")


def confusion(truth, pred, weight=None, ptr=None, classes: int = 2, strict: bool = True, out=None):
    """(counts [S, C, C] int64, wsum [S, C, C] float64 or None, invalid [S] int64), all on the device: ``counts[s, t, p]`` = the
    points of segment s with truth t and prediction p, ``wsum`` the sum of their weights, ``invalid[s]`` the points that entered no
    cell (an id that is not an integer in [0, classes), or a weight that is not finite and >= 0).

    ``truth`` / ``pred``: CUDA tensors of n class ids, any real dtype (converted to float32); ``weight``: n weights (converted to
    float64) or None; ``ptr``: [S + 1] ascending offsets with ptr[0] = 0 and ptr[S] = n, or None for one segment; ``classes``: 2 .. 8.
    ``out``: optional (counts, wsum, invalid) device tensors to write into (contiguous, S*C*C / S*C*C / S elements).
    Nothing here waits for the device except ``strict=True``, which reads ``invalid`` back and raises ``ValueError`` naming the
    first offending segment."""
    classes = int(classes)
    if not 2 <= classes <= _lib.EVAL_MAX_CLASSES:
        raise ValueError(f"classes must be in 2 .. {_lib.EVAL_MAX_CLASSES}, got {classes}")
    _lib.require_cuda(truth, pred, weight)
    dev = truth.device
    t = _aligned(truth.reshape(-1).to(torch.float32).contiguous())
    p = _aligned(pred.reshape(-1).to(torch.float32).contiguous())
    n = t.numel()
    if p.numel() != n:
        raise ValueError(f"truth has {n} points, pred {p.numel()}")
    w = None
    if weight is not None:
        w = _aligned(weight.reshape(-1).to(torch.float64).contiguous())
        if w.numel() != n:
            raise ValueError(f"truth has {n} points, weight {w.numel()}")
    if ptr is None:
        S, sp = 1, None
    else:
        ptr = torch.as_tensor(ptr)
        S = ptr.numel() - 1
        if S < 1:
            raise ValueError("ptr needs at least two entries")
        if not ptr.is_cuda:     # offsets on the host can be checked for free
            h = ptr.reshape(-1).to(torch.int64)
            if int(h[0]) != 0 or int(h[-1]) != n or bool((h[1:] < h[:-1]).any()):
                raise ValueError(f"ptr must ascend from 0 to {n}")
        sp = ptr.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    cells = S * classes * classes
    if out is None:
        counts = torch.empty(cells, dtype=torch.int64, device=dev)
        wsum = torch.empty(cells, dtype=torch.float64, device=dev) if w is not None else None
        invalid = torch.empty(S, dtype=torch.int64, device=dev)
    else:
        counts, wsum, invalid = out
        want = ((counts, torch.int64, cells), (invalid, torch.int64, S)) + (((wsum, torch.float64, cells),) if w is not None else ())
        for o, dt, size in want:
            if o is None or not o.is_cuda or o.dtype != dt or o.numel() != size or not o.is_contiguous():
                raise ValueError(f"out: a contiguous CUDA {dt} tensor of {size} elements is needed")
        wsum = wsum if w is not None else None
    L = lib()
    ws = torch.empty(int(L.p2w_confusion_ws_bytes(n, S, classes)), dtype=torch.uint8, device=dev)
    check(L.p2w_confusion(_p(t), _p(p), _p(w), _p(sp), n, S, classes, _p(counts), _p(wsum), _p(invalid), _p(ws), ws.numel(),
                          _lib.stream()), "p2w_confusion")
    if strict:
        _raise_invalid(invalid.cpu().numpy(), "segment")
    shape = (S, classes, classes)
    return counts.view(shape), (wsum.view(shape) if wsum is not None else None), invalid


def _raise_invalid(invalid, what):
    bad = np.flatnonzero(np.asarray(invalid))
    if bad.size:
        raise ValueError(f"{what} {int(bad[0])}: {int(invalid[bad[0]])} points with a class id that is no integer of the "
                         "class range, or a weight that is not finite and >= 0")


def _div(a, b):
    return float(a / b) if b != 0 else 0.0


def binary_metrics(m):
    """precision, recall, f1, balanced_accuracy and accuracy of a 2 x 2 matrix (row = truth, column = prediction; counts or weight
    sums), in float64 with the formulas of sklearn's ``precision_score`` / ``recall_score`` / ``f1_score`` (``average='binary',
    zero_division=0``) and ``balanced_accuracy_score``: an empty denominator gives 0.0; balanced accuracy is the mean recall of the
    classes that occur in the truth, NaN when there is none."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (2, 2):
        raise ValueError(f"a 2 x 2 matrix is needed, got shape {m.shape}")
    tn, fp, fn, tp = m[0, 0], m[0, 1], m[1, 0], m[1, 1]
    rows = m.sum(axis=1)
    recalls = [m[c, c] / rows[c] for c in range(2) if rows[c] != 0]
    return {
        "precision": _div(tp, tp + fp),
        "recall": _div(tp, tp + fn),
        "f1": _div(2 * tp, 2 * tp + fp + fn),
        "balanced_accuracy": float(np.mean(recalls)) if recalls else float("nan"),
        "accuracy": float((tp + tn) / m.sum()) if m.sum() != 0 else float("nan"),
    }


class LabelledVoxelDataset(VoxelDataset):
    """``VoxelDataset`` whose items also carry ``y`` = column ``label_index`` as float32: the reference's ``TrainingDataset`` without
    augmentation (trainer.py:46-60).  Rows the NaN filter drops lose their label too."""

    def __init__(self, voxels, reflectance_index: int = 3, label_index: int = 4):
        super().__init__(voxels, reflectance_index)
        self.label_index = label_index


def evaluate_voxels(model, dataset, batch_size: int = 4, threshold: float = 0.5, drop_last: bool = False, device="cuda"):
    """The reference's held-out evaluation (trainer.py:223-267) on one GPU: every batch of ``dataset`` (a ``LabelledVoxelDataset``)
    through ``model.stream`` as ``predicter.classify`` feeds it, predictions ``sigmoid(nan_to_num(logits)) >= threshold`` as
    ``predicter._consume`` makes them, one ``confusion`` call per batch into a row of a device buffer, ONE device-to-host copy at
    the end.

    Batches are ``batch_size`` consecutive voxels in dataset order (the reference's test loader has ``int(batch_size / 2)`` voxels per
    batch, shuffles and drops the last incomplete batch; the shuffle is not reproduced, ``drop_last=True`` gives its batch count).
    Returns ``{"batches": [{"matrix": 2 x 2 int64, **metrics}, ...], "mean": each metric summed over the batches and divided by the
    batch count (what the reference reports), "pooled": {"matrix": the summed matrix, **its metrics}}``."""
    bs = int(batch_size)
    if bs < 1:
        raise ValueError(f"batch_size must be at least 1, got {batch_size}")
    if not hasattr(model, "stream") or torch.device(device).type != "cuda":
        raise RuntimeError("evaluate_voxels needs a pointstowood_amd.Net on an MI355X (cuda) device; there is no CPU fallback")
    batches = [list(range(i, min(i + bs, len(dataset)))) for i in range(0, len(dataset), bs)]
    if drop_last and batches and len(batches[-1]) < bs:
        batches.pop()
    buf = torch.zeros((len(batches), 5), dtype=torch.int64, device=device)      # per batch: tn, fp, fn, tp, invalid
    held = []

    def feed():
        for data in prefetch_batches(dataset, batches, pin=True):
            d = data.to(device, non_blocking=True)
            held.append(d)
            yield d
    with torch.no_grad():
        for i, logits in enumerate(model.stream(feed())):
            d = held.pop(0)
            preds = torch.sigmoid(torch.nan_to_num(logits)).reshape(-1) >= threshold
            confusion(d.y, preds, classes=2, strict=False, out=(buf[i, :4], None, buf[i, 4:]))
    host = buf.cpu().numpy()
    _raise_invalid(host[:, 4], "batch")
    rows = []
    for r in host:
        m = r[:4].reshape(2, 2).copy()
        rows.append({"matrix": m, **binary_metrics(m)})
    mean = {}
    for k in METRICS:
        total = 0.0
        for r in rows:
            total += r[k]
        mean[k] = total / len(rows) if rows else float("nan")
    pooled = host[:, :4].sum(axis=0).reshape(2, 2)
    return {"batches": rows, "mean": mean, "pooled": {"matrix": pooled, **binary_metrics(pooled)}}


# ---- comparetofsct.py ------------------------------------------------------------------------------------------------------------

COUNTRIES = {"pol": "Poland", "spa": "Spain", "fin": "Finland"}                 # comparetofsct.py:129-134
RESULT_COLUMNS = ("Accuracy fsct", "Accuracy ours", "Accuracy weighted fsct", "Accuracy weighted ours", "Precision fsct",
                  "Precision ours", "Recall fsct", "Recall ours")              # the column order its column sort arrives at (:153)


def _columns(path):
    """The columns of one file with the ``scalar_`` prefixes stripped (comparetofsct.py:39,42)."""
    from .io import read_ply
    out = {}
    for name, v in read_ply(path).items():
        name = name.replace("scalar_", "")
        if name in out:
            raise ValueError(f"{path}: column '{name}' occurs twice once the scalar_ prefixes are stripped")
        out[name] = v
    for need in ("truth", "label"):
        if need not in out:
            raise ValueError(f"{path}: no '{need}' column")
    return out


def _file_matrices(path, remap: bool):
    """(2 x 2 counts, 2 x 2 weight sums or None) of one file: ONE 4-class confusion of truth x label on the device, weighted by
    ``pathlength`` where the column exists, and the reference's rules as arithmetic on the 4 x 4 matrices: the points labelled 2
    leave (:40,43), and for the fsct file (``remap``) more than two remaining distinct labels turn the label into ``label == 3``
    (:73)."""
    cols = _columns(path)
    dev = "cuda"
    w = torch.from_numpy(np.ascontiguousarray(cols["pathlength"], dtype=np.float64)).to(dev) if "pathlength" in cols else None
    t = torch.from_numpy(np.ascontiguousarray(cols["truth"], dtype=np.float32)).to(dev)
    l = torch.from_numpy(np.ascontiguousarray(cols["label"], dtype=np.float32)).to(dev)
    counts, wsum, invalid = confusion(t, l, w, classes=4, strict=False)
    got = torch.cat([counts.reshape(-1).to(torch.float64), wsum.reshape(-1) if wsum is not None else counts.new_zeros(0, dtype=torch.float64),
                     invalid.to(torch.float64)]).cpu().numpy()        # (counts below 2^53 are exact in float64: one copy)
    if got[-1] > 0:
        raise ValueError(f"{path}: {int(got[-1])} points whose truth or label is no integer in 0 .. 3, or whose pathlength is not "
                         "finite and >= 0")
    mats = [got[:16].reshape(4, 4)] + ([got[16:32].reshape(4, 4)] if wsum is not None else [])
    c = mats[0]
    present = [k for k in (0, 1, 3) if c[:, k].sum() > 0]              # the distinct labels once label 2 has left
    if c[2:, present].sum() > 0:
        raise ValueError(f"{path}: truth outside {{0, 1}}")
    binary = len(present) > 2 and remap
    if not binary and 3 in present:
        raise ValueError(f"{path}: label outside {{0, 1}}")
    out = []
    for m in mats:
        m = m[:2]
        out.append(np.stack([m[:, 0] + m[:, 1], m[:, 3]], axis=1) if binary else m[:, :2].copy())
    return out[0].astype(np.int64), (out[1] if wsum is not None else None)


def _repr_row(values):
    return ",".join(repr(float(v)) for v in values)


def compare_directory(path, verbose: bool = False):
    """The reference's ``comparetofsct.py DIR`` (:29-165): for every ``*_fsct.ply`` of ``path`` with its ``*_ours.ply``, precision, recall,
    balanced accuracy and ``pathlength``-weighted balanced accuracy of ``label`` against ``truth`` for both files (weight 1 where there
    is no ``pathlength`` column).  Returns the per-file rows (dicts, ascending by file name) and writes ``results.csv`` in the
    reference's layout - one row per country (the file name's first three characters; pol / spa / fin spelt out), the mean over its
    files rounded to 8 decimals - and ``results_files.csv`` with the per-file rows, unrounded.  The reference's PNG table is not
    written."""
    files = sorted(glob.glob(os.path.join(path, "*_fsct.ply")))
    if not files:
        raise ValueError(f"{path}: no *_fsct.ply file")
    rows = []
    for fsct_file in files:
        base = os.path.basename(fsct_file)[: -len("_fsct.ply")]
        ours_file = os.path.join(path, base + "_ours.ply")
        if not os.path.exists(ours_file):
            raise ValueError(f"{fsct_file}: no {base}_ours.ply beside it")
        row = {"File": base}
        for who, f in (("fsct", fsct_file), ("ours", ours_file)):
            counts, wsum = _file_matrices(f, remap=who == "fsct")
            m = binary_metrics(counts)
            row[f"Precision {who}"], row[f"Recall {who}"], row[f"Accuracy {who}"] = m["precision"], m["recall"], m["balanced_accuracy"]
            row[f"F1 {who}"] = m["f1"]
            row[f"Accuracy weighted {who}"] = binary_metrics(wsum)["balanced_accuracy"] if wsum is not None else m["balanced_accuracy"]
        if verbose:
            print(fsct_file)
            print(f"Accuracy fsct: {row['Accuracy fsct']}, Accuracy ours: {row['Accuracy ours']}")
        rows.append(row)
    by_country = {}
    for r in rows:
        by_country.setdefault(COUNTRIES.get(r["File"][:3], r["File"][:3]), []).append(r)
    with open(os.path.join(path, "results.csv"), "w") as f:
        f.write("Country," + ",".join(RESULT_COLUMNS) + "\n")
        for country in sorted(by_country):
            group = by_country[country]
            f.write(country + "," + _repr_row(np.round(np.mean([r[c] for r in group]), 8) for c in RESULT_COLUMNS) + "\n")
    with open(os.path.join(path, "results_files.csv"), "w") as f:
        f.write("File," + ",".join(RESULT_COLUMNS) + "\n")
        for r in rows:
            f.write(r["File"] + "," + _repr_row(r[c] for c in RESULT_COLUMNS) + "\n")
    return rows
