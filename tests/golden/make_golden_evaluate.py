#!/usr/bin/env python3
"""Generate the evaluation fixtures in tests/golden/evaluate/ FROM THE REFERENCE AND FROM SKLEARN.

Run by hand in the authoring container (sklearn, pandas and tqdm installed), never by a test:

    python tests/golden/make_golden_evaluate.py --reference /path/to/PointsToWood

  matrix_<case>.npz   truth, pred [n] float32, weight [n] float64, ptr [S + 1] int64, exact_weights (every weight a multiple of
                      1/1024: every partial sum is exact in float64), and per segment what sklearn returns for it:
                      precision / recall / f1 (``average='binary', zero_division=0``) and balanced_accuracy [S], the same four with
                      ``sample_weight`` as w_precision ... [S], and ``confusion_matrix(labels=[0, 1])`` without and with the
                      weights as matrix [S, 2, 2] int64 / w_matrix [S, 2, 2] float64
  compare/            eight PLY files written by the reference's ``save_file`` (pol_a, pol_b, fin_x, ger_1, each as _ours and _fsct),
                      the ``results.csv`` the reference's unmodified ``comparetofsct.py`` wrote for that directory (run through
                      ``runpy`` with a stand-in ``dataframe_image`` module, which the script needs only for its PNG table), and
                      ``compare.json``: sklearn's values per file, after the script's drop / remap rules restated with pandas here
  manifest.json       sha256 of every file above

The reference's source never enters this repository; only these data vectors do.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import runpy
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "evaluate")


def matrix_cases():
    g = np.random.default_rng(20)

    def exact(n):
        return g.integers(1, 4097, n).astype(np.float64) / 1024.0                    # multiples of 1/1024 in (0, 4]

    def labels(n, p=0.5):
        return (g.random(n) < p).astype(np.float32)
    n = 6000
    t = labels(n, 0.3)
    noisy = np.where(g.random(n) < 0.85, t, 1 - t).astype(np.float32)
    out = {
        "random_binary": (t, noisy, exact(n), [0, 1, 700, 4796, n]),
        "truth_all_0": (np.zeros(900, np.float32), labels(900), exact(900), [0, 400, 900]),
        "truth_all_1": (np.ones(900, np.float32), labels(900), exact(900), [0, 900]),
        "pred_all_0": (labels(1100), np.zeros(1100, np.float32), exact(1100), [0, 1100]),
        "pred_all_1": (labels(1100), np.ones(1100, np.float32), exact(1100), [0, 300, 1100]),
        "one_point": (np.ones(1, np.float32), np.ones(1, np.float32), exact(1), [0, 1]),
        "weights_1024": (t, noisy, exact(n), [0, 2500, n]),
        "weights_pathlength": (t, noisy, (g.random(n) * 30).astype(np.float32).astype(np.float64), [0, 2500, n]),
    }
    return out


def sklearn_scores(t, p, w=None):
    from sklearn.metrics import balanced_accuracy_score, confusion_matrix, f1_score, precision_score, recall_score
    t, p = t.astype(int), p.astype(int)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "y_pred contains classes not in y_true" of the single-class cases
        return {
            "precision": precision_score(t, p, average="binary", zero_division=0, sample_weight=w),
            "recall": recall_score(t, p, average="binary", zero_division=0, sample_weight=w),
            "f1": f1_score(t, p, average="binary", zero_division=0, sample_weight=w),
            "balanced_accuracy": balanced_accuracy_score(t, p, sample_weight=w),
            "matrix": confusion_matrix(t, p, labels=[0, 1], sample_weight=w),
        }


def write_matrices():
    for name, (t, p, w, ptr) in matrix_cases().items():
        ptr = np.asarray(ptr, dtype=np.int64)
        rec = {}
        for s in range(len(ptr) - 1):
            a, b = ptr[s], ptr[s + 1]
            for prefix, ww in (("", None), ("w_", w[a:b])):
                for k, v in sklearn_scores(t[a:b], p[a:b], ww).items():
                    rec.setdefault(prefix + k, []).append(v)
        arrays = {k: np.asarray(v, dtype=np.int64 if k == "matrix" else np.float64) for k, v in rec.items()}
        np.savez_compressed(os.path.join(OUT, f"matrix_{name}.npz"), truth=t, pred=p, weight=w, ptr=ptr,
                            exact_weights=np.bool_(bool(np.all(w * 1024 == np.round(w * 1024)))), **arrays)
        print(f"matrix_{name}: {len(t)} points, {len(ptr) - 1} segments")


def compare_clouds():
    """name -> (columns of the _ours file, columns of the _fsct file).  Label 2 (the reference drops those points) occurs in every
    fsct file and in one ours file; pol_a's fsct labels are {0, 1, 2, 3} (-> label == 3), pol_b's {0, 1, 2} (two remain: kept as they
    are); fin_x has no pathlength column; ger_1's ours file carries scalar_ prefixes."""
    g = np.random.default_rng(21)
    out = {}
    for name, n in (("pol_a", 900), ("pol_b", 640), ("fin_x", 500), ("ger_1", 777)):
        def cloud(flip, labels4=False, with2=True):
            m = n - int(g.integers(0, 40))
            truth = (g.random(m) < 0.35).astype(np.float64)
            label = np.where(g.random(m) < flip, 1 - truth, truth)
            if labels4:                            # FSCT's classes: 0 terrain, 1 vegetation, 2 coarse woody debris, 3 stem
                label = np.where(label == 1, 3.0, np.where(g.random(m) < 0.2, 0.0, 1.0))
            if with2:
                label = np.where(g.random(m) < 0.07, 2.0, label)
            cols = {"x": g.uniform(0, 20, m), "y": g.uniform(0, 20, m), "z": g.uniform(0, 25, m), "truth": truth, "label": label}
            if name != "fin_x":
                cols["pathlength"] = (g.random(m) * 30).astype(np.float32).astype(np.float64)
            return cols
        ours = cloud(0.08, with2=name == "pol_b")
        fsct = cloud(0.2, labels4=name in ("pol_a", "ger_1"))
        if name == "ger_1":
            ours = {(k if k in "xyz" else "scalar_" + k): v for k, v in ours.items()}
        out[name] = (ours, fsct)
    return out


def file_scores(df, remap):
    """sklearn's values for one file after the rules of comparetofsct.py:39-43,73,100-106, restated with pandas."""
    df = df.rename(columns=lambda c: c.replace("scalar_", ""))
    df = df[df["label"] != 2]
    label = df["label"]
    if remap and label.nunique() > 2:
        label = (label == 3).astype(int)
    t, p = df["truth"].to_numpy(), label.to_numpy()
    w = df["pathlength"].to_numpy() if "pathlength" in df.columns else np.ones(len(df))
    plain, weighted = sklearn_scores(t, p), sklearn_scores(t, p, w)
    return {"n": int(len(df)), "precision": plain["precision"], "recall": plain["recall"], "f1": plain["f1"],
            "balanced_accuracy": plain["balanced_accuracy"], "weighted_balanced_accuracy": weighted["balanced_accuracy"],
            "has_pathlength": "pathlength" in df.columns, "matrix": plain["matrix"].tolist()}


def write_compare(reference):
    import pandas as pd
    sys.path.insert(0, os.path.join(reference, "pointstowood"))
    import src.io as ref_io
    cdir = os.path.join(OUT, "compare")
    os.makedirs(cdir, exist_ok=True)
    scores = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, pair in compare_clouds().items():
            for who, cols in zip(("ours", "fsct"), pair):
                df = pd.DataFrame(cols)
                f = os.path.join(tmp, f"{name}_{who}.ply")
                ref_io.save_file(f, df.copy(), additional_fields=[c for c in df.columns if c not in ("x", "y", "z")])
                scores[f"{name}_{who}.ply"] = file_scores(ref_io.load_file(f), remap=who == "fsct")
        stand_in = types.ModuleType("dataframe_image")        # the script imports it for its PNG table only
        stand_in.export = lambda *a, **k: None
        sys.modules["dataframe_image"] = stand_in
        argv = sys.argv
        sys.argv = ["comparetofsct.py", tmp]
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                runpy.run_path(os.path.join(reference, "pointstowood", "comparetofsct.py"), run_name="__main__")
        finally:
            sys.argv = argv
            del sys.modules["dataframe_image"]
        text = open(os.path.join(tmp, "results.csv")).read()
        lines = text.splitlines()
        assert lines[0] == ("Country,Accuracy fsct,Accuracy ours,Accuracy weighted fsct,Accuracy weighted ours,Precision fsct,"
                            "Precision ours,Recall fsct,Recall ours"), lines[0]
        # a last-bit difference of a weighted sum must not be able to flip the rounding to 8 decimals: no unrounded value of the
        # table, times 1e8, lies within 1e-3 of a half-integer
        means = {}
        for fname, s in scores.items():
            means.setdefault((fname[:3], fname[-8:-4]), []).append(s)
        for group in means.values():
            for k in ("precision", "recall", "balanced_accuracy", "weighted_balanced_accuracy"):
                x = float(np.mean([s[k] for s in group])) * 1e8
                assert abs(x - np.floor(x) - 0.5) > 1e-3, (k, x)
        for f in sorted(os.listdir(tmp)):
            if f.endswith(".ply") or f == "results.csv":
                shutil.copy(os.path.join(tmp, f), os.path.join(cdir, f))
    with open(os.path.join(cdir, "compare.json"), "w") as f:
        json.dump(scores, f, indent=1, sort_keys=True)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds pointstowood/comparetofsct.py)")
    args = ap.parse_args()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    write_matrices()
    write_compare(os.path.abspath(args.reference))
    man = {}
    for root, _, files in os.walk(OUT):
        for f in files:
            rel = os.path.relpath(os.path.join(root, f), OUT)
            if rel != "manifest.json":
                man[rel] = hashlib.sha256(open(os.path.join(root, f), "rb").read()).hexdigest()
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    for rel in man:
        assert os.path.getsize(os.path.join(OUT, rel)) < 256 << 10, rel


if __name__ == "__main__":
    main()
