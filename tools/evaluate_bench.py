#!/usr/bin/env python3
"""Evaluation against truth labels (pointstowood_amd.evaluate): the confusion kernel as a streaming read, the reference's four
sklearn calls on one batch on the same host, and ``evaluate_voxels`` beside ``classify_voxels``.

    python tools/evaluate_bench.py [--n 10000000] [--repeat 20] [--voxels 64] [--out profiles/evaluate_bench.json]

* ``p2w_confusion`` at ``--n`` points, S = 1 and S = 256 segments, without and with float64 weights: the median of ``--repeat``
  event-timed calls after two warm-up calls (the three launches of a call, workspace allocated before) that rotate over copies
  of the input 1 GiB in all, so that no call reads what an earlier one left in the 256 MiB Infinity Cache; bytes per second
  counting 8 B per point unweighted (two float32 ids) and 16 B weighted.  ``hbm_fraction`` divides by 8 TB/s, the MI355X's HBM3E peak.
* The reference's evaluation of one batch (trainer.py:239-242: precision_score, recall_score, balanced_accuracy_score, f1_score) on
  131 072 points, wall time on this host, when sklearn can be imported; ``null`` otherwise.
* ``evaluate_voxels`` points per second on ``--voxels`` synthetic voxels, beside ``predicter.classify`` over the same batches
  (``--batch-size`` voxels in dataset order through ``Net.stream``) and ``classify_voxels`` with its own point-budget batches; best of
  three runs each after one warm-up run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import Net, _lib, evaluate as EV  # noqa: E402
from pointstowood_amd import synthetic_voxels as synth, synthetic_weights as weights  # noqa: E402
from pointstowood_amd.predicter import VoxelDataset, classify, classify_voxels, prefetch_batches  # noqa: E402

HBM_PEAK = 8.0e12
ROTATE_BYTES = 1 << 30        # four times the 256 MiB Infinity Cache: no call finds its input cached by an earlier one


def kernel_runs(n, segments, weighted, repeat, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    t = (torch.rand(n, device=dev, generator=g) < 0.3).float()
    p = (torch.rand(n, device=dev, generator=g) < 0.3).float()
    w = torch.rand(n, device=dev, generator=g, dtype=torch.float64) * 30 if weighted else None
    ptr = None if segments == 1 else torch.linspace(0, n, segments + 1, device=dev).to(torch.int64)
    out = (torch.empty(segments * 4, dtype=torch.int64, device=dev), torch.empty(segments * 4, dtype=torch.float64, device=dev) if weighted else None,
           torch.empty(segments, dtype=torch.int64, device=dev))
    L = _lib.lib()
    ws = torch.empty(int(L.p2w_confusion_ws_bytes(n, segments, 2)), dtype=torch.uint8, device=dev)
    nbytes = n * (16 if weighted else 8)
    copies = -(-ROTATE_BYTES // nbytes)          # the calls rotate over copies of the input that together exceed the Infinity Cache
    sets = [(t, p, w)] + [(t.clone(), p.clone(), None if w is None else w.clone()) for _ in range(copies - 1)]
    ms = []
    for i in range(repeat + 2):
        ti, pi, wi = sets[i % copies]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(L.p2w_confusion(ti.data_ptr(), pi.data_ptr(), _lib.ptr(wi), _lib.ptr(ptr), n, segments, 2, out[0].data_ptr(),
                                   _lib.ptr(out[1]), out[2].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), "p2w_confusion")
        b.record()
        b.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    assert int(out[0].sum()) == n and int(out[2].sum()) == 0
    med = statistics.median(ms)
    return {"segments": segments, "weighted": weighted, "rotating_inputs": copies, "ms_median": med, "ms_min": min(ms), "bytes": nbytes,
            "bytes_per_s": nbytes / (med * 1e-3), "hbm_fraction": nbytes / (med * 1e-3) / HBM_PEAK, "points_per_s": n / (med * 1e-3)}


def sklearn_batch(n=131072):
    try:
        from sklearn.metrics import balanced_accuracy_score, f1_score, precision_score, recall_score
    except ImportError:
        return None
    g = np.random.default_rng(0)
    y, p = torch.from_numpy((g.random(n) < 0.3).astype(np.float32)), torch.from_numpy((g.random(n) < 0.3).astype(np.int64))
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        precision_score(y, p, average="binary", zero_division=0)
        recall_score(y, p, average="binary", zero_division=0)
        balanced_accuracy_score(y, p, sample_weight=None)
        f1_score(y, p, average="binary", zero_division=0)
        best = min(best, time.perf_counter() - t0)
    return {"n": n, "ms_best_of_3": best * 1e3, "calls": "precision_score, recall_score, balanced_accuracy_score, f1_score (trainer.py:239-242)"}


def voxel_runs(count, batch_size, dev):
    g = np.random.default_rng(1)
    voxels = []
    for i, n in enumerate(g.integers(2000, 16385, count)):
        pos, refl = synth.uniform_points(2.0, int(n), 500 + i, reflectance=True)
        voxels.append(torch.cat([pos, refl[:, None], torch.from_numpy((g.random(int(n)) < 0.4).astype(np.float32))[:, None]], 1))
    points = sum(len(v) for v in voxels)
    net = Net(1)
    net.load_state_dict(weights.synth_state_dict(1, 32, seed=0), strict=True)
    net = net.to(dev).eval()
    batches = [list(range(i, min(i + batch_size, count))) for i in range(0, count, batch_size)]
    labelled, plain = EV.LabelledVoxelDataset(voxels), VoxelDataset(voxels)

    def best(fn):
        times = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times[1:])
    te = best(lambda: EV.evaluate_voxels(net, labelled, batch_size=batch_size))
    tc = best(lambda: classify(net, prefetch_batches(plain, batches), 0.5, "cuda"))
    tv = best(lambda: classify_voxels(net, plain))
    return {"voxels": count, "points": points, "batch_size": batch_size, "evaluate_voxels_s": te, "evaluate_voxels_points_per_s": points / te,
            "classify_same_batches_s": tc, "classify_same_batches_points_per_s": points / tc,
            "classify_voxels_s": tv, "classify_voxels_points_per_s": points / tv}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--voxels", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "n": a.n, "chunk": _lib.EVAL_CHUNK, "hbm_peak_bytes_per_s": HBM_PEAK, "confusion": []}
    for segments in (1, 256):
        for weighted in (False, True):
            r = kernel_runs(a.n, segments, weighted, a.repeat, dev)
            res["confusion"].append(r)
            print(f"S={segments} weighted={weighted}: {r['ms_median']:.3f} ms  {r['bytes_per_s'] / 1e12:.2f} TB/s "
                  f"({100 * r['hbm_fraction']:.0f} % of HBM peak)", flush=True)
    res["sklearn_batch"] = sklearn_batch()
    print("sklearn, one 131 072-point batch:", res["sklearn_batch"], flush=True)
    res["voxels"] = voxel_runs(a.voxels, a.batch_size, dev)
    print(res["voxels"], flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
