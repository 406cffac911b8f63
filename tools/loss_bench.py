#!/usr/bin/env python3
"""Forward + backward of the Poly-1 focal loss (pointstowood_amd.loss.Poly1FocalLoss, csrc/p2w_loss.hip) with ``reduction="mean"``
against the same composite written in plain PyTorch operations on the same GPU - what the reference's class executes there.

    python tools/loss_bench.py [--repeat 20] [--out profiles/loss_bench.json]

* Sizes: 131 072 elements (one 8 x 16 384-point batch) and 10^7.  The trainer's configuration: gamma = 2, alpha = None,
  label_smoothing = 0.1.
* One step = ``loss = criterion(logits, labels); loss.backward()`` with a fresh ``.grad``.  The median of ``--repeat`` event-timed
  steps after a warm-up pass over every input; the steps rotate over copies of the inputs 1 GiB in all, so that no step reads what
  an earlier one left in the 256 MiB Infinity Cache.
* ``launches``: the kernels of one step, counted by ``torch.profiler`` in a run of its own (not timed).
* ``hbm_fraction`` (10^7 only): the bytes the fused step has to move - 8 B read and 4 B of derivative written per element in the
  forward, 4 B read and 4 B written in the backward's multiply: 20 B per element - over the median time, over 8 TB/s, the MI355X's
  HBM3E peak.  The same byte count is divided into the PyTorch composite's time, so its figure is its share of that minimum, not of
  the traffic it really has.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402

HBM_PEAK = 8.0e12
ROTATE_BYTES = 1 << 30
STEP_BYTES_PER_ELEMENT = 20
CONFIG = dict(epsilon=0.1, gamma=2.0, alpha=None, label_smoothing=0.1, eps=1e-6)


def composite_mean(logits, labels, epsilon, gamma, alpha, label_smoothing, eps):
    """The loss's formula, one PyTorch operation per step of it."""
    z = logits.clamp(-10, 10)
    y = labels if label_smoothing is None else labels * (1 - label_smoothing) + 0.5 * label_smoothing
    p = torch.sigmoid(z).clamp(eps, 1 - eps)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="none").clamp(max=100.0)
    pt = (y * p + (1 - y) * (1 - p)).clamp(eps, 1 - eps)
    focal = torch.pow(1 - pt, gamma).clamp(max=2.0) * ce
    if alpha is not None:
        focal = (alpha * y + (1 - alpha) * (1 - y)) * focal
    loss = (focal + (epsilon * torch.pow(1 - pt, gamma + 1)).clamp(max=100.0)).clamp(0.0, 100.0)
    return torch.where(torch.isnan(loss), torch.zeros_like(loss), loss).mean()


def count_launches(step):
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    count = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
    return count or None          # None: the profiler recorded no device activity here; the launches are then not counted


def measure(fn, n, repeat, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    copies = max(2, -(-ROTATE_BYTES // (8 * n)))
    sets = []
    for _ in range(copies):
        x = (torch.randn(n, device=dev, generator=g) * 4).requires_grad_()
        sets.append((x, (torch.rand(n, device=dev, generator=g) < 0.3).float()))

    def step(i):
        x, y = sets[i % copies]
        x.grad = None
        loss = fn(x, y)
        loss.backward()
        return loss
    for i in range(copies):
        step(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    out = {"n": n, "rotating_inputs": copies, "us_median": med * 1e3, "us_min": min(ms) * 1e3, "us_max": max(ms) * 1e3, "repeat": repeat,
           "launches": count_launches(lambda: step(0)), "loss": float(step(0))}
    if n >= 10 ** 7:
        out["hbm_fraction"] = STEP_BYTES_PER_ELEMENT * n / (med * 1e-3) / HBM_PEAK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[131072, 10_000_000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs an MI355X: a time taken elsewhere says nothing about it")
    dev = torch.device("cuda", 0)
    criterion = Poly1FocalLoss(reduction="mean", **CONFIG)
    res = {"device": torch.cuda.get_device_name(0), "config": CONFIG, "reduction": "mean", "hbm_peak_bytes_per_s": HBM_PEAK,
           "step_bytes_per_element": STEP_BYTES_PER_ELEMENT, "sizes": []}
    for n in a.sizes:
        fused = measure(lambda x, y: criterion(x, y)[0], n, a.repeat, dev)
        plain = measure(lambda x, y: composite_mean(x, y, **CONFIG), n, a.repeat, dev)
        res["sizes"].append({"n": n, "fused": fused, "pytorch_composite": plain})
        print(f"n={n}: fused {fused['us_median']:.1f} us in {fused['launches']} launches, PyTorch composite {plain['us_median']:.1f} us in "
              f"{plain['launches']} launches" + (f"; fused at {100 * fused['hbm_fraction']:.0f} % of the HBM peak" if "hbm_fraction" in fused else ""),
              flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
