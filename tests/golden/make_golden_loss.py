#!/usr/bin/env python3
"""Generate the loss fixtures in tests/golden/loss/ FROM THE REFERENCE's unmodified ``src.loss.Poly1FocalLoss``, on the CPU.

Run by hand in the authoring container, never by a test:

    python tests/golden/make_golden_loss.py --reference /path/to/PointsToWood

  inputs.npz            logits [4116] float32 (17 edge logits, then 4099 draws of randn * 4), labels (Bernoulli(0.3)), labels_soft
                        (uniform in [0, 1]: label smoothing feeds non-binary targets), weight_n [4116], weight_1 [1], seed
  <config>__<labels>.npz  for every configuration of tests/loss_ref.CONFIGS and both label vectors, from the reference's class:
                        loss64 / grad64 = the per-element loss (reduction="none") and the gradient of its sum with the inputs in
                        float64, loss32 / grad32 = the same in float32, reduced64 / reduced32 = what the class returns with the
                        configuration's own reduction ("none": the per-element loss again) and rgrad64 / rgrad32 = the gradient
                        of that (of its sum for "none")
  configs.json          the constructor arguments of every configuration
  noise.json            per case the largest |float32 - float64| of the reference itself, for loss and for gradient
  manifest.json         sha256 of every file above

The reference's source never enters this repository; only these data vectors do.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import shutil
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loss")
sys.path.insert(0, os.path.dirname(HERE))
import loss_ref as R  # noqa: E402


def run(cls, logits, labels, weight, kwargs, dtype):
    """(loss, gradient of its sum, reduced value, gradient of the reduced value) of the reference's class in ``dtype``."""
    y = torch.from_numpy(labels).to(dtype)
    w = None if weight is None else torch.from_numpy(weight).to(dtype)
    out = []
    for reduction in ("none", kwargs["reduction"]):
        x = torch.from_numpy(logits).to(dtype).requires_grad_()
        loss, gamma = cls(**dict(kwargs, reduction=reduction, weight=w))(x, y)
        assert gamma == kwargs["gamma"]
        loss.sum().backward()
        out += [loss.detach().numpy(), x.grad.numpy()]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds pointstowood/src/loss.py)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.reference), "pointstowood"))
    from src.loss import Poly1FocalLoss
    torch.manual_seed(0)
    torch.set_num_threads(1)
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    inputs = R.make_inputs()
    np.savez_compressed(os.path.join(OUT, "inputs.npz"), seed=np.int64(R.FIXTURE_SEED), **inputs)
    noise = {}
    for config in R.CONFIGS:
        for kind in R.LABEL_KINDS:
            logits, labels, weight, kwargs = R.case_tensors(inputs, config, kind)
            l64, g64, r64, rg64 = run(Poly1FocalLoss, logits, labels, weight, kwargs, torch.float64)
            l32, g32, r32, rg32 = run(Poly1FocalLoss, logits, labels, weight, kwargs, torch.float32)
            assert np.isfinite(l64).all() and np.isfinite(g64).all() and np.isfinite(l32).all() and np.isfinite(g32).all()
            name = f"{config}__{kind}"
            np.savez_compressed(os.path.join(OUT, name + ".npz"), loss64=l64, grad64=g64, loss32=l32, grad32=g32, reduced64=r64,
                                reduced32=r32, rgrad64=rg64, rgrad32=rg32)
            noise[name] = {"loss": float(np.abs(l32.astype(np.float64) - l64).max()),
                           "grad": float(np.abs(g32.astype(np.float64) - g64).max())}
            print(name, noise[name])
    with open(os.path.join(OUT, "configs.json"), "w") as f:
        json.dump({k: {"kwargs": kw, "weight": w} for k, (kw, w) in R.CONFIGS.items()}, f, indent=1, sort_keys=True)
    with open(os.path.join(OUT, "noise.json"), "w") as f:
        json.dump({"what": "largest |float32 - float64| of the reference's Poly1FocalLoss on the CPU, per-element loss and "
                           "gradient of the summed loss", "torch": torch.__version__, "cases": noise}, f, indent=1, sort_keys=True)
    man = {}
    for f in sorted(os.listdir(OUT)):
        if f != "manifest.json":
            man[f] = hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()
            assert os.path.getsize(os.path.join(OUT, f)) < 256 << 10, f
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
