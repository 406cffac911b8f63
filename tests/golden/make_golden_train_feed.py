#!/usr/bin/env python3
"""Generate the training-feed fixtures in tests/golden/train_feed/ FROM THE REFERENCE's unmodified ``src.augmentation.augmentations``
and ``src.cosine_scheduler.CosineAnnealingWarmupRestarts``, on the CPU.

Run by hand in the authoring container, never by a test:

    python tests/golden/make_golden_train_feed.py --reference /path/to/PointsToWood

  <case>.npz     pc [n, 5] float32 (x, y, z, reflectance, label) = the voxel file's content; the reference's draws re-derived by
                 re-seeding the global generator and drawing in its consumption order - u_refl, u_pos, then the per-point noise [n]
                 (only when it perturbs; zeros otherwise), then the angle uniforms u_angles [3] (only when it rotates; zeros
                 otherwise); and pos [n, 3], reflectance [n], y [n], sf = what ``augmentations`` followed by the arithmetic of
                 ``TrainingDataset.__getitem__`` (trainer.py:49-56, the same torch calls) returns
  cases.json     per case: mode, the global seed, n, refl_mode (0 keep, 1 silence, 2 perturb), rotate, offset
  edges.json     what ``augmentations`` does for draws exactly on and just below 0.25 and 0.5 (``torch.rand`` replaced by the values)
  tune_lr.json   the learning rates of the reference's scheduler with the --tune parameters of trainer.py:119-120 at num_epochs = 50,
                 over three cycles
  manifest.json  sha256 of every file above

Cases: the three reflectance branches x rotated or not, in both modes (in "test" the perturb interval keeps the reflectance), a rotated
voxel at plot coordinates (+300 m) and a rotated voxel near the origin.  The reference's source never enters this repository; only
these data vectors do.
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
OUT = os.path.join(HERE, "train_feed")
ROOT = os.path.dirname(os.path.dirname(HERE))


def voxel(n, seed, offset):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * 2.0 + torch.tensor(offset, dtype=torch.float32)
    refl = torch.rand(n, generator=g) * 2 - 1
    label = (torch.rand(n, generator=g) < 0.3).float()
    return torch.cat([xyz, refl[:, None], label[:, None]], dim=1)


def classes(seed):
    torch.manual_seed(seed)
    u_refl, u_pos = torch.rand(1), torch.rand(1)
    return (0 if u_refl < 0.25 else 1 if u_refl < 0.5 else 2), bool(u_pos < 0.25)


def find_seed(want_refl, want_rot, start):
    s = start
    while classes(s) != (want_refl, want_rot):
        s += 1
    return s


def item(augmentations, pc, mode, seed):
    """The reference's item and its draws."""
    pos, refl, y = pc[:, :3].clone(), pc[:, 3].clone(), pc[:, 4].clone()
    torch.manual_seed(seed)
    pos, refl, y = augmentations(pos, refl, y, mode)
    shift = torch.mean(pos[:, :3], axis=0)                              # trainer.py:54-56
    pos = pos - shift
    sf = torch.sqrt((pos ** 2).sum(dim=1)).max()
    torch.manual_seed(seed)                                             # the draws, in the order augmentations() consumes them
    u_refl, u_pos = torch.rand(1), torch.rand(1)
    n = pc.shape[0]
    refl_mode = 1 if u_refl < 0.25 else 2 if (mode == "train" and u_refl < 0.5) else 0
    noise = torch.normal(mean=0.0, std=0.1, size=(n,)) if refl_mode == 2 else torch.zeros(n)
    rotate = bool(u_pos < 0.25)
    u_angles = torch.rand(3) if rotate else torch.zeros(3)
    if refl_mode == 2:
        assert torch.equal(refl, pc[:, 3] + noise)
    arrays = dict(pc=pc.numpy(), u_refl=u_refl.numpy(), u_pos=u_pos.numpy(), noise=noise.numpy(), u_angles=u_angles.numpy(),
                  pos=pos.numpy(), reflectance=refl.numpy(), y=y.numpy(), sf=sf.numpy())
    return arrays, refl_mode, rotate


def edges(augmentations):
    import src.augmentation as A
    real = torch.rand
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
    rows = []
    pc = voxel(64, 99, (0.0, 0.0, 0.0))
    for mode in ("train", "test"):
        for u_refl in (0.25, below(0.25), 0.5, below(0.5)):
            for u_pos in (0.25, below(0.25)):
                queue = [torch.tensor([u_refl], dtype=torch.float32), torch.tensor([u_pos], dtype=torch.float32)]
                A.torch.rand = lambda *size, **kw: queue.pop(0) if queue and tuple(size) == (1,) else real(*size, **kw)
                try:
                    pos, refl, _ = augmentations(pc[:, :3].clone(), pc[:, 3].clone(), pc[:, 4].clone(), mode)
                finally:
                    A.torch.rand = real
                silenced = bool((refl == 0).all())
                rows.append({"mode": mode, "u_refl": u_refl, "u_pos": u_pos, "rotate": not torch.equal(pos, pc[:, :3]),
                             "refl_mode": 1 if silenced else 0 if torch.equal(refl, pc[:, 3]) else 2})
    return rows


def tune_lr(cls):
    num_epochs = 50
    model = torch.nn.Linear(2, 1)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-6, weight_decay=1e-2)
    kw = dict(first_cycle_steps=num_epochs // 5, cycle_mult=1.0, max_lr=1e-6, min_lr=1e-8, warmup_steps=5, gamma=0.5)
    sched = cls(opt, **kw)
    lrs = [opt.param_groups[0]["lr"]]
    for _ in range(3 * kw["first_cycle_steps"] + 2):
        opt.step()
        sched.step()
        lrs.append(opt.param_groups[0]["lr"])
    return {"num_epochs": num_epochs, "kwargs": kw, "lr": lrs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds pointstowood/src/augmentation.py)")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)                                            # the stubs import oracle.ops
    sys.path.insert(0, os.path.join(ROOT, "oracle", "stubs"))
    sys.path.insert(0, os.path.join(os.path.abspath(args.reference), "pointstowood"))
    from src.augmentation import augmentations
    from src.cosine_scheduler import CosineAnnealingWarmupRestarts
    torch.set_num_threads(1)
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    cases, k = {}, 0
    plan = [(mode, r, rot, (10.0, 20.0, 5.0)) for mode in ("train", "test") for r in (0, 1, 2) for rot in (False, True)]
    plan += [("train", 2, True, (300.0, 310.0, 20.0)), ("train", 2, True, (-1.0, -1.0, -1.0))]
    names = {0: "silence", 1: "perturb", 2: "keep"}
    for mode, r, rot, offset in plan:
        seed = find_seed(r, rot, 1000 * (k + 1))
        n = 257 + 131 * k
        pc = voxel(n, 7 + k, offset)
        arrays, refl_mode, rotate = item(augmentations, pc, mode, seed)
        assert rotate == rot and refl_mode == {0: 1, 1: 2 if mode == "train" else 0, 2: 0}[r]
        name = f"{mode}_{names[r]}_{'rot' if rot else 'norot'}" if k < 12 else ("plot300" if k == 12 else "origin")
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
        cases[name] = {"mode": mode, "seed": seed, "n": n, "refl_mode": refl_mode, "rotate": rotate, "offset": list(offset)}
        print(name, cases[name])
        k += 1
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump({"torch": torch.__version__, "cases": cases}, f, indent=1, sort_keys=True)
    with open(os.path.join(OUT, "edges.json"), "w") as f:
        json.dump(edges(augmentations), f, indent=1)
    with open(os.path.join(OUT, "tune_lr.json"), "w") as f:
        json.dump(tune_lr(CosineAnnealingWarmupRestarts), f, indent=1)
    man = {}
    for f in sorted(os.listdir(OUT)):
        man[f] = hashlib.sha256(open(os.path.join(OUT, f), "rb").read()).hexdigest()
        assert os.path.getsize(os.path.join(OUT, f)) < 256 << 10, f
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
