#!/usr/bin/env python3
"""The training feed per batch: ``feed.TrainingFeed`` (device-resident set, one ``p2w_train_feed`` call, augmentation on) beside the host
route the package offered for labelled voxels before it - ``evaluate.LabelledVoxelDataset.__getitem__`` per voxel,
``Batch.from_data_list`` and ``.to(device)``, ``num_workers=0``, no augmentation (that route has none) - and both as a share of a whole
training step of ``train.Net`` (C = 32) on the same batch.

    python tools/train_feed_bench.py [--repeat 10] [--commit <hash>] [--out profiles/train_feed_bench.json]

8 voxels of 16 384 synthetic points per batch (uniform 2 m cubes at plot coordinates, with reflectance and labels), a set of 24 voxels.
Timed with device events around each call (an idle device waits for the host, so host time is inside the interval); the method is
``tools/net_train_bench.py``'s: two warm-up calls per route, then ``--repeat`` calls that alternate between the routes and rotate over
three batches; median, minimum and maximum.  The per-epoch plan upload of the feed (48 bytes per voxel) is outside the per-batch
figure.  No ratio is asserted: what is measured is what is written.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import feed as F, synthetic_voxels, train  # noqa: E402
from pointstowood_amd.data import Batch  # noqa: E402
from pointstowood_amd.evaluate import LabelledVoxelDataset  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES  # noqa: E402
from tools.net_train_bench import measured  # noqa: E402

B, N, C, V = 8, 16384, 32, 24


def voxels():
    out = []
    for i in range(V):
        p, refl = synthetic_voxels.uniform_points(2.0, N, 1000 + i, reflectance=True, offset=(300.0 + 2 * i, 310.0, 20.0))
        y = (torch.rand(N, generator=torch.Generator().manual_seed(i)) < 0.3).float()
        out.append(torch.cat([p, refl[:, None], y[:, None]], 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_feed_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    vox = voxels()
    feed = F.TrainingFeed(F.TrainingSet(vox, dev), B, shuffle=False, augmentation=True, mode="train", seed=0)
    feed.set_epoch(1)
    plan = F.plan_to_device(feed.plan(), dev)
    host_set = LabelledVoxelDataset(vox)
    sets = [list(range(B * s, B * s + B)) for s in range(COPIES)]

    torch.manual_seed(0)
    net = train.Net(1, C).to(dev).train()
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    optimizer, scaler = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2), torch.amp.GradScaler("cuda", init_scale=512)
    ready = {tuple(ids): feed.batch(ids, plan) for ids in sets}

    def run(route, ids):
        def fn():
            if route == "feed":
                d = feed.batch(ids, plan)
                return d.pos, d.sf
            if route == "host":
                d = Batch.from_data_list([host_set[i] for i in ids]).to(dev)
                return d.pos, d.sf
            d = ready[tuple(ids)]
            optimizer.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16):
                outputs = net(d)
                loss, _ = criterion(outputs, d.y)
            scaler.scale(loss).backward()
            scaler.unscale_(optimizer)
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
            scaler.step(optimizer)
            scaler.update()
            return outputs.detach(), loss.detach()
        return measured(fn)

    _, r = alternate({k: k for k in ("feed", "host", "step")}, run, sets, a.repeat)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "voxels": B,
           "points_per_voxel": N, "C": C, "repeat": a.repeat, "rotating_inputs": COPIES, "host_threads": torch.get_num_threads(),
           "routes": {"feed": "TrainingFeed.batch: one upload, p2w_train_feed, augmentation on",
                      "host": "LabelledVoxelDataset.__getitem__ x 8 + Batch.from_data_list + .to(device), num_workers=0, no augmentation",
                      "step": "one training step of train.Net (fused) on a batch of the feed"}, **r}
    step = r["step"]["ms_median"]
    for k in ("feed", "host"):
        res[f"{k}_share_of_feed_plus_step"] = r[k]["ms_median"] / (r[k]["ms_median"] + step)
        print(f"{k}: {r[k]['ms_median']:.3f} ms ({r[k]['ms_min']:.3f}..{r[k]['ms_max']:.3f}) per {B} x {N}-point batch, "
              f"{100 * res[f'{k}_share_of_feed_plus_step']:.1f} % of feed + step", flush=True)
    print(f"step: {step:.1f} ms ({r['step']['ms_min']:.1f}..{r['step']['ms_max']:.1f})", flush=True)
    res["time_ratio_host_over_feed"] = r["host"]["ms_median"] / r["feed"]["ms_median"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
