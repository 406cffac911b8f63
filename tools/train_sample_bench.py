#!/usr/bin/env python3
"""The training sample of ``train.SAModule``: the reference's host draw (``random_sample(n).to(device)``: a CPU ``randperm``, a CPU sort
and a synchronous copy) beside ``ops.random_subset`` (``train.DeviceSampler``), per level and as part of one whole training step.

    python tools/train_sample_bench.py [--repeat 10] [--commit <hash>] [--out profiles/train_sample_bench.json]

1. Per level of an 8 x 16 384-point batch (n = 131 072, 65 536, 32 768, k = n // 2): the host route by a host clock that ends in a
   device synchronise; the device route by device events and by the same host clock.
2. One whole training step of ``train.Net`` (C = 32, fused, autocast, ``Poly1FocalLoss``, ``GradScaler``, clip, AdamW: the step of
   ``tools/net_train_bench.py``) with ``net.sampler = None`` beside ``net.sampler = DeviceSampler(seed)``, on the SAME net: a host clock
   around a step that ends in a device synchronise - what is looked for is host time leaking into the step, and an enqueue time
   would not show it.

One process, ``torch.set_num_threads(1)`` (``train.py``'s default ``--num_procs 1``; recorded beside the CPU model).  Two warm-up calls
per route, then ``--repeat`` calls that alternate between the routes and rotate over three batches; median, minimum and maximum.  No
ratio is asserted: what is measured is what is written.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import ops, synthetic_voxels, train  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402

B, N, C, COPIES, SEED = 8, 16384, 32, 3, 141190
LEVELS = (B * N, B * N // 2, B * N // 4)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def host_clock(fn):
    """fn() from an idle device to an idle device, in host milliseconds"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def run_levels(repeat, dev):
    out = {}
    for n in LEVELS:
        routes = {"host": lambda i: train.SAModule.random_sample(None, n).to(dev),      # the draw itself (it does not use its module)
                  "device": lambda i: ops.random_subset(n, n // 2, SEED, counter=(i, 1), device=dev)}
        times = {"host": [], "device": [], "device_events": []}
        for i in range(2 + repeat):
            for name, fn in routes.items():
                ms = host_clock(lambda: fn(i))
                if i >= 2:
                    times[name].append(ms)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            routes["device"](i)
            b.record()
            b.synchronize()
            if i >= 2:
                times["device_events"].append(a.elapsed_time(b))
        out[str(n)] = {"n": n, "k": n // 2, **{k: summary(v) for k, v in times.items()}}
    return out


class _Batch:
    pass


def run_step(repeat, dev):
    sets = []
    for s in range(COPIES):
        b = synthetic_voxels.collate([synthetic_voxels.uniform_voxel(2.0, N, 1000 * s + i, reflectance=True) for i in range(B)])
        d = _Batch()
        d.pos, d.batch, d.reflectance, d.sf = (b[k].to(dev) for k in ("pos", "batch", "reflectance", "sf"))
        d.y = (torch.rand(B * N, generator=torch.Generator().manual_seed(s)) < 0.3).float().to(dev)
        sets.append(d)
    torch.manual_seed(0)
    net = train.Net(1, C).to(dev).train()
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    optimizer, scaler = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2), torch.amp.GradScaler("cuda", init_scale=512)
    samplers = {"host_sample": None, "device_sample": train.DeviceSampler(SEED)}

    def step(route, d):
        net.sampler = samplers[route]
        optimizer.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            outputs = net(d)
            loss, _ = criterion(outputs, d.y)
        scaler.scale(loss).backward()
        scaler.unscale_(optimizer)
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
        scaler.step(optimizer)
        scaler.update()

    times = {k: [] for k in samplers}
    for i in range(2 + repeat):
        for route in samplers:                                  # the routes alternate, the inputs rotate
            ms = host_clock(lambda: step(route, sets[i % COPIES]))
            if i >= 2:
                times[route].append(ms)
    r = {k: summary(v) for k, v in times.items()}
    spread = max(v["ms_max"] - v["ms_min"] for v in r.values())
    gain = r["host_sample"]["ms_median"] - r["device_sample"]["ms_median"]
    r.update(voxels=B, points_per_voxel=N, C=C, clock="host clock around a step that ends in torch.cuda.synchronize()",
             median_gain_ms=gain, larger_spread_ms=spread, gain_exceeds_spread=gain > spread,
             note="one net, the two routes alternating: the weights move on between the steps, the shapes do not")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["levels", "step"], default=None)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_sample_bench needs an MI355X: a timing taken anywhere else says nothing")
    torch.set_num_threads(1)
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "repeat": a.repeat,
           "warmups": 2, "rotating_inputs": COPIES, "host_threads": torch.get_num_threads(), "cpu": cpu_model(), "seed": SEED}
    if a.only != "step":
        r = res["levels"] = run_levels(a.repeat, dev)
        for n, v in r.items():
            print(f"n = {n}: host {v['host']['ms_median']:.3f} ms ({v['host']['ms_min']:.3f}..{v['host']['ms_max']:.3f}), device "
                  f"{v['device']['ms_median']:.3f} ms ({v['device']['ms_min']:.3f}..{v['device']['ms_max']:.3f}) by the host clock, "
                  f"{v['device_events']['ms_median']:.3f} ms ({v['device_events']['ms_min']:.3f}..{v['device_events']['ms_max']:.3f}) "
                  "by device events", flush=True)
    if a.only != "levels":
        r = res["step"] = run_step(a.repeat, dev)
        for k in ("host_sample", "device_sample"):
            print(f"step {B} x {N}, C = {C}, {k}: {r[k]['ms_median']:.2f} ms ({r[k]['ms_min']:.2f}..{r[k]['ms_max']:.2f})", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
