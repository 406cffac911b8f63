#!/usr/bin/env python3
"""The trainable ``pointstowood_amd.train.Net``: its fused head operator beside the two compositions it can replace, and one whole
training step with ``Net.fused = True`` beside ``False``, in one process.

    python tools/net_train_bench.py [--repeat 10] [--commit <hash>] [--out profiles/net_train_bench.json]

1. ``ops.bn_relu_rowdot(z, bn, w, b)`` at z [131 072, 512] (the head of an 8 x 16 384-point batch at C = 32) against the plain
   composition ``F.linear(torch.relu(bn(z)), w, b)`` and against ``F.linear(ops.bn_chain(z, [(bn, True)]), w, b)``: forward + backward
   of ``sum(out * g)`` with gradients to z and every parameter.
2. One whole step on 8 x 16 384 synthetic points (uniform cubes of 2 m with reflectance), C = 32, as ``trainer.py:169-186`` takes it:
   the forward under autocast, ``Poly1FocalLoss``, ``GradScaler(init_scale=512)``, ``clip_grad_norm_`` and AdamW - the sampling, the
   searches and the optimiser included, they are the same in both routes.

Timed with device events around the whole step; the method is ``tools/fp_train_bench.py``'s: two warm-up steps per route, then
``--repeat`` steps that alternate between the routes and rotate over three copies of the inputs; median, minimum and maximum.
``peak_bytes`` is ``torch.cuda.max_memory_allocated`` over a step minus what was allocated before it.  No ratio is asserted: what is
measured is what is written.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import ops, synthetic_voxels, train  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES, rel_l2  # noqa: E402

B, N, C = 8, 16384, 32


def measured(fn):
    """One call of fn() between two device events: (ms, peak bytes above what was allocated before, fn's two results)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out, grad = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out, grad


def run_head(repeat, dev):
    M, W = B * N, 16 * C
    gen = torch.Generator(device=dev).manual_seed(5)
    sets = [dict(z=torch.randn(M, W, device=dev, generator=gen), g=torch.randn(M, device=dev, generator=gen)) for _ in range(COPIES)]
    torch.manual_seed(0)
    mods = {}
    for route in ("fused", "plain", "bn_chain"):
        bn, conv2 = torch.nn.BatchNorm1d(W).to(dev).train(), torch.nn.Conv1d(W, 1, 1).to(dev)
        if mods:
            conv2.load_state_dict(mods["fused"][1].state_dict())
        mods[route] = (bn, conv2)

    def step(route, d):
        bn, conv2 = mods[route]
        bn.zero_grad(set_to_none=True), conv2.zero_grad(set_to_none=True)
        z = d["z"].detach().requires_grad_()

        def fn():
            if route == "fused":
                out = ops.bn_relu_rowdot(z, bn, conv2.weight, conv2.bias)
            else:
                u = torch.relu(bn(z)) if route == "plain" else ops.bn_chain(z, [(bn, True)])
                out = F.linear(u, conv2.weight[:, :, 0], conv2.bias)[:, 0]
            (out * d["g"]).sum().backward()
            return out.detach(), z.grad
        return measured(fn)

    first, r = alternate({k: k for k in mods}, step, sets, repeat)
    r.update(M=M, C=W, repeat=repeat, rotating_inputs=COPIES, activation_bytes_derived=M * W * 4,
             passes_derived={"bn_chain": {"forward": 4, "backward": 7}, "fused": {"forward": 2, "backward": 3}})
    for other in ("plain", "bn_chain"):
        r[f"time_ratio_{other}_over_fused"] = r[other]["ms_median"] / r["fused"]["ms_median"]
        r[f"out_rel_l2_vs_{other}"] = rel_l2(first["fused"][2], first[other][2])
        r[f"grad_z_rel_l2_vs_{other}"] = rel_l2(first["fused"][3], first[other][3])
    return r


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
    nets = {"fused": train.Net(1, C).to(dev).train()}
    nets["plain"] = copy.deepcopy(nets["fused"])
    nets["plain"].fused = False
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    state = {k: (torch.optim.AdamW(n.parameters(), lr=1e-4, weight_decay=1e-2), torch.amp.GradScaler("cuda", init_scale=512))
             for k, n in nets.items()}

    def step(route, d):
        net, (optimizer, scaler) = nets[route], state[route]

        def fn():
            optimizer.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16):
                outputs = net(d)
                loss, _ = criterion(outputs, d.y)
            scaler.scale(loss).backward()
            scaler.unscale_(optimizer)
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
            grad = net.conv1.weight.grad.detach().clone()
            scaler.step(optimizer)
            scaler.update()
            return outputs.detach(), grad
        return measured(fn)

    first, r = alternate({k: k for k in nets}, step, sets, repeat)
    r.update(voxels=B, points_per_voxel=N, C=C, repeat=repeat, rotating_inputs=COPIES,
             time_ratio_plain_over_fused=r["plain"]["ms_median"] / r["fused"]["ms_median"],
             peak_ratio_plain_over_fused=r["plain"]["peak_bytes"] / r["fused"]["peak_bytes"],
             note="the two nets start from the same weights and draw different random samples: their logits are not compared")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["head", "step"], default=None)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("net_train_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit}
    if a.only != "step":
        r = res["head"] = run_head(a.repeat, dev)
        for k in ("fused", "plain", "bn_chain"):
            print(f"head [{r['M']}, {r['C']}] {k}: {r[k]['ms_median']:.2f} ms ({r[k]['ms_min']:.2f}..{r[k]['ms_max']:.2f}), "
                  f"{r[k]['peak_bytes'] / 2**20:.0f} MiB", flush=True)
        torch.cuda.empty_cache()
    if a.only != "head":
        r = res["step"] = run_step(a.repeat, dev)
        for k in ("fused", "plain"):
            print(f"step {B} x {N}, C = {C}, Net.fused = {k == 'fused'}: {r[k]['ms_median']:.1f} ms ({r[k]['ms_min']:.1f}..{r[k]['ms_max']:.1f}), "
                  f"{r[k]['peak_bytes'] / 2**20:.0f} MiB", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
