#!/usr/bin/env python3
"""``optim.ClipAdamW`` against what ``trainer.finish_step`` composes (``scaler.unscale_``, ``clip_grad_norm_(1.0)``, ``scaler.step(AdamW)``,
``scaler.update()``): the optimiser step alone on the same gradients, and one whole training step of ``pointstowood_amd.train.Net`` with
``--fused_step`` on and off - under float16 and bfloat16 autocast, in one process.

    python tools/fused_step_bench.py [--repeat 10] [--only optimizer|step] [--amp fp16 bf16] [--commit <hash>]
                                     [--out profiles/fused_step_bench.json]

The method is ``tools/bn_max_io_bench.py``'s (``train.Net`` at C = 32, an 8 x 16 384-point batch; device events around the measured
statements; two warm-up steps per route, then ``--repeat`` steps that alternate between the routes and rotate over three copies of the
inputs; median, minimum and maximum).  Routes:

    optimizer  clip_adamw     ClipAdamW.step() on the 158 parameter tensors
               foreach        finish_step with torch.optim.AdamW as the trainer builds it (foreach at torch's default)
               fused_adamw    finish_step with torch.optim.AdamW(fused=True)
               the gradients (three fixed sets, scaled by 512 under fp16) are put in place before the first event: unscale_ and the clip
               change them in place, so every step gets fresh copies.
    step       fused_step / plain: zero_grad, forward, loss, backward and the optimiser step as trainer.SemanticTraining runs them

``verdict`` applies the rule fixed before the measurement: ``--fused_step`` is recommended for speed only if the whole step's gain over
the plain route exceeds the larger of the two routes' min .. max spreads.  The default stays off either way: the roundings differ from
torch's.  ``bytes_per_element_derived`` are computed from the operations, not measured.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import synthetic_voxels, train  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402
from pointstowood_amd.optim import ClipAdamW  # noqa: E402
from pointstowood_amd.trainer import AMP_DTYPES, finish_step  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES  # noqa: E402
from tools.net_train_bench import B, C, N, _Batch, measured  # noqa: E402

OPT_ROUTES = ("clip_adamw", "foreach", "fused_adamw")
STEP_ROUTES = ("fused_step", "plain")
# g read twice, p, m and v read and written once; the composition: unscale 8, norm 4, clip 8 and some ten AdamW passes of 8 to 12
BYTES_DERIVED = {"clip_adamw": 32, "foreach_composition_order_of": 100}


def _optimizer(route, params, amp):
    if route in ("clip_adamw", "fused_step"):
        return ClipAdamW(params, lr=1e-4, weight_decay=1e-2, max_norm=1.0, loss_scale=512.0 if amp == "fp16" else None), None
    kw = {"fused": True} if route == "fused_adamw" else {}
    return (torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-2, **kw),
            torch.amp.GradScaler("cuda", init_scale=512, enabled=amp == "fp16"))


def run_optimizer(amp, repeat, dev):
    torch.manual_seed(0)
    base = train.Net(1, C).to(dev)
    shapes = [p.shape for p in base.parameters()]
    gen = torch.Generator(device=dev).manual_seed(1)
    scale = 512.0 if amp == "fp16" else 1.0
    sets = [[torch.randn(s, device=dev, generator=gen) * (1e-3 * scale) for s in shapes] for _ in range(COPIES)]
    holders = {r: torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in base.parameters()]) for r in OPT_ROUTES}
    state = {r: _optimizer(r, list(holders[r].parameters()), amp) for r in OPT_ROUTES}
    for _, scaler in state.values():
        if scaler is not None:
            scaler.scale(torch.zeros((), device=dev))             # (creates the scale tensor outside the timing)

    def step(route, grads):
        holder, (optimizer, scaler) = holders[route], state[route]
        for p, g in zip(holder.parameters(), grads):
            p.grad = g.clone()

        def fn():
            if scaler is None:
                optimizer.step()
            else:
                finish_step(holder, optimizer, scaler, amp)
            return None, None
        return measured(fn)

    _, r = alternate({k: k for k in OPT_ROUTES}, step, sets, repeat)
    r.update(tensors=len(shapes), elements=sum(s.numel() for s in shapes), repeat=repeat, rotating_inputs=COPIES)
    for k in ("foreach", "fused_adamw"):
        r[f"time_ratio_{k}_over_clip_adamw"] = r[k]["ms_median"] / r["clip_adamw"]["ms_median"]
    r["clip_adamw_record"] = state["clip_adamw"][0].read()
    return r


def run_step(amp, repeat, dev):
    sets = []
    for s in range(COPIES):
        b = synthetic_voxels.collate([synthetic_voxels.uniform_voxel(2.0, N, 1000 * s + i, reflectance=True) for i in range(B)])
        d = _Batch()
        d.pos, d.batch, d.reflectance, d.sf = (b[k].to(dev) for k in ("pos", "batch", "reflectance", "sf"))
        d.y = (torch.rand(B * N, generator=torch.Generator().manual_seed(s)) < 0.3).float().to(dev)
        sets.append(d)
    torch.manual_seed(0)
    base = train.Net(1, C).to(dev).train()
    nets = {route: copy.deepcopy(base) for route in STEP_ROUTES}
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    state = {r: _optimizer(r, [p for p in nets[r].parameters() if p.requires_grad], amp) for r in STEP_ROUTES}

    def step(route, d):
        net, (optimizer, scaler) = nets[route], state[route]

        def fn():
            optimizer.zero_grad()
            with torch.autocast("cuda", dtype=AMP_DTYPES[amp]):
                outputs = net(d)
                loss, _ = criterion(outputs, d.y)
            if scaler is None:
                optimizer.scale(loss).backward()
                optimizer.step()
            else:
                scaler.scale(loss).backward()
                finish_step(net, optimizer, scaler, amp)
            return outputs.detach(), None
        return measured(fn)

    _, r = alternate({k: k for k in STEP_ROUTES}, step, sets, repeat)
    r.update(voxels=B, points_per_voxel=N, C=C, repeat=repeat, rotating_inputs=COPIES,
             note="the nets start from the same weights and draw different random samples: their logits are not compared")
    f, p = r["fused_step"], r["plain"]
    gain, spread = p["ms_median"] - f["ms_median"], max(f["ms_max"] - f["ms_min"], p["ms_max"] - p["ms_min"])
    r["verdict"] = {"gain_ms_fused_step_over_plain": gain, "larger_min_max_spread_ms": spread, "recommend_for_speed": bool(gain > spread)}
    r["fused_step_record"] = state["fused_step"][0].read()
    return r


def _line(what, k, v):
    print(f"{what} {k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f}..{v['ms_max']:.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["optimizer", "step"], default=None)
    ap.add_argument("--amp", nargs="*", choices=list(AMP_DTYPES), default=list(AMP_DTYPES))
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fused_step_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "torch": torch.__version__,
           "bytes_per_element_derived": BYTES_DERIVED, "optimizer": {}, "step": {}}
    for amp in a.amp:
        if a.only in (None, "optimizer"):
            r = res["optimizer"][amp] = run_optimizer(amp, a.repeat, dev)
            for k in OPT_ROUTES:
                _line(f"{amp} optimiser step, {r['tensors']} tensors, {r['elements']} elements", k, r[k])
            torch.cuda.empty_cache()
        if a.only in (None, "step"):
            r = res["step"][amp] = run_step(amp, a.repeat, dev)
            for k in STEP_ROUTES:
                _line(f"{amp} step {B} x {N}, C = {C}", k, r[k])
            torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
