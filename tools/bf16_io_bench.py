#!/usr/bin/env python3
"""bfloat16 autocast through the fused training operators: ``ops.half_io`` on against off on bfloat16 tensors, with float16 ``half_io``
on as the sibling, for the four operator families that take a 16-bit tensor as it is, each alone, and for one whole training step of
``pointstowood_amd.train.Net``, in one process; and what one step costs in accuracy under either autocast dtype.

    python tools/bf16_io_bench.py [--repeat 10] [--only ops|step|accuracy] [--commit <hash>] [--parent-json FILE ...]
                                  [--out profiles/bf16_io_bench.json]

The method and the shapes are ``tools/half_io_bench.py``'s (an 8 x 16 384-point batch at C = 32; device events; two warm-up steps per
route, then ``--repeat`` steps that alternate between the routes and rotate over three copies of the inputs; median, minimum and
maximum; ``peak_bytes`` above what was allocated before the step).  Routes:

    bf16_on    bfloat16 autocast, ``half_io`` on: the bfloat16 kernels (P2W_BF16)
    bf16_off   bfloat16 autocast, ``half_io`` off: every operator casts to fp32 first - the route bfloat16 took before
    fp16_on    float16 autocast, ``half_io`` on

On a tree whose library has no P2W_BF16 (``_lib.BF16`` absent) only the whole step runs, as route ``bf16_parent``: bfloat16 can only
take the cast-first route there.  That run, in a process of its own, is the time the new code is compared against: write it with
``--out``, and give the file to the run on the new tree as ``--parent-json`` (once per parent process), which copies its ``commit`` and
``step`` into the list ``step_parent_commit`` of its own output - how ``profiles/bf16_io_bench.json`` is put together.  The whole step is
the trainer's: float16 with ``GradScaler(512)``; bfloat16 with the scaler disabled and the clip's norm read once (trainer.finish_step).

``--only accuracy``: one step of ``train.Net`` at C = 8 on two voxels of 600 and 200 points (the inputs, weights and injected samples
of tests/test_gpu_train_net.py) under float16 and under bfloat16 autocast, judged against the float64 composition of
tests/net_train_ref.py: relative L2 of the logits, and the median and the maximum over the parameter gradients whose true value is
not zero.  A recorded fact for whoever chooses a mode, not a gate: the error is the GEMMs' own.  No ratio is asserted anywhere.
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import _lib, ops, synthetic_voxels, train  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES  # noqa: E402
from tools.net_train_bench import B, C, N, _Batch, measured  # noqa: E402

HAS_BF16 = hasattr(_lib, "BF16")
BF, HALF = torch.bfloat16, torch.float16
# route -> (autocast dtype, ops.half_io)
ROUTES = {"bf16_on": (BF, True), "bf16_off": (BF, False), "fp16_on": (HALF, True)} if HAS_BF16 else {"bf16_parent": (BF, True)}


class _switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old, ops.half_io = ops.half_io, self.value

    def __exit__(self, *a):
        ops.half_io = self.old


def _bn(width, dev):
    return torch.nn.BatchNorm1d(width).to(dev).train()


def _dw(width, dev):
    return torch.nn.Conv1d(width, width, 1, groups=width).to(dev)


def operator_families(dev):
    """name -> (shape, make(): modules, call(z, modules, dtype) -> out)."""
    n_dst, k = B * N // 2, 32
    index = torch.arange(n_dst, device=dev).repeat_interleave(k)
    return {
        "bn_chain": ((B * N // 2, 16 * C), lambda: [_bn(16 * C, dev), _bn(16 * C, dev), _bn(16 * C, dev), _dw(16 * C, dev)],
                     lambda z, m, dt: ops.bn_chain(z, [(m[0], True), (m[1], True), (m[2], True, m[3])], out_dtype=dt)),
        "relu_bn": ((B * N, 8 * C), lambda: [_bn(8 * C, dev)], lambda z, m, dt: ops.relu_bn(z, m[0], out_dtype=dt)),
        "bn_relu_rowdot": ((B * N, 16 * C), lambda: [_bn(16 * C, dev), torch.nn.Conv1d(16 * C, 1, 1).to(dev)],
                           lambda z, m, dt: ops.bn_relu_rowdot(z, m[0], m[1].weight, m[1].bias)),
        "scatter_max": ((n_dst * k, 4 * C), lambda: [], lambda z, m, dt: ops.scatter_max(z, index, dim=0, dim_size=n_dst)[0]),
    }


def _spread(r):
    return max(v["ms_max"] - v["ms_min"] for v in r.values() if isinstance(v, dict) and "ms_max" in v)


def run_operator(name, shape, make, call, repeat, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    sets32 = [torch.randn(shape, device=dev, generator=gen) for _ in range(COPIES)]
    sets = [{dt: z.to(dt) for dt in (BF, HALF)} for z in sets32]
    del sets32
    torch.manual_seed(0)
    base = make()
    mods = {route: copy.deepcopy(base) for route in ROUTES}          # the same weights on every route
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        like = call(sets[0][BF], copy.deepcopy(base), BF)
    cot32 = torch.randn(like.shape, device=dev, generator=gen)
    cot = {dt: cot32.to(dt) for dt in (BF, HALF, torch.float32)}        # cast once, outside the timed step
    del like, cot32

    def step(route, zs):
        dtype, on = ROUTES[route]
        for m in mods[route]:
            m.zero_grad(set_to_none=True)
        z = zs[dtype].detach().requires_grad_()

        def fn():
            with _switch(on), torch.autocast("cuda", dtype=dtype):
                out = call(z, mods[route], dtype)
            out.backward(cot[out.dtype])
            return out.detach(), z.grad
        return measured(fn)

    first, r = alternate({k: k for k in ROUTES}, step, sets, repeat)
    r["largest_min_max_spread_ms"] = _spread(r)
    r.update(shape=list(shape), repeat=repeat, rotating_inputs=COPIES)
    r["time_ratio_bf16_off_over_on"] = r["bf16_off"]["ms_median"] / r["bf16_on"]["ms_median"]
    r["time_ratio_fp16_on_over_bf16_on"] = r["fp16_on"]["ms_median"] / r["bf16_on"]["ms_median"]
    r["same_bits_bf16_on_off"] = bool(torch.equal(first["bf16_on"][2], first["bf16_off"][2]) and
                                      torch.equal(first["bf16_on"][3], first["bf16_off"][3]))
    return r


def run_step(repeat, dev):
    sets = []
    for s in range(COPIES):
        b = synthetic_voxels.collate([synthetic_voxels.uniform_voxel(2.0, N, 1000 * s + i, reflectance=True) for i in range(B)])
        d = _Batch()
        d.pos, d.batch, d.reflectance, d.sf = (b[k].to(dev) for k in ("pos", "batch", "reflectance", "sf"))
        d.y = (torch.rand(B * N, generator=torch.Generator().manual_seed(s)) < 0.3).float().to(dev)
        sets.append(d)
    torch.manual_seed(0)
    base = train.Net(1, C).to(dev).train()
    nets = {route: copy.deepcopy(base) for route in ROUTES}
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    state = {k: (torch.optim.AdamW(n.parameters(), lr=1e-4, weight_decay=1e-2),
                 torch.amp.GradScaler("cuda", init_scale=512, enabled=ROUTES[k][0] == HALF)) for k, n in nets.items()}

    def step(route, d):
        net, (optimizer, scaler), (dtype, on) = nets[route], state[route], ROUTES[route]

        def fn():
            with _switch(on):
                optimizer.zero_grad()
                with torch.autocast("cuda", dtype=dtype):
                    outputs = net(d)
                    loss, _ = criterion(outputs, d.y)
                scaler.scale(loss).backward()
                scaler.unscale_(optimizer)
                norm = torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
                grad = net.conv1.weight.grad.detach().clone()
                if dtype == HALF or math.isfinite(float(norm)):             # (the bfloat16 loop's one host read: trainer.finish_step)
                    scaler.step(optimizer)
                scaler.update()
            return outputs.detach(), grad
        return measured(fn)

    _, r = alternate({k: k for k in ROUTES}, step, sets, repeat)
    r["largest_min_max_spread_ms"] = _spread(r)
    r.update(voxels=B, points_per_voxel=N, C=C, repeat=repeat, rotating_inputs=COPIES,
             note="the nets start from the same weights and draw different random samples: their logits are not compared")
    if HAS_BF16:
        r["time_ratio_bf16_off_over_on"] = r["bf16_off"]["ms_median"] / r["bf16_on"]["ms_median"]
        r["peak_ratio_bf16_off_over_on"] = r["bf16_off"]["peak_bytes"] / r["bf16_on"]["peak_bytes"]
        r["time_ratio_fp16_on_over_bf16_on"] = r["fp16_on"]["ms_median"] / r["bf16_on"]["ms_median"]
    return r


def run_accuracy():
    """One step at C = 8 on tests/test_gpu_train_net.py's inputs under either autocast dtype against tests/net_train_ref.py in float64."""
    from tests import net_train_ref as R
    from tests import test_gpu_train_net as TN
    inp, sd = R.inputs(TN.SEED), R.state(TN.SEED)
    res, ref = {}, None
    for name, dtype in (("fp32", None), ("fp16", HALF), ("bf16", BF)):
        net, d = TN._net(sd), TN._data(inp)
        with TN._searches() as found:
            if dtype is None:
                logits = net(d)
            else:
                with torch.autocast("cuda", dtype=dtype):
                    logits = net(d)
        (logits.float() * inp["g"].cuda()).sum().backward()
        geo = [dict(idx=m.seen_idx.cpu(), edge_index=torch.stack([source, target]).cpu()) for m, (target, source) in zip(TN._sa(net), found)]
        grads = {k: p.grad.float().cpu() for k, p in net.named_parameters() if ".reflectanceyesno." not in k}
        if ref is None:                                                      # the float64 composition on the fp32 run's indices and edges
            l64, g64 = R.step(sd, inp, geo, torch.float64)
            norms = {k: float(v.norm()) for k, v in g64.items()}
            live = [k for k, n in norms.items() if n >= 1e-9 * statistics.median(norms.values())]
            ref = (l64, g64, live, geo)
        l64, g64, live, geo0 = ref
        same_geo = all(torch.equal(a[k], b[k]) for a, b in zip(geo, geo0) for k in ("idx", "edge_index"))
        errs = [R.rel_l2(grads[k], g64[k]) for k in live]
        res[name] = {"logits_rel_l2": R.rel_l2(logits.detach().float().cpu(), l64), "grad_rel_l2_median": statistics.median(errs),
                     "grad_rel_l2_max": max(errs), "gradients_judged": len(live), "same_samples_and_edges_as_fp32": bool(same_geo)}
        print(f"accuracy {name}: logits {res[name]['logits_rel_l2']:.3e}, gradients median {res[name]['grad_rel_l2_median']:.3e} "
              f"max {res[name]['grad_rel_l2_max']:.3e} of {len(live)}", flush=True)
    res["note"] = ("Net(1, 8), voxels of 600 and 200 points, tests/test_gpu_train_net.py's weights, samples and cotangent; relative L2 against "
                   "tests/net_train_ref.py in float64; gradients whose float64 norm is below 1e-9 of the median norm are left out")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["ops", "step", "accuracy"], default=None)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--parent-json", action="append", default=[], help="--out file of this tool's run on the parent commit's tree; repeatable")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_io_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "library_has_bf16": HAS_BF16,
           "routes": {k: [str(dt).split(".")[-1], on] for k, (dt, on) in ROUTES.items()}}
    if a.only in (None, "ops") and HAS_BF16:
        res["operators"] = {}
        for name, (shape, make, call) in operator_families(dev).items():
            r = res["operators"][name] = run_operator(name, shape, make, call, a.repeat, dev)
            for k in ROUTES:
                print(f"{name} {list(shape)} {k}: {r[k]['ms_median']:.2f} ms ({r[k]['ms_min']:.2f}..{r[k]['ms_max']:.2f}), "
                      f"{r[k]['peak_bytes'] / 2**20:.0f} MiB", flush=True)
            torch.cuda.empty_cache()
    if a.only in (None, "step"):
        r = res["step"] = run_step(a.repeat, dev)
        for k in ROUTES:
            print(f"step {B} x {N}, C = {C}, {k}: {r[k]['ms_median']:.1f} ms ({r[k]['ms_min']:.1f}..{r[k]['ms_max']:.1f}), "
                  f"{r[k]['peak_bytes'] / 2**20:.0f} MiB", flush=True)
        torch.cuda.empty_cache()
    if a.only in (None, "accuracy") and HAS_BF16:
        res["accuracy"] = run_accuracy()
    if a.parent_json:
        res["step_parent_commit"] = []
        for path in a.parent_json:
            with open(path) as f:
                p = json.load(f)
            res["step_parent_commit"].append({k: p[k] for k in ("commit", "date", "library_has_bf16", "routes", "step")})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
