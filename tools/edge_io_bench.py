#!/usr/bin/env python3
"""``ops.edge_layer1`` with a float16 / bfloat16 H1 and a recomputed ReLU mask under autocast: ``ops.PointNetConv`` in training mode at
the three level shapes and one whole training step of ``pointstowood_amd.train.Net``, ``ops.half_io`` on against off - for float16 and
for bfloat16, in one process.

    python tools/edge_io_bench.py [--repeat 10] [--only layer|step] [--dtypes fp16 bf16] [--commit <hash>] [--parent-json FILE ...]
                                  [--out profiles/edge_io_bench.json]

The method is ``tools/bn_max_io_bench.py``'s (an 8 x 16 384-point batch at C = 32, k = 32; device events around forward + backward - the
whole trainer step for the network; two warm-up steps per route, then ``--repeat`` steps that alternate between the routes and rotate
over three copies of the inputs; median, minimum and maximum; ``peak_bytes`` above what was allocated before the step, the inputs
among it).  Routes, all from the same weights:

    layer      on          half_io on: edge_layer1 writes H1 in the autocast dtype, saves no [E, C1] tensor, recomputes the mask
               off         half_io off: every operator casts first (edge_layer1: fp32 H1 saved, the GEMM casts it)
               cast_edge   half_io on, but edge_layer1 alone called as before this route existed (fp32 out, the GEMM casts it): what
                           separates edge_layer1's own share from the other operators that half_io switches in the same layer
    step       plain_on / plain_off / fused_on / fused_off: fused_bn_max False / True on the three PointNetConvs x half_io on / off

On a tree whose library has no ``p2w_edge_l1_io`` only the whole step with half_io on runs, as routes ``plain_parent`` and
``fused_parent``: the times the new code is compared against, taken in a process of its own.  Write them with ``--out`` and give the
file to the run on the new tree as ``--parent-json``, which copies it into ``step_parent_commit`` of its own output.

``verdict`` applies the rule fixed before the measurement: a route is called faster only where the gain of the medians exceeds the
larger of the two routes' min .. max spreads, and slower only where the loss does.  The peak difference is reported beside the derived
``4 E C1`` bytes per level (the fp32 H1 that is no longer kept); it is no gate.  ``bytes_per_element_derived`` are computed from the
operations, not measured.
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import _lib, ops, synthetic_voxels, train  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES, K, LEVELS, level_inputs, mlp  # noqa: E402
from tools.net_train_bench import B, C, N, _Batch, measured  # noqa: E402

HAS_IO = "p2w_edge_l1_io" in _lib.SIGNATURES
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
LAYER_ROUTES = {"on": (True, False), "off": (False, False), "cast_edge": (True, True)}                  # route -> (half_io, cast edge_layer1 first)
STEP_ROUTES = ({"plain_on": (False, True), "plain_off": (False, False), "fused_on": (True, True), "fused_off": (True, False)}
               if HAS_IO else {"plain_parent": (False, True), "fused_parent": (True, True)})           # route -> (fused_bn_max, half_io)
# HBM bytes per element of H1 [E, C1], forward and backward, from the operations (the gather of P, [n_src, C1], is not counted: it is
# read once from HBM and again from the caches): cast first = fp32 store, cast (4 + 2), GEMM read 2 | gradient widened (2 + 4), the
# fp32 gradient and the fp32 H1 read twice each; 16-bit = 16-bit store, GEMM read | the 16-bit gradient read twice and geo, src
BYTES_DERIVED = {"edge_layer1_cast_first": [12, 26], "edge_layer1_16bit_io": [4, 6]}


class _switch:
    """ops.half_io = value; with cast_edge, ops.edge_layer1 is called without out_dtype for the time being."""

    def __init__(self, value, cast_edge=False):
        self.value, self.cast_edge = value, cast_edge

    def __enter__(self):
        self.old, ops.half_io = ops.half_io, self.value
        self.inner = ops.edge_layer1
        if self.cast_edge:
            ops.edge_layer1 = lambda *a, **k: self.inner(*a)

    def __exit__(self, *a):
        ops.half_io, ops.edge_layer1 = self.old, self.inner


def verdict(new, old):
    """The rule: faster / slower only where the difference of the medians exceeds the larger min .. max spread."""
    gain, spread = old["ms_median"] - new["ms_median"], max(new["ms_max"] - new["ms_min"], old["ms_max"] - old["ms_min"])
    return {"gain_ms": gain, "larger_min_max_spread_ms": spread, "faster": bool(gain > spread), "slower": bool(-gain > spread),
            "peak_saved_bytes": old["peak_bytes"] - new["peak_bytes"]}


def run_layer(shape, dtype, repeat, dev):
    n_src, M, F_in, C1, C2 = shape
    sets = level_inputs(n_src, M, F_in, C2, dev, seed=n_src)
    E = int(sets[0]["ei"].shape[1])
    torch.manual_seed(0)
    base = ops.PointNetConv(local_nn=mlp(F_in, C1, C2), add_self_loops=False).to(dev).train()
    convs = {route: copy.deepcopy(base) for route in LAYER_ROUTES}

    def step(route, d):
        (on, cast_edge), conv = LAYER_ROUTES[route], convs[route]
        conv.zero_grad(set_to_none=True)
        x, ps = d["x"].detach().requires_grad_(), d["pos_src"].detach().requires_grad_()

        def fn():
            with _switch(on, cast_edge), torch.autocast("cuda", dtype=dtype):
                out = conv(x, (ps, d["pos_dst"]), d["ei"])
            (out.float() * d["g"]).sum().backward()
            return out.detach(), x.grad
        return measured(fn)

    first, r = alternate({k: k for k in LAYER_ROUTES}, step, sets, repeat)
    r.update(n_src=n_src, M=M, F_in=F_in, C1=C1, C2=C2, k=K, E=E, repeat=repeat, rotating_inputs=COPIES, fp32_H1_bytes_derived=4 * E * C1)
    r["verdict_on_vs_off"] = verdict(r["on"], r["off"])
    r["verdict_on_vs_cast_edge"] = verdict(r["on"], r["cast_edge"])
    r["same_bits"] = bool(all(torch.equal(first["on"][i], first[k][i]) for k in ("off", "cast_edge") for i in (2, 3)))
    return r


def run_step(dtype, repeat, dev):
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
    shapes = []
    for route, (fused, _) in STEP_ROUTES.items():
        for m in nets[route].modules():
            if isinstance(m, ops.PointNetConv):
                m.fused_bn_max = fused
    half = dtype == torch.float16
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    state = {k: (torch.optim.AdamW(n.parameters(), lr=1e-4, weight_decay=1e-2), torch.amp.GradScaler("cuda", init_scale=512, enabled=half))
             for k, n in nets.items()}

    def step(route, d):
        net, (optimizer, scaler), (_, on) = nets[route], state[route], STEP_ROUTES[route]

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
                if half or math.isfinite(float(norm)):                      # (the bfloat16 loop's one host read: trainer.finish_step)
                    scaler.step(optimizer)
                scaler.update()
            return outputs.detach(), grad
        return measured(fn)

    # the three [E, C1] shapes of a step: one forward with edge_layer1 watched, outside the measurement
    inner = ops.edge_layer1

    def watch(*a, **k):
        out = inner(*a, **k)
        shapes.append(tuple(out.shape))
        return out
    ops.edge_layer1 = watch
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            copy.deepcopy(base)(sets[0])
    finally:
        ops.edge_layer1 = inner
    _, r = alternate({k: k for k in STEP_ROUTES}, step, sets, repeat)
    r.update(voxels=B, points_per_voxel=N, C=C, repeat=repeat, rotating_inputs=COPIES, H1_shapes=shapes,
             fp32_H1_bytes_derived=sum(4 * e * c for e, c in shapes),
             note="the nets start from the same weights and draw different random samples: their logits are not compared")
    if HAS_IO:
        r["verdict_plain_on_vs_off"] = verdict(r["plain_on"], r["plain_off"])
        r["verdict_fused_on_vs_off"] = verdict(r["fused_on"], r["fused_off"])
    return r


def _line(what, k, v):
    print(f"{what} {k}: {v['ms_median']:.2f} ms ({v['ms_min']:.2f}..{v['ms_max']:.2f}), {v['peak_bytes'] / 2**20:.0f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["layer", "step"], default=None)
    ap.add_argument("--dtypes", nargs="*", choices=list(DTYPES), default=list(DTYPES))
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--parent-json", action="append", default=[], help="--out file of this tool's run on the parent commit's tree; repeatable")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_io_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "library_has_edge_l1_io": HAS_IO,
           "bytes_per_element_derived": BYTES_DERIVED, "layer": {}, "step": {}}
    for name in a.dtypes:
        dtype = DTYPES[name]
        if a.only in (None, "layer") and HAS_IO:
            res["layer"][name] = []
            for li in a.levels:
                r = run_layer(LEVELS[li], dtype, a.repeat, dev)
                res["layer"][name].append(r)
                for k in LAYER_ROUTES:
                    _line(f"{name} PointNetConv level {li} [{r['E']}, {r['C1']}]", k, r[k])
                torch.cuda.empty_cache()
        if a.only in (None, "step"):
            r = res["step"][name] = run_step(dtype, a.repeat, dev)
            for k in STEP_ROUTES:
                _line(f"{name} step {B} x {N}, C = {C}", k, r[k])
            torch.cuda.empty_cache()
    if a.parent_json:
        res["step_parent_commit"] = []
        for path in a.parent_json:
            with open(path) as f:
                p = json.load(f)
            res["step_parent_commit"].append({k: p[k] for k in ("commit", "date", "library_has_edge_l1_io", "step")})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
