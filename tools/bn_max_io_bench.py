#!/usr/bin/env python3
"""``ops.relu_bn_max`` on the 16-bit output of the layer-2 GEMM under autocast: ``ops.half_io`` on against off and against the plain
composition ``scatter_max(bn(relu(z)))``, at the three level shapes, and what ``fused_bn_max`` then does to one whole training step of
``pointstowood_amd.train.Net`` - for float16 and for bfloat16, in one process.

    python tools/bn_max_io_bench.py [--repeat 10] [--only ops|step] [--dtypes fp16 bf16] [--commit <hash>] [--parent-json FILE ...]
                                    [--out profiles/bn_max_io_bench.json]

The method is ``tools/bf16_io_bench.py``'s (an 8 x 16 384-point batch at C = 32; device events around forward + backward - the whole
trainer step for the network; two warm-up steps per route, then ``--repeat`` steps that alternate between the routes and rotate over
three copies of the inputs; median, minimum and maximum; ``peak_bytes`` above what was allocated before the step, the inputs among
it).  The operator's z is [E, C2] with E = 32 M of ``tools/conv_train_bench.py``'s LEVELS, 32 rows per target.  Routes:

    operator   io_on      relu_bn_max, half_io on: z read as it is and saved itself, dz written in its dtype by the kernel
               io_off     relu_bn_max, half_io off: z cast to fp32 first, that copy saved, fp32 dz rounded in one more pass
               plain      scatter_max(bn(relu(z))) in the autocast dtype, half_io on
    step       fused_on / fused_off / plain_on / plain_off: fused_bn_max True / False on the three PointNetConvs x half_io on / off

On a tree whose library has no ``p2w_relu_bn_max_io`` only the whole step with ``fused_bn_max`` True runs, as route ``fused_parent``:
the time the new code is compared against, taken in a process of its own.  Write it with ``--out`` and give the file to the run on
the new tree as ``--parent-json``, which copies it into ``step_parent_commit`` of its own output.

``verdict`` applies the rule fixed before the measurement: ``--fused_bn_max`` is recommended for speed only if the step's gain of
fused_on over plain_on exceeds the larger of the two routes' min .. max spreads; the peak difference is reported either way.
``bytes_per_element_derived`` are computed from the operations, not measured.
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
from tools.conv_train_bench import COPIES, K, LEVELS  # noqa: E402
from tools.net_train_bench import B, C, N, _Batch, measured  # noqa: E402

HAS_IO = "p2w_relu_bn_max_io" in _lib.SIGNATURES
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
OP_ROUTES = {"io_on": (True, True), "io_off": (True, False), "plain": (False, True)}                    # route -> (fused, half_io)
STEP_ROUTES = ({"fused_on": (True, True), "fused_off": (True, False), "plain_on": (False, True), "plain_off": (False, False)}
               if HAS_IO else {"fused_parent": (True, True)})
# bytes per element of z [E, C2], forward and backward, from the operations
BYTES_DERIVED = {"plain_16bit_composition": [12, 18], "relu_bn_max_16bit_io": [2, 4], "relu_bn_max_cast_first": [10, 14]}


class _switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old, ops.half_io = ops.half_io, self.value

    def __exit__(self, *a):
        ops.half_io = self.old


def _plain(z, index, bn, M):
    return ops.scatter_max(bn(torch.relu(z)), index, dim=0, dim_size=M)[0]


def run_operator(shape, dtype, repeat, dev):
    _, M, _, _, C2 = shape
    E = M * K
    gen = torch.Generator(device=dev).manual_seed(M)
    index = torch.arange(M, device=dev).repeat_interleave(K)
    sets = [dict(z=torch.randn(E, C2, device=dev, generator=gen).to(dtype), g=torch.randn(M, C2, device=dev, generator=gen))
            for _ in range(COPIES)]
    torch.manual_seed(0)
    base = torch.nn.BatchNorm1d(C2).to(dev).train()
    bns = {route: copy.deepcopy(base) for route in OP_ROUTES}

    def step(route, d):
        fused, on = OP_ROUTES[route]
        bn = bns[route]
        bn.zero_grad(set_to_none=True)
        z = d["z"].detach().requires_grad_()

        def fn():
            with _switch(on), torch.autocast("cuda", dtype=dtype):
                out = (ops.relu_bn_max if fused else _plain)(z, index, bn, M)
            out.backward(d["g"])
            return out.detach(), z.grad
        return measured(fn)

    first, r = alternate({k: k for k in OP_ROUTES}, step, sets, repeat)
    r.update(E=E, M=M, C2=C2, repeat=repeat, rotating_inputs=COPIES, z_bytes=E * C2 * 2)
    r["time_ratio_io_off_over_on"] = r["io_off"]["ms_median"] / r["io_on"]["ms_median"]
    r["time_ratio_plain_over_io_on"] = r["plain"]["ms_median"] / r["io_on"]["ms_median"]
    r["peak_saved_bytes_io_on_vs_off"] = r["io_off"]["peak_bytes"] - r["io_on"]["peak_bytes"]
    r["peak_saved_bytes_io_on_vs_plain"] = r["plain"]["peak_bytes"] - r["io_on"]["peak_bytes"]
    r["same_bits_io_on_off"] = bool(torch.equal(first["io_on"][2], first["io_off"][2]) and torch.equal(first["io_on"][3], first["io_off"][3]))
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

    _, r = alternate({k: k for k in STEP_ROUTES}, step, sets, repeat)
    r.update(voxels=B, points_per_voxel=N, C=C, repeat=repeat, rotating_inputs=COPIES,
             note="the nets start from the same weights and draw different random samples: their logits are not compared")
    if HAS_IO:
        f, p = r["fused_on"], r["plain_on"]
        gain, spread = p["ms_median"] - f["ms_median"], max(f["ms_max"] - f["ms_min"], p["ms_max"] - p["ms_min"])
        r["verdict"] = {"gain_ms_fused_on_over_plain_on": gain, "larger_min_max_spread_ms": spread, "recommend_for_speed": bool(gain > spread),
                        "peak_saved_bytes_fused_on_vs_plain_on": p["peak_bytes"] - f["peak_bytes"],
                        "gain_ms_fused_on_over_fused_off": r["fused_off"]["ms_median"] - f["ms_median"],
                        "peak_saved_bytes_fused_on_vs_fused_off": r["fused_off"]["peak_bytes"] - f["peak_bytes"]}
    return r


def _line(what, k, v):
    print(f"{what} {k}: {v['ms_median']:.2f} ms ({v['ms_min']:.2f}..{v['ms_max']:.2f}), {v['peak_bytes'] / 2**20:.0f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["ops", "step"], default=None)
    ap.add_argument("--dtypes", nargs="*", choices=list(DTYPES), default=list(DTYPES))
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--parent-json", action="append", default=[], help="--out file of this tool's run on the parent commit's tree; repeatable")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_max_io_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "library_has_relu_bn_max_io": HAS_IO,
           "bytes_per_element_derived": BYTES_DERIVED, "operator": {}, "step": {}}
    for name in a.dtypes:
        dtype = DTYPES[name]
        if a.only in (None, "ops") and HAS_IO:
            res["operator"][name] = []
            for li in a.levels:
                r = run_operator(LEVELS[li], dtype, a.repeat, dev)
                res["operator"][name].append(r)
                for k in OP_ROUTES:
                    _line(f"{name} relu_bn_max level {li} [{r['E']}, {r['C2']}]", k, r[k])
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
            res["step_parent_commit"].append({k: p[k] for k in ("commit", "date", "library_has_relu_bn_max_io", "step")})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
