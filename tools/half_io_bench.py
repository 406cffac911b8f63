#!/usr/bin/env python3
"""``ops.half_io`` on against off: the four operator families that take a float16 tensor as it is, each alone, and one whole training
step of ``pointstowood_amd.train.Net``, in one process.

    python tools/half_io_bench.py [--repeat 10] [--only ops|step] [--commit <hash>] [--out profiles/half_io_bench.json]

Shapes of an 8 x 16 384-point batch at C = 32, every operator forward + backward under autocast on a float16 input:

    bn_chain        z [65 536, 512], three stages (the middle chain of sa1's residual block), out_dtype = float16
    relu_bn         z [131 072, 256], out_dtype = float16
    bn_relu_rowdot  z [131 072, 512] (the head)
    scatter_max     x [2 097 152, 128] over 65 536 targets of 32 rows (sa1's edge tensor)

and the whole step as ``tools/net_train_bench.py`` takes it.  On a commit without the switch (``ops.half_io`` absent) only the whole
step runs, as route ``absent``: the baseline that ``off`` must agree with.

Timed with device events; the method is ``tools/net_train_bench.py``'s: two warm-up steps per route, then ``--repeat`` steps that
alternate between the routes and rotate over three copies of the inputs; median, minimum and maximum.  ``peak_bytes`` is
``torch.cuda.max_memory_allocated`` over a step minus what was allocated before it (the inputs).  The two routes give the same bits
(tests/test_gpu_half_io.py); no ratio is asserted: what is measured is what is written.

What an operator row times: the call and ``backward`` on a cotangent that already has the output's dtype (it is cast before the
timing starts).  ``bn_chain`` and ``relu_bn`` are asked for ``out_dtype=torch.float16`` on both routes, so ``off`` ends with the
``.to(float16)`` of its fp32 result inside the operator; in the network's ``off`` route the modules do not ask for float16 and the
same pass runs inside the next ``F.linear`` under autocast instead - the row charges it to the operator, the step to the GEMM.
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
from pointstowood_amd import ops, synthetic_voxels, train  # noqa: E402
from pointstowood_amd.loss import Poly1FocalLoss  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES  # noqa: E402
from tools.net_train_bench import B, C, N, _Batch, measured  # noqa: E402

HAS_SWITCH = hasattr(ops, "half_io")
ROUTES = {"on": True, "off": False} if HAS_SWITCH else {"absent": None}


class _switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        if self.value is not None:
            self.old, ops.half_io = ops.half_io, self.value

    def __exit__(self, *a):
        if self.value is not None:
            ops.half_io = self.old


def _bn(width, dev):
    return torch.nn.BatchNorm1d(width).to(dev).train()


def _dw(width, dev):
    return torch.nn.Conv1d(width, width, 1, groups=width).to(dev)


def operator_families(dev):
    """name -> (shape, make(): modules, call(z, modules) -> out)."""
    n_dst, k = B * N // 2, 32
    index = torch.arange(n_dst, device=dev).repeat_interleave(k)
    return {
        "bn_chain": ((B * N // 2, 16 * C), lambda: [_bn(16 * C, dev), _bn(16 * C, dev), _bn(16 * C, dev), _dw(16 * C, dev)],
                     lambda z, m: ops.bn_chain(z, [(m[0], True), (m[1], True), (m[2], True, m[3])], out_dtype=torch.float16)),
        "relu_bn": ((B * N, 8 * C), lambda: [_bn(8 * C, dev)], lambda z, m: ops.relu_bn(z, m[0], out_dtype=torch.float16)),
        "bn_relu_rowdot": ((B * N, 16 * C), lambda: [_bn(16 * C, dev), torch.nn.Conv1d(16 * C, 1, 1).to(dev)],
                           lambda z, m: ops.bn_relu_rowdot(z, m[0], m[1].weight, m[1].bias)),
        "scatter_max": ((n_dst * k, 4 * C), lambda: [], lambda z, m: ops.scatter_max(z, index, dim=0, dim_size=n_dst)[0]),
    }


def run_operator(name, shape, make, call, repeat, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    sets = [torch.randn(shape, device=dev, generator=gen).half() for _ in range(COPIES)]
    torch.manual_seed(0)
    base = make()
    mods = {route: copy.deepcopy(base) for route in ROUTES}          # the same weights on every route: their bits are compared
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        like = call(sets[0], copy.deepcopy(base))
    cot32 = torch.randn(like.shape, device=dev, generator=gen)
    cot = {dt: cot32.to(dt) for dt in (torch.float16, torch.float32)}    # cast once, outside the timed step
    del like, cot32

    def step(route, z16):
        for m in mods[route]:
            m.zero_grad(set_to_none=True)
        z = z16.detach().requires_grad_()

        def fn():
            with _switch(ROUTES[route]), torch.autocast("cuda", dtype=torch.float16):
                out = call(z, mods[route])
            out.backward(cot[out.dtype])
            return out.detach(), z.grad
        return measured(fn)

    first, r = alternate({k: k for k in ROUTES}, step, sets, repeat)
    r.update(shape=list(shape), repeat=repeat, rotating_inputs=COPIES)
    if HAS_SWITCH:
        r["time_ratio_off_over_on"] = r["off"]["ms_median"] / r["on"]["ms_median"]
        r["same_bits"] = bool(torch.equal(first["on"][2], first["off"][2]) and torch.equal(first["on"][3], first["off"][3]))
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
    state = {k: (torch.optim.AdamW(n.parameters(), lr=1e-4, weight_decay=1e-2), torch.amp.GradScaler("cuda", init_scale=512))
             for k, n in nets.items()}

    def step(route, d):
        net, (optimizer, scaler) = nets[route], state[route]

        def fn():
            with _switch(ROUTES[route]):
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

    _, r = alternate({k: k for k in ROUTES}, step, sets, repeat)
    r.update(voxels=B, points_per_voxel=N, C=C, repeat=repeat, rotating_inputs=COPIES,
             note="the nets start from the same weights and draw different random samples: their logits are not compared")
    if HAS_SWITCH:
        r["time_ratio_off_over_on"] = r["off"]["ms_median"] / r["on"]["ms_median"]
        r["peak_ratio_off_over_on"] = r["off"]["peak_bytes"] / r["on"]["peak_bytes"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--only", choices=["ops", "step"], default=None)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("half_io_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "half_io_switch": HAS_SWITCH}
    if a.only != "step" and HAS_SWITCH:
        res["operators"] = {}
        for name, (shape, make, call) in operator_families(dev).items():
            r = res["operators"][name] = run_operator(name, shape, make, call, a.repeat, dev)
            for k in ROUTES:
                print(f"{name} {list(shape)} half_io {k}: {r[k]['ms_median']:.2f} ms ({r[k]['ms_min']:.2f}..{r[k]['ms_max']:.2f}), "
                      f"{r[k]['peak_bytes'] / 2**20:.0f} MiB", flush=True)
            torch.cuda.empty_cache()
    if a.only != "ops":
        r = res["step"] = run_step(a.repeat, dev)
        for k in ROUTES:
            print(f"step {B} x {N}, C = {C}, half_io {k}: {r[k]['ms_median']:.1f} ms ({r[k]['ms_min']:.1f}..{r[k]['ms_max']:.1f}), "
                  f"{r[k]['peak_bytes'] / 2**20:.0f} MiB", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
