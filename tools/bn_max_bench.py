#!/usr/bin/env python3
"""Training-mode ``ops.PointNetConv`` with ``fused_bn_max`` on and off, and ``ops.relu_bn_max`` alone beside
``ops.scatter_max(bn(relu(z)))``.

    python tools/bn_max_bench.py [--repeat 10] [--commit <hash>] [--out profiles/bn_max_bench.json]

The three level shapes, the inputs and the method are ``tools/conv_train_bench.py``'s: forward + backward of ``sum(out * g)`` with
gradients to x, to pos_src and to every parameter (to z and BatchNorm's weight and bias for the operator alone), timed with device
events around the whole step; two warm-up steps per route, then ``--repeat`` steps that alternate between the routes and rotate over
three copies of the inputs; median, minimum and maximum.  ``peak_bytes`` is ``torch.cuda.max_memory_allocated`` over a step minus
what was allocated before it (inputs and parameters; for the operator alone z counts as an input).  ``*_rel_l2`` compare the two
routes' results on the same inputs.  ``edge_tensor_bytes_derived`` = E C2 4 is one [E, C2] fp32 tensor and
``passes_saved_derived`` the [E, C2] passes the fused route leaves out after the GEMM (7 + 9 against 1 + 2), both computed from the
shapes, not measured.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import ops  # noqa: E402
from tools.conv_train_bench import COPIES, LEVELS, level_inputs, mlp, rel_l2, step  # noqa: E402

PASSES_PLAIN, PASSES_FUSED = 7 + 9, 1 + 2


def op_step(fn, bn, d, M):
    """One forward + backward of the operator alone; (ms, peak bytes above what was allocated before, out, grad_z)."""
    bn.zero_grad(set_to_none=True)
    z = d["z"].detach().requires_grad_()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn(z, d["index"], bn, M)
    (out * d["g"]).sum().backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out.detach(), z.grad


def summarise(ms, peak):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "peak_bytes": max(peak)}


def alternate(routes, run, sets, repeat):
    """Two warm-up steps per route, then `repeat` steps alternating between the routes over rotating inputs."""
    first = {}
    for name, r in routes.items():
        for _ in range(2):
            first[name] = run(r, sets[0])
    ms, peak = {k: [] for k in routes}, {k: [] for k in routes}
    for i in range(repeat):
        for name, r in routes.items():
            t, p, _, _ = run(r, sets[i % COPIES])
            ms[name].append(t)
            peak[name].append(p)
    return first, {k: summarise(ms[k], peak[k]) for k in routes}


def run_level(shape, repeat, dev):
    n_src, M, F_in, C1, C2 = shape
    sets = level_inputs(n_src, M, F_in, C2, dev, seed=n_src)
    E = int(sets[0]["ei"].shape[1])
    torch.manual_seed(0)
    nn = mlp(F_in, C1, C2)
    layers = {"fused": ops.PointNetConv(local_nn=copy.deepcopy(nn), add_self_loops=False).to(dev).train(),
              "plain": ops.PointNetConv(local_nn=copy.deepcopy(nn), add_self_loops=False).to(dev).train()}
    layers["fused"].fused_bn_max = True
    first, res_layer = alternate(layers, step, sets, repeat)
    res = {"n_src": n_src, "M": M, "F_in": F_in, "C1": C1, "C2": C2, "E": E, "repeat": repeat, "rotating_inputs": COPIES,
           "edge_tensor_bytes_derived": E * C2 * 4, "passes_saved_derived": PASSES_PLAIN - PASSES_FUSED,
           "traffic_saved_bytes_derived": (PASSES_PLAIN - PASSES_FUSED) * E * C2 * 4,
           "layer": res_layer, "layer_out_rel_l2": rel_l2(first["fused"][2], first["plain"][2]),
           "layer_grad_x_rel_l2": rel_l2(first["fused"][3], first["plain"][3])}
    res["layer_time_ratio_plain_over_fused"] = res_layer["plain"]["ms_median"] / res_layer["fused"]["ms_median"]
    res["layer_peak_ratio_plain_over_fused"] = res_layer["plain"]["peak_bytes"] / res_layer["fused"]["peak_bytes"]
    del layers, first
    torch.cuda.empty_cache()
    # the operator alone on a z of the level's shape
    g = torch.Generator(device=dev).manual_seed(n_src + 1)
    index = sets[0]["ei"][1].contiguous()
    zsets = [dict(z=torch.randn(E, C2, device=dev, generator=g), index=index, g=s["g"]) for s in sets]
    del sets
    bn = nn[1][2]
    ops_ = {"fused": (ops.relu_bn_max, copy.deepcopy(bn).to(dev).train()),
            "plain": (lambda z, i, b, m: ops.scatter_max(b(torch.relu(z)), i, dim=0, dim_size=m)[0], copy.deepcopy(bn).to(dev).train())}
    first, res_op = alternate(ops_, lambda r, d: op_step(r[0], r[1], d, M), zsets, repeat)
    res["operator"] = res_op
    res["operator_out_rel_l2"] = rel_l2(first["fused"][2], first["plain"][2])
    res["operator_grad_z_rel_l2"] = rel_l2(first["fused"][3], first["plain"][3])
    res["operator_time_ratio_plain_over_fused"] = res_op["plain"]["ms_median"] / res_op["fused"]["ms_median"]
    res["operator_peak_ratio_plain_over_fused"] = res_op["plain"]["peak_bytes"] / res_op["fused"]["peak_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_max_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "levels": []}
    for li in a.levels:
        r = run_level(LEVELS[li], a.repeat, dev)
        res["levels"].append(r)
        for what in ("layer", "operator"):
            f, p = r[what]["fused"], r[what]["plain"]
            print(f"level {li} E={r['E']} C2={r['C2']} {what}: fused {f['ms_median']:.2f} ms ({f['ms_min']:.2f}..{f['ms_max']:.2f}), "
                  f"{f['peak_bytes'] / 2**20:.0f} MiB | plain {p['ms_median']:.2f} ms ({p['ms_min']:.2f}..{p['ms_max']:.2f}), "
                  f"{p['peak_bytes'] / 2**20:.0f} MiB | plain / fused {r[what + '_time_ratio_plain_over_fused']:.2f}x", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
