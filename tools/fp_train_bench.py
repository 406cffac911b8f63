#!/usr/bin/env python3
"""Training-mode ``ops.FPModule`` with ``fused = True`` (layer 0 hoisted behind the interpolation, ``interp_add_relu``, ``relu_bn``)
beside the same module with ``fused = False`` (``knn_interpolate``, ``torch.cat``, PyTorch's Linear / ReLU / BatchNorm1d: what the
operators gave before the fused route existed), in one process.

    python tools/fp_train_bench.py [--repeat 10] [--commit <hash>] [--out profiles/fp_train_bench.json]

The four levels of an 8 x 16 384-point training batch, (n_c, m, Fc, Fs, NN); k = 2 as the reference builds its FPModules; the coarse
points are every second fine point (fp4: one point per batch at the origin).  Forward + backward of ``sum(out * g)`` with gradients to
x, x_skip and every parameter, timed with device events around the whole step - the neighbour search included, it is the same in both
routes; the method is ``tools/res_block_bench.py``'s: two warm-up steps per route, then ``--repeat`` steps that alternate between the
routes and rotate over three copies of the inputs; median, minimum and maximum.  ``peak_bytes`` is ``torch.cuda.max_memory_allocated``
over a step minus what was allocated before it.  ``*_rel_l2`` compare the two routes' results on the same inputs.
``concat_bytes_derived`` = m (Fc + Fs) 4 and ``layer0_gflop_derived`` = 2 m (Fc + Fs) C1 against 2 (n_c Fc + m Fs) C1 are counted from
the shapes, not measured.  Then, at the fp1 shape, ``relu_bn`` alone against ``bn(relu(z))`` and ``interp_add_relu`` alone against
``relu(knn_interpolate(Pc) + S)``.  No ratio is asserted: what is measured is what is written.
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
from pointstowood_amd import ops  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES, rel_l2  # noqa: E402

B, K = 8, 2
LEVELS = {"fp4": (8, 16384, 512, 512, [1024, 768, 512]), "fp3": (16384, 32768, 512, 256, [768, 640, 512]),
          "fp2": (32768, 65536, 512, 128, [640, 512, 512]), "fp1": (65536, 131072, 512, 32, [544, 512, 512])}


def timed(fn, leaves):
    """One forward + backward of fn(); (ms, peak bytes above what was allocated before, out, the first leaf's gradient)."""
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out, g = fn()
    (out * g).sum().backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out.detach(), leaves[0].grad


def geometry(n_c, m, dev, gen):
    pos_skip = torch.rand(m, 3, device=dev, generator=gen)
    batch_skip = torch.arange(m, device=dev) // (m // B)
    if n_c == B:
        return torch.zeros(B, 3, device=dev), torch.arange(B, device=dev), pos_skip, batch_skip
    return pos_skip[::m // n_c].contiguous(), batch_skip[::m // n_c].contiguous(), pos_skip, batch_skip


def module_step(mod, d):
    mod.zero_grad(set_to_none=True)
    x, xs = d["x"].detach().requires_grad_(), d["x_skip"].detach().requires_grad_()
    return timed(lambda: (mod(x, d["pos"], d["batch"], xs, d["pos_skip"], d["batch_skip"])[0], d["g"]), [x, xs])


def run_level(name, repeat, dev):
    n_c, m, Fc, Fs, NN = LEVELS[name]
    gen = torch.Generator(device=dev).manual_seed(n_c + m)
    sets = []
    for _ in range(COPIES):
        pos, batch, pos_skip, batch_skip = geometry(n_c, m, dev, gen)
        sets.append(dict(pos=pos, batch=batch, pos_skip=pos_skip, batch_skip=batch_skip, x=torch.randn(n_c, Fc, device=dev, generator=gen),
                         x_skip=torch.randn(m, Fs, device=dev, generator=gen), g=torch.randn(m, NN[-1], device=dev, generator=gen)))
    torch.manual_seed(0)
    fused = ops.FPModule(K, NN).to(dev).train()
    plain = copy.deepcopy(fused)
    plain.fused = False
    first, res_mod = alternate({"fused": fused, "plain": plain}, module_step, sets, repeat)
    res = {"level": name, "n_c": n_c, "m": m, "Fc": Fc, "Fs": Fs, "NN": NN, "k": K, "repeat": repeat, "rotating_inputs": COPIES,
           "concat_bytes_derived": m * (Fc + Fs) * 4,
           "layer0_gflop_derived": {"plain": 2 * m * (Fc + Fs) * NN[1] / 1e9, "hoisted": 2 * (n_c * Fc + m * Fs) * NN[1] / 1e9},
           "module": res_mod, "out_rel_l2": rel_l2(first["fused"][2], first["plain"][2]),
           "grad_x_rel_l2": rel_l2(first["fused"][3], first["plain"][3])}
    res["time_ratio_plain_over_fused"] = res_mod["plain"]["ms_median"] / res_mod["fused"]["ms_median"]
    res["peak_ratio_plain_over_fused"] = res_mod["plain"]["peak_bytes"] / res_mod["fused"]["peak_bytes"]
    return res


def run_solo(repeat, dev):
    """relu_bn and interp_add_relu on their own at the fp1 shape, each beside the composition it replaces."""
    n_c, m, _, _, NN = LEVELS["fp1"]
    C = NN[1]
    gen = torch.Generator(device=dev).manual_seed(7)
    sets = []
    for _ in range(COPIES):
        pos, batch, pos_skip, batch_skip = geometry(n_c, m, dev, gen)
        sets.append(dict(pos=pos, batch=batch, pos_skip=pos_skip, batch_skip=batch_skip, z=torch.randn(m, C, device=dev, generator=gen),
                         Pc=torch.randn(n_c, C, device=dev, generator=gen), g=torch.randn(m, C, device=dev, generator=gen)))
    bns = {k: torch.nn.BatchNorm1d(C).to(dev).train() for k in ("fused", "plain")}

    def bn_step(route, d):
        bn = bns[route]
        bn.zero_grad(set_to_none=True)
        z = d["z"].detach().requires_grad_()
        return timed(lambda: (ops.relu_bn(z, bn) if route == "fused" else bn(torch.relu(z)), d["g"]), [z])

    def interp_step(route, d):
        Pc, S = d["Pc"].detach().requires_grad_(), d["z"].detach().requires_grad_()
        geo = (d["pos"], d["pos_skip"], d["batch"], d["batch_skip"])
        if route == "fused":
            return timed(lambda: (ops.interp_add_relu(Pc, S, *geo, k=K), d["g"]), [Pc, S])
        return timed(lambda: (torch.relu(ops.knn_interpolate(Pc, *geo, k=K) + S), d["g"]), [Pc, S])

    out = {"m": m, "n_c": n_c, "C": C, "k": K, "repeat": repeat}
    for key, step in (("relu_bn", bn_step), ("interp_add_relu", interp_step)):
        first, r = alternate({"fused": "fused", "plain": "plain"}, step, sets, repeat)
        r["time_ratio_plain_over_fused"] = r["plain"]["ms_median"] / r["fused"]["ms_median"]
        r["out_rel_l2"] = rel_l2(first["fused"][2], first["plain"][2])
        r["grad_rel_l2"] = rel_l2(first["fused"][3], first["plain"][3])
        out[key] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--levels", nargs="*", default=list(LEVELS), choices=list(LEVELS))
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp_train_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "levels": []}
    for name in a.levels:
        r = run_level(name, a.repeat, dev)
        res["levels"].append(r)
        f, p = r["module"]["fused"], r["module"]["plain"]
        print(f"{name} n_c={r['n_c']} m={r['m']} NN={r['NN']}: fused {f['ms_median']:.2f} ms ({f['ms_min']:.2f}..{f['ms_max']:.2f}), "
              f"{f['peak_bytes'] / 2**20:.0f} MiB | plain {p['ms_median']:.2f} ms ({p['ms_min']:.2f}..{p['ms_max']:.2f}), "
              f"{p['peak_bytes'] / 2**20:.0f} MiB | plain / fused {r['time_ratio_plain_over_fused']:.2f}x, "
              f"out rel L2 {r['out_rel_l2']:.2e}, grad x rel L2 {r['grad_x_rel_l2']:.2e}", flush=True)
        torch.cuda.empty_cache()
    res["solo_fp1"] = run_solo(a.repeat, dev)
    for key in ("relu_bn", "interp_add_relu"):
        r = res["solo_fp1"][key]
        print(f"{key} alone at fp1: fused {r['fused']['ms_median']:.2f} ms, {r['fused']['peak_bytes'] / 2**20:.0f} MiB | plain "
              f"{r['plain']['ms_median']:.2f} ms, {r['plain']['peak_bytes'] / 2**20:.0f} MiB | plain / fused "
              f"{r['time_ratio_plain_over_fused']:.2f}x", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
