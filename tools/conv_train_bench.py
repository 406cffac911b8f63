#!/usr/bin/env python3
"""Training-mode ``ops.PointNetConv`` (hoisted layer 1 through ``ops.edge_layer1``) beside the route that trained before it: a
reference-style ``PointNetConv`` subclass over ``ops.MessagePassing`` that builds the [E, F_in + 4] message per edge.

    python tools/conv_train_bench.py [--repeat 10] [--commit <hash>] [--out profiles/conv_train_bench.json]

Three levels of the reference's training step (8 voxels of 16 384 points, every level keeps half of the points, k = 32), as
(n_src, M, F_in, C1, C2): (131072, 65536, 32, 64, 128), (65536, 32768, 128, 192, 256), (32768, 16384, 256, 384, 512).  Edges come from
``ops.knn`` on uniform points, the targets are a sorted random half of the sources of each voxel.

Per level and route: forward + backward of ``sum(out * g)`` with gradients to x, to pos_src and to every parameter, timed with
device events around the whole step; two warm-up steps per route, then ``--repeat`` steps that alternate between the routes and
rotate over three copies of the inputs; median, minimum and maximum.  ``peak_bytes`` is ``torch.cuda.max_memory_allocated`` over a
step minus what was allocated before it (inputs and parameters).  ``out_rel_l2`` / ``grad_x_rel_l2`` compare the two routes' results
on the same inputs, ``grad_x_row_rel_median`` / ``grad_x_rows_above_1e-4`` row by row (see ``row_diff``).
``message_bytes_derived`` = E (F_in + 4) 4 is the message tensor alone, computed from the shapes, not measured.
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
from torch.nn import BatchNorm1d as BN, Linear as Lin, ReLU, Sequential as Seq

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import ops  # noqa: E402

LEVELS = [(131072, 65536, 32, 64, 128), (65536, 32768, 128, 192, 256), (32768, 16384, 256, 384, 512)]
VOXELS, K, COPIES = 8, 32, 3


class MessageConv(ops.MessagePassing):
    """The layer as the reference writes it (pointnet.py:19-132): gathers per edge, message(), max aggregation by propagate."""

    def __init__(self, local_nn):
        super().__init__(aggr="max")
        self.local_nn = local_nn

    def forward(self, x, pos, edge_index):
        return self.propagate(edge_index, x=(x, None), pos=pos)

    def message(self, x_j, pos_i, pos_j, edge_index_i):
        msg = torch.zeros((pos_j.size(0), pos_j.size(1)), device=pos_j.device)
        relative_pos = pos_j[:, :3] - pos_i[:, :3]
        max_distances, _ = ops.scatter_max(torch.norm(relative_pos, dim=1, keepdim=True), edge_index_i, dim=0)
        msg[:, :3] = relative_pos / (max_distances[edge_index_i] + 1e-8)
        msg[:, 3] = pos_j[:, 3]
        return self.local_nn(torch.cat([x_j, msg], dim=1))


def mlp(f_in, c1, c2):
    return Seq(Seq(Lin(f_in + 4, c1), ReLU()), Seq(Lin(c1, c2), ReLU(), BN(c2)))


def level_inputs(n_src, M, F_in, C2, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    per, keep = n_src // VOXELS, M // VOXELS
    pos = torch.rand(n_src, 4, device=dev, generator=g)
    batch = torch.repeat_interleave(torch.arange(VOXELS, device=dev), per)
    idx = torch.cat([v * per + torch.randperm(per, device=dev, generator=g)[:keep].sort().values for v in range(VOXELS)])
    row, col = ops.knn(pos[:, :3], pos[idx, :3], K, batch, batch[idx])
    sets = []
    for _ in range(COPIES):
        sets.append(dict(x=torch.randn(n_src, F_in, device=dev, generator=g), pos_src=pos.clone(), pos_dst=pos[idx].clone(),
                         ei=torch.stack([col, row], 0).clone(), g=torch.randn(M, C2, device=dev, generator=g)))
    return sets


def step(conv, d):
    """One training step's forward + backward; (ms, peak bytes above what was allocated before, out, grad_x)."""
    conv.zero_grad(set_to_none=True)
    x, ps = d["x"].detach().requires_grad_(), d["pos_src"].detach().requires_grad_()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = conv(x, (ps, d["pos_dst"]), d["ei"])
    (out * d["g"]).sum().backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out.detach(), x.grad


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def row_diff(a, b):
    """Per row of the gradient: |a - b| / |b|; (median, rows above 1e-4).  A winner of the max that switches at a near-tie moves
    whole rows of a few sources; a different summation order moves every row in its last bits."""
    r = (a.double() - b.double()).norm(dim=1) / b.double().norm(dim=1).clamp_min(1e-300)
    return float(r.median()), int((r > 1e-4).sum())


def run_level(shape, repeat, dev):
    n_src, M, F_in, C1, C2 = shape
    sets = level_inputs(n_src, M, F_in, C2, dev, seed=n_src)
    E = int(sets[0]["ei"].shape[1])
    torch.manual_seed(0)
    nn = mlp(F_in, C1, C2)
    routes = {"edge_layer1": ops.PointNetConv(local_nn=copy.deepcopy(nn), add_self_loops=False).to(dev).train(),
              "message_passing": MessageConv(copy.deepcopy(nn)).to(dev).train()}
    first = {}
    for name, conv in routes.items():
        for w in range(2):
            first[name] = step(conv, sets[0])
    ms, peak = {k: [] for k in routes}, {k: [] for k in routes}
    for r in range(repeat):
        for name, conv in routes.items():
            t, p, _, _ = step(conv, sets[r % COPIES])
            ms[name].append(t)
            peak[name].append(p)
    res = {"n_src": n_src, "M": M, "F_in": F_in, "C1": C1, "C2": C2, "k": K, "E": E, "repeat": repeat, "rotating_inputs": COPIES,
           "message_bytes_derived": E * (F_in + 4) * 4,
           "out_rel_l2": rel_l2(first["edge_layer1"][2], first["message_passing"][2]),
           "grad_x_rel_l2": rel_l2(first["edge_layer1"][3], first["message_passing"][3])}
    res["grad_x_row_rel_median"], res["grad_x_rows_above_1e-4"] = row_diff(first["edge_layer1"][3], first["message_passing"][3])
    for name in routes:
        res[name] = {"ms_median": statistics.median(ms[name]), "ms_min": min(ms[name]), "ms_max": max(ms[name]), "peak_bytes": max(peak[name])}
    res["time_ratio_message_passing_over_edge_layer1"] = res["message_passing"]["ms_median"] / res["edge_layer1"]["ms_median"]
    res["peak_ratio_message_passing_over_edge_layer1"] = res["message_passing"]["peak_bytes"] / res["edge_layer1"]["peak_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_train_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "levels": []}
    for li in a.levels:
        r = run_level(LEVELS[li], a.repeat, dev)
        res["levels"].append(r)
        print(f"level {li} E={r['E']}: edge_layer1 {r['edge_layer1']['ms_median']:.2f} ms ({r['edge_layer1']['ms_min']:.2f}..{r['edge_layer1']['ms_max']:.2f}), "
              f"{r['edge_layer1']['peak_bytes'] / 2**20:.0f} MiB | message_passing {r['message_passing']['ms_median']:.2f} ms "
              f"({r['message_passing']['ms_min']:.2f}..{r['message_passing']['ms_max']:.2f}), {r['message_passing']['peak_bytes'] / 2**20:.0f} MiB | "
              f"out rel L2 {r['out_rel_l2']:.2e}, grad x rel L2 {r['grad_x_rel_l2']:.2e} (row median {r['grad_x_row_rel_median']:.2e}, "
              f"{r['grad_x_rows_above_1e-4']} of {r['n_src']} rows above 1e-4)", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
