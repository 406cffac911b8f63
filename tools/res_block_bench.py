#!/usr/bin/env python3
"""Training-mode ``ops.InvertedResidualBlock`` (four GEMMs and four ``bn_chain`` calls on rows) beside a block of the reference's
structure in plain PyTorch (``Conv1d`` / ``BatchNorm1d`` / ``ReLU`` on the transposed [1, C, M] view, as a user of the reference has it).

    python tools/res_block_bench.py [--repeat 10] [--commit <hash>] [--out profiles/res_block_bench.json]

The three level shapes (M, C) of an 8 x 16 384-point batch; forward + backward of ``sum(out * g)`` with gradients to x and to every
parameter, timed with device events around the whole step; the method is ``tools/bn_max_bench.py``'s: two warm-up steps per route,
then ``--repeat`` steps that alternate between the routes and rotate over three copies of the inputs; median, minimum and maximum.
``peak_bytes`` is ``torch.cuda.max_memory_allocated`` over a step minus what was allocated before it (inputs and parameters).
``*_rel_l2`` compare the two routes' results on the same inputs.  ``wide_tensor_bytes_derived`` = M 4C 4 is one [M, 4C] fp32 tensor;
``passes_derived`` are the passes over such a tensor between the GEMMs of the block's middle stretch (three BatchNorms, three ReLUs, one
depthwise convolution), counted from the operations, not measured.  No ratio is asserted: what is measured is what is written.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import ops  # noqa: E402
from tools.bn_max_bench import alternate  # noqa: E402
from tools.conv_train_bench import COPIES, rel_l2  # noqa: E402

LEVELS = [(65536, 128), (32768, 256), (16384, 512)]
# the stretch between conv.0.pointwise_conv and conv.3.pointwise_conv, passes over an [M, 4C] tensor (README, "derived")
PASSES_PLAIN = {"forward": 3 * 3 + 3 * 2 + 2, "backward": 3 * 5 + 3 * 3 + 5}
PASSES_FUSED = {"forward": 3 + 2, "backward": 3 * 2 + 3}


class _PlainSeparable(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.depthwise_conv = torch.nn.Conv1d(c, c, kernel_size=1, groups=c)
        self.depthwise_bn = torch.nn.BatchNorm1d(c)
        self.pointwise_conv = torch.nn.Conv1d(c, c, kernel_size=1)
        self.pointwise_bn = torch.nn.BatchNorm1d(c)

    def forward(self, x):
        x = torch.relu_(self.depthwise_bn(self.depthwise_conv(x)))
        return torch.relu_(self.pointwise_bn(self.pointwise_conv(x)))


class PlainBlock(torch.nn.Module):
    """The block as plain PyTorch modules on the [1, C, M] view, with the submodule names of ``ops.InvertedResidualBlock`` so that one
    state dict serves both."""

    def __init__(self, c, expansion_factor=4):
        super().__init__()
        from torch.nn import BatchNorm1d, Conv1d, ReLU, Sequential
        e = c * expansion_factor
        self.expand = Sequential(Conv1d(c, e, kernel_size=1), BatchNorm1d(e), ReLU())
        self.conv = Sequential(_PlainSeparable(e), BatchNorm1d(e), ReLU(), _PlainSeparable(e), BatchNorm1d(e))
        self.project = Sequential(Conv1d(e, c, kernel_size=1), BatchNorm1d(c))
        self.shortcut = Sequential()

    def forward(self, x):
        out = self.project(self.conv(self.expand(x.t().unsqueeze(0))))
        return torch.relu(out.squeeze(0).t() + x)


def block_step(block, d):
    """One forward + backward; (ms, peak bytes above what was allocated before, out, grad_x)."""
    block.zero_grad(set_to_none=True)
    x = d["x"].detach().requires_grad_()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = block(x)
    (out * d["g"]).sum().backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out.detach(), x.grad


def run_level(shape, repeat, dev):
    M, C = shape
    g = torch.Generator(device=dev).manual_seed(M + C)
    sets = [dict(x=torch.randn(M, C, device=dev, generator=g), g=torch.randn(M, C, device=dev, generator=g)) for _ in range(COPIES)]
    torch.manual_seed(0)
    fused = ops.InvertedResidualBlock(C, C).to(dev).train()
    plain = PlainBlock(C).to(dev).train()
    plain.load_state_dict(fused.state_dict())
    first, res_block = alternate({"fused": fused, "plain": plain}, block_step, sets, repeat)
    wide = M * 4 * C * 4
    res = {"M": M, "C": C, "repeat": repeat, "rotating_inputs": COPIES, "wide_tensor_bytes_derived": wide,
           "passes_derived": {"plain": PASSES_PLAIN, "fused": PASSES_FUSED}, "block": res_block,
           "out_rel_l2": rel_l2(first["fused"][2], first["plain"][2]), "grad_x_rel_l2": rel_l2(first["fused"][3], first["plain"][3])}
    res["time_ratio_plain_over_fused"] = res_block["plain"]["ms_median"] / res_block["fused"]["ms_median"]
    res["peak_ratio_plain_over_fused"] = res_block["plain"]["peak_bytes"] / res_block["fused"]["peak_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("res_block_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "levels": []}
    for li in a.levels:
        r = run_level(LEVELS[li], a.repeat, dev)
        res["levels"].append(r)
        f, p = r["block"]["fused"], r["block"]["plain"]
        print(f"level {li} M={r['M']} C={r['C']}: fused {f['ms_median']:.2f} ms ({f['ms_min']:.2f}..{f['ms_max']:.2f}), "
              f"{f['peak_bytes'] / 2**20:.0f} MiB | plain {p['ms_median']:.2f} ms ({p['ms_min']:.2f}..{p['ms_max']:.2f}), "
              f"{p['peak_bytes'] / 2**20:.0f} MiB | plain / fused {r['time_ratio_plain_over_fused']:.2f}x, "
              f"out rel L2 {r['out_rel_l2']:.2e}, grad x rel L2 {r['grad_x_rel_l2']:.2e}", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
