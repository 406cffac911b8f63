#!/usr/bin/env python3
"""Forward + backward of the operator route's three differentiable operators (ops.scatter_max as MessagePassing.propagate uses
it, ops.global_max_pool, ops.knn_interpolate: HIP, csrc/p2w_grad.hip) against the same operators written in plain PyTorch on the
same device (scatter_reduce(amax), index_add_) - what a user without torch-scatter / torch-geometric would otherwise write.

Shapes: the levels one 8 x 16384-point batch (bench.py, BASELINE configs[1]) produces - sizes, edge counts and neighbour tables
are read from the engine's geometry of the synthetic voxels; the widths are the reference model's at bench.C.  The searches are
not timed (both sides get the same neighbour tables).  Each repeat times one forward + backward with device events on inputs
it has not touched for at least 512 MiB of other traffic (the Infinity Cache holds 256 MiB), after a warm-up of every shape.

    python tools/ops_backward_bench.py [--repeats 9] [--out profiles/ops_backward_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pointstowood_amd import Net, ops  # noqa: E402
from pointstowood_amd import synthetic_weights as weights  # noqa: E402

ROTATE_BYTES = 512 << 20


def torch_segment_max(x, index, nb):
    out = torch.zeros((nb, x.shape[1]), dtype=x.dtype, device=x.device)
    return out.scatter_reduce(0, index[:, None].expand_as(x), x, reduce="amax", include_self=False)


def torch_interpolate(x, q, j, w, m):
    num = torch.zeros((m, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, q, x[j] * w[:, None])
    den = torch.zeros((m, 1), dtype=x.dtype, device=x.device).index_add_(0, q, w[:, None])
    return num / den


def measure(fn, inputs, grads, repeats):
    """fn(x) -> out; out.backward(g).  Rotates over `inputs` (copies of one tensor).  Milliseconds per forward + backward."""
    def once(i):
        x = inputs[i % len(inputs)]
        x.grad = None
        fn(x).backward(grads[i % len(grads)])
    for i in range(len(inputs) + 1):
        once(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        once(i + 1)
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=repeats)


def copies(rows, cols, dev, seed):
    """Enough copies of a [rows, cols] fp32 tensor that a rotation touches ROTATE_BYTES before it returns to one (2 .. 8)."""
    n = max(2, min(8, -(-ROTATE_BYTES // max(1, rows * cols * 4))))
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.randn((rows, cols), generator=g, device=dev)
    return [base.clone().requires_grad_() for _ in range(n)]


def compare(entry, name, hip, plain, rows, cols, out_rows, dev, repeats, seed):
    xs = copies(rows, cols, dev, seed)
    gs = [t.detach()[:1].new_empty((out_rows, cols)).normal_() for t in xs[:2]]
    a = measure(hip, xs, gs, repeats)
    b = measure(plain, xs, gs, repeats)
    # same seeded input, same upstream gradient: the two gradients agree to fp32 rounding (ties aside: randn has none)
    xs[0].grad = None; hip(xs[0]).backward(gs[0]); g_hip = xs[0].grad.clone()
    xs[0].grad = None; plain(xs[0]).backward(gs[0]); g_plain = xs[0].grad
    err = float((g_hip - g_plain).abs().max() / g_plain.abs().max().clamp(min=1e-30))
    entry[name] = dict(shape=dict(rows=rows, cols=cols, out_rows=out_rows), hip=a, plain_pytorch=b,
                       hip_over_plain=a["median_ms"] / b["median_ms"], grad_max_rel_diff=err)
    print(f"{name:28s} [{rows} x {cols}] -> {out_rows}:  hip {a['median_ms']:8.3f} ms ({a['min_ms']:.3f} .. {a['max_ms']:.3f})   "
          f"plain {b['median_ms']:8.3f} ms ({b['min_ms']:.3f} .. {b['max_ms']:.3f})   ratio {entry[name]['hip_over_plain']:.2f}   "
          f"grad diff {err:.1e}", flush=True)
    del xs, gs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ops_backward_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ops_backward_bench needs an MI355X: there is nothing to measure on a host")
    dev = torch.device("cuda", 0)
    net = Net(1, C=bench.C, k=bench.K_NBR)
    net.load_state_dict(weights.synth_state_dict(1, bench.C, seed=0))
    net = net.to(dev).eval()
    d = bench.make_batch(0, dev)
    net(d)
    geo = net._engine.geometry(d.pos, d.reflectance, d.ptr.to(torch.int32), d.sf)
    torch.cuda.synchronize()
    C, lv = bench.C, geo.levels
    M = [geo.N] + [lv[l].n for l in (1, 2, 3)]
    res = {"workload": f"one batch of {geo.B} x {bench.NPTS} points (bench.py configs[1]); level sizes {M}", "C": C, "ops": {}}
    ent = res["ops"]
    # the max aggregation of SA1..SA3 (pointnet.py:108): E_l messages of local_nn's output width, grouped by target
    for l, width in ((1, 4 * C), (2, 8 * C), (3, 16 * C)):
        deg = lv[l].deg[: M[l]].long()
        index = torch.repeat_interleave(torch.arange(M[l], device=dev), deg)
        E = int(index.numel())
        compare(ent, f"scatter_max SA{l}", lambda x: ops.scatter_max(x, index, dim=0, dim_size=M[l])[0],
                lambda x: torch_segment_max(x, index, M[l]), E, width, M[l], dev, args.repeats, 10 + l)
    # global_max_pool (model.py:136) over level 3
    b3 = lv[3].batch[: M[3]].long()
    compare(ent, "global_max_pool", lambda x: ops.global_max_pool(x, b3, size=geo.B), lambda x: torch_segment_max(x, b3, geo.B),
            M[3], 16 * C, geo.B, dev, args.repeats, 20)
    # knn_interpolate of FP4..FP1 (model.py:149): coarse -> fine, k = 2 (FP4: the voxel's one global row, k = 1)
    for name, f in (("FP4", 3), ("FP3", 2), ("FP2", 1), ("FP1", 0)):
        m = M[f]
        rf = (geo.sorted0 if f == 0 and geo.rows0_sorted else lv[f].xyzr)[:m].contiguous()   # the rows fp_nbr[0] is in
        if f == 3:
            nc, kw = geo.B, 1
            nbr, dg = lv[3].batch[:m].to(torch.int32).reshape(m, 1).contiguous(), torch.ones(m, dtype=torch.int32, device=dev)
            rc = torch.zeros((nc, 4), device=dev)
        else:
            nc, kw = M[f + 1], 2
            nbr, dg = (t[:m].contiguous() for t in geo.fp_nbr[f])
            rc = lv[f + 1].xyzr[:nc].contiguous()
        mask = torch.arange(kw, device=dev)[None, :] < dg[:, None]
        q = torch.arange(m, device=dev)[:, None].expand(m, kw)[mask]
        j = nbr[mask].long()
        w = 1.0 / ((rc[j, :3] - rf[q, :3]) ** 2).sum(1).clamp(min=1e-16)
        compare(ent, f"knn_interpolate {name}", lambda x: ops._KnnInterpolate.apply(x, rc, rf, nbr, dg, kw),
                lambda x: torch_interpolate(x, q, j, w, m), nc, 16 * C, m, dev, args.repeats, 30 + f)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
