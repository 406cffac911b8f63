"""The maths of the training route of ops.PointNetConv, pinned on the CPU in float64 before any kernel runs: the hoisted
formulation (tests/conv_train_ref.py) against the reference-style message() + local_nn composition over oracle/ops.py, and the
kernel references of the GPU tests against that formulation."""
import copy
import json
import os

import torch

from oracle import ops as O
from tests import conv_train_ref as R
from tests.test_gpu_ops_backward import _OracleMessagePassing, _mlp, _ref_style_conv

NOISE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_train", "noise.json")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _case(seed=3):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 40, (60,), generator=g)
    deg[[0, 9]] = 0
    i = torch.repeat_interleave(torch.arange(60), deg)
    j = torch.randint(0, 90, (i.numel(),), generator=g)
    return dict(ei=torch.stack([j, i], 0), x=torch.randn(100, 8, generator=g, dtype=torch.float64),
                pos_src=torch.rand(100, 4, generator=g, dtype=torch.float64), pos_dst=torch.rand(60, 4, generator=g, dtype=torch.float64),
                g=torch.randn(60, 32, generator=g, dtype=torch.float64))


def _run(fn, nn, c):
    x, ps = c["x"].clone().requires_grad_(), c["pos_src"].clone().requires_grad_()
    out = fn(nn, x, ps)
    (out * c["g"]).sum().backward()
    bn = nn[1][2]
    return dict(out=out.detach(), x=x.grad, pos_src=ps.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                **{k: p.grad for k, p in nn.named_parameters()})


def test_hoisted_formulation_equals_the_reference_composition_in_fp64():
    """Output, running statistics and every gradient (x, all of pos_src - column 3 included -, every parameter) of the hoisted
    formulation equal those of message() + local_nn over oracle.ops within 1e-12 relative, in training and in eval mode."""
    c = _case()
    for train in (True, False):
        nn = _mlp([12, 16, 32], seed=8).double().train(train)
        a, b = copy.deepcopy(nn), copy.deepcopy(nn)
        ref = _run(lambda m, x, ps: _ref_style_conv(_OracleMessagePassing, O.scatter_max, m).train(train)(x, (ps, c["pos_dst"]), c["ei"]), a, c)
        got = _run(lambda m, x, ps: R.hoisted_conv(x, ps, c["pos_dst"], c["ei"], m), b, c)
        assert set(got) == set(ref) and len(ref) == 11
        for k in ref:
            assert _rel(got[k], ref[k]) <= 1e-12, (train, k, _rel(got[k], ref[k]))
        assert float(ref["pos_src"][:, 3].abs().max()) > 0 and float(ref["x"].abs().max()) > 0
        assert bool((ref["out"][[0, 9]] == 0).all())


def test_kernel_references_agree_with_the_formulation():
    """forward_case's H1 is the hoisted formulation's layer 1 (same geo, same ReLU), the planted rows are there, and
    backward_reference is the autograd gradient of sum(H1 * gH) with respect to P, Wg and the reflectance."""
    c, f = R.edge_case(), R.forward_case(6)
    deg = c["deg"]
    assert deg[:5].tolist() == [0, 1, 32, 33, 100] and int(c["ptr"][-1]) == c["E"] == f["H1"].shape[0]
    cnt = torch.bincount(c["src"].long(), minlength=R.N_SRC)
    assert 2900 <= int(cnt[R.HUB]) <= 3100 and bool((cnt[587:] == 0).all()) and int((cnt == 0).sum()) >= 13
    coincident = c["i"] == R.COINCIDENT
    assert bool((f["geo"][coincident, :3] == 0).all()) and bool((f["cap_geo"][coincident, :3] == 0).all())
    P, Wg, ps = f["P"].double().requires_grad_(), f["Wg"].double().requires_grad_(), c["pos_src"].double().requires_grad_()
    j, i = c["src"].long(), c["i"]
    rel = ps[j, :3].detach() - c["pos_dst"].double()[i, :3]
    maxd = O.scatter_max(rel.norm(dim=1, keepdim=True), i, dim=0, dim_size=R.M_DST)[0]
    geo = torch.cat([rel / (maxd[i] + R.E8), ps[j, 3:4]], 1)
    H1 = torch.relu(P[j] + geo @ Wg)
    assert _rel(H1.detach(), f["H1"]) <= 1e-14 and _rel(geo.detach(), f["geo"]) <= 1e-14
    gH = torch.randn(H1.shape, generator=torch.Generator().manual_seed(1))
    (H1 * gH.double()).sum().backward()
    (gP, gR, gWg), caps = R.backward_reference(gH, H1.detach().float(), geo.detach().float(), c["src"], f["Wg"], R.N_SRC)
    # (the reference's mask and geo are the fp32 roundings it is handed: rows whose pre-activation rounds to 0 aside, the same sums)
    assert _rel(gP, P.grad) <= 1e-6 and _rel(gR, ps.grad[:, 3]) <= 1e-6 and _rel(gWg, Wg.grad) <= 1e-6
    assert bool((ps.grad[:, :3] == 0).all())
    assert all(bool((cap >= 0).all()) for cap in caps) and bool((caps[0][587:] == 0).all()) and bool((caps[1][587:] == 0).all())


def test_recorded_noise_covers_every_compared_tensor():
    noise = json.load(open(NOISE_JSON))["rel_l2"]
    nn = _mlp([12, 16, 32], seed=8)
    want = {"out", "x", "pos_src_refl", "running_mean", "running_var"} | {f"local_nn.{k}" for k, _ in nn.named_parameters()}
    assert set(noise) == want
    assert all(0 < v < 1e-4 for v in noise.values())
