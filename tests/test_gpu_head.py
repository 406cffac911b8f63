"""The head behind conv1 for training on the GPU: p2w_bn_relu_rowdot / _bwd (csrc/p2w_head.hip) through the C ABI - the statistics and
the backward held EXACTLY to p2w_bn_chain / p2w_bn_chain_bwd (L = 1, ReLU; the backward fed the materialised gradient fl(g[r] w[c])),
the two access widths held to each other bit for bit, everything held to tests/head_ref.py's float64 references within its derived
caps - and ops.bn_relu_rowdot under autograd.

"Equal" is equal values and equal NaN positions (_same); where bits are compared, NaNs are left out (a NaN's sign and payload are
not pinned)."""

import pytest
import torch

from tests import head_ref as R

pytestmark = pytest.mark.gpu

EINVAL, ENULL, EALIGN, EWORKSPACE = -1, -2, -3, -4
NAN = float("nan")


@pytest.fixture(scope="module")
def H():
    from pointstowood_amd import ops
    return ops


@pytest.fixture(scope="module")
def L():
    from pointstowood_amd._lib import lib
    return lib()


def _abi():
    from pointstowood_amd._lib import BnStage, ptr, stream
    return BnStage, ptr, stream


def _same(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def _same_bits(a, b):
    ok = ~torch.isnan(a)
    return _same(a, b) and torch.equal(a.contiguous().view(torch.int32)[ok], b.contiguous().view(torch.int32)[ok])


def _pitched(t, ld):
    buf = torch.full((t.shape[0], ld), NAN, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf


def _run(L, c, ld, chain=False):
    """Forward and backward through the ABI with z and dz pitched to ld: p2w_bn_relu_rowdot / _bwd, or (chain) p2w_bn_chain / _bwd with
    one ReLU stage, its backward fed G = fl(g[r] w[c]).  One guard row or element of NaN behind every output."""
    BnStage, ptr, stream = _abi()
    (M, C) = c["z"].shape
    z = _pitched(c["z"], ld)
    gamma, beta, w, bias, g = (c[k].cuda() for k in ("gamma", "beta", "w", "bias", "g"))
    rm, rv = (torch.cat([c[k], torch.full((1,), NAN)]).cuda() for k in ("rm", "rv"))
    dz = torch.full((M + 1, ld), NAN, device="cuda")
    mean, invstd, dgamma, dbeta, dw = (torch.full((C + 1,), NAN, device="cuda") for _ in range(5))
    dbias, logit = torch.full((2,), NAN, device="cuda"), torch.full((M + 1,), NAN, device="cuda")
    r = {}
    if chain:
        need = int(L.p2w_bn_chain_ws_size(M, C, 1))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        out, G = torch.full((M, ld), NAN, device="cuda"), _pitched(R.materialised_gradient(c), ld)
        arr = (BnStage * 1)()
        arr[0] = BnStage(None, None, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), R.MOMENTUM, R.BN_EPS, 1)
        assert L.p2w_bn_chain(ptr(z), ld, None, 0, arr, 1, M, C, ptr(out), ld, ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
        assert L.p2w_bn_chain_bwd(ptr(G), ld, ptr(z), ld, None, 0, arr, 1, ptr(mean), ptr(invstd), M, C, ptr(dz), ld, None, 0, ptr(dgamma),
                                  ptr(dbeta), None, None, ptr(ws), need, stream()) == 0
        r["u"] = out[:, :C]
    else:
        need = int(L.p2w_bn_relu_rowdot_ws_size(M, C))
        assert need > 0 and need % 256 == 0
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert L.p2w_bn_relu_rowdot(ptr(z), ld, ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(rm), ptr(rv), R.MOMENTUM, R.BN_EPS, M, C,
                                    ptr(logit), ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
        assert L.p2w_bn_relu_rowdot_bwd(ptr(g), ptr(z), ld, ptr(gamma), ptr(beta), ptr(w), ptr(mean), ptr(invstd), M, C, ptr(dz), ld,
                                        ptr(dgamma), ptr(dbeta), ptr(dw), ptr(dbias), ptr(ws), need, stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(logit[M])) and bool(torch.isnan(dw[C])) and bool(torch.isnan(dbias[1]))
        r.update(logit=logit[:M], dw=dw[:C], dbias=dbias[:1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz[M]).all()) and bool(torch.isnan(dz[:, C:]).all())
    for t in (mean, invstd, dgamma, dbeta, rm, rv):
        assert bool(torch.isnan(t[C]))
    r.update(dz=dz[:M, :C], mean=mean[:C], invstd=invstd[:C], dgamma=dgamma[:C], dbeta=dbeta[:C], running_mean=rm[:C], running_var=rv[:C])
    return {k: v.contiguous().cpu() for k, v in r.items()}


CHAIN_KEYS = ("mean", "invstd", "running_mean", "running_var", "dz", "dgamma", "dbeta")


@pytest.mark.parametrize("C", [1, 4, 67, 132, 520])
@pytest.mark.parametrize("M", [2, 31, 33, 257])
def test_head_equals_the_chain_and_both_widths_agree(L, M, C):
    """mean, invstd and the running statistics bit for bit against p2w_bn_chain (L = 1, ReLU) on the same z; dz, dgamma, dbeta bit for bit
    against p2w_bn_chain_bwd fed the materialised gradient g[r] w[c]; the logits of the chain's u in the documented order.  M = 2 / 31 /
    33 / 257 are below, across and above one work item of 32 rows, and 1, 1, 3 and 17 waves of 16 rows; C = 1 and 67 run with 4-byte
    accesses, 4, 132 and 520 with 16-byte accesses (pitch C + 8) and with 4-byte accesses (pitch C + 3): the same bits in every number.
    C = 520 gives the first lanes three passes.  Planted (C >= 5): a zero-variance column, gamma = 0, gamma < 0, w = 0, a NaN column."""
    for nan in ((False, True) if C >= 5 else (False,)):
        c = R.case(M, C, nan=nan)
        first = None
        for ld in ([C + 8, C + 3] if C % 4 == 0 else [C + 3]):
            got, want = _run(L, c, ld), _run(L, c, ld, chain=True)
            for k in CHAIN_KEYS:
                assert _same_bits(got[k], want[k]), (k, ld)
            assert _same_bits(got["logit"], _ordered_rowdot(want["u"], c["w"], c["bias"])), ld
            if first is None:
                first = got
            for k in got:
                assert _same_bits(got[k], first[k]), (k, ld)
        plain = R.composition(c["z"], c["gamma"], c["beta"], c["w"], c["bias"], c["rm"].clone(), c["rv"].clone())
        assert torch.equal(torch.isnan(first["logit"]), torch.isnan(plain))
        assert bool(torch.isnan(first["logit"]).all()) == nan                   # a NaN poisons its column, and w NaN is a NaN in every row
        if C >= 5:
            assert bool((first["dz"][:, R.GAMMA_ZERO] == 0).all()) and bool((first["dz"][:, R.W_ZERO] == 0).all())
            assert float(first["mean"][R.ZERO_VAR]) == 0.25 and float(first["dw"][R.ZERO_VAR]) != 0.0
            assert bool(torch.isnan(first["dz"][:, R.NAN_COL]).all()) == nan


def _ordered_rowdot(u, w, bias):
    """include/p2w.h's summation order in torch fp32 on the CPU: lane l owns the columns 256 p + 4 l + e; lanes start at +0 and add
    their columns in ascending order; butterfly over the 64 lanes (partner l ^ 32, ^ 16, .. ^ 1); bias last."""
    M, C = u.shape
    acc = torch.zeros(M, 64)
    for c0 in range(0, C, 256):
        for e in range(4):
            cols = torch.arange(64) * 4 + c0 + e
            ok = cols < C
            prod = torch.zeros(M, 64)
            prod[:, ok] = u[:, cols[ok]] * w[cols[ok]]
            acc = torch.where(ok[None, :], acc + prod, acc)
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0] + bias


@pytest.mark.parametrize("M,C", [(257, 132), (257, 520), (33, 67)])
def test_head_against_fp64(L, M, C):
    """Logits, mean, invstd, running statistics, dz, dgamma, dbeta, dw and dbias against tests/head_ref.py's float64 references, within
    its derived caps (finite case; the planted zero-variance, gamma = 0, gamma < 0 and w = 0 columns are in it)."""
    c = R.case(M, C)
    got = _run(L, c, C + 8 if C % 4 == 0 else C + 3)
    ref, caps = R.forward_reference(c, got["mean"], got["invstd"])
    bref, bcaps = R.backward_reference(c, got["mean"], got["invstd"])
    ref.update(bref), caps.update(bcaps)
    ratios = {k: R.ratio(got[k].reshape(ref[k].shape), ref[k], caps[k]) for k in ref}
    print(f"HEAD_RATIO M {M} C {C} " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0
    assert float(got["dz"].abs().max()) > 0 and float(got["dw"].abs().max()) > 0


def test_head_guards_launch_nothing(L):
    """P2W_ENULL, P2W_EALIGN (the workspace), P2W_EINVAL (M = 1, C = 0, a pitch below C, eps < 0, momentum > 1) and P2W_EWORKSPACE of both
    entry points: the NaN-filled outputs stay NaN and the running statistics stay put.  The workspace size is what the chain's one-stage
    workspace and one double per work item need.  Then the good calls write."""
    _, ptr, stream = _abi()
    M, C = 70, 8
    z, g = torch.randn(M, C + 4, device="cuda"), torch.randn(M, device="cuda")
    gamma, beta, w = (torch.rand(C, device="cuda") + 0.5 for _ in range(3))
    bias = torch.ones(1, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    dz, logit = torch.full((M, C + 4), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")
    mean, invstd, dgamma, dbeta, dw = (torch.full((C,), NAN, device="cuda") for _ in range(5))
    dbias = torch.full((1,), NAN, device="cuda")
    need = int(L.p2w_bn_relu_rowdot_ws_size(M, C))
    items = (M + 31) // 32
    assert need == int(L.p2w_bn_chain_ws_size(M, C, 1)) + 256 * ((8 * items + 255) // 256)
    assert L.p2w_bn_relu_rowdot_ws_size(1, C) == 0 and L.p2w_bn_relu_rowdot_ws_size(M, 0) == 0
    assert L.p2w_bn_relu_rowdot_ws_size(2 ** 31 - 1, 1) == 0 and L.p2w_bn_relu_rowdot_ws_size(2 ** 30, 512) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    s = stream()

    def fwd(z_=ptr(z), ldz=C + 4, gamma_=ptr(gamma), beta_=ptr(beta), w_=ptr(w), bias_=ptr(bias), rm_=ptr(rm), rv_=ptr(rv), mom=0.1, eps=1e-5,
            M_=M, C_=C, logit_=ptr(logit), mean_=ptr(mean), invstd_=ptr(invstd), ws_=ptr(ws), wsb=need):
        return L.p2w_bn_relu_rowdot(z_, ldz, gamma_, beta_, w_, bias_, rm_, rv_, mom, eps, M_, C_, logit_, mean_, invstd_, ws_, wsb, s)

    def bwd(g_=ptr(g), z_=ptr(z), ldz=C + 4, gamma_=ptr(gamma), beta_=ptr(beta), w_=ptr(w), mean_=ptr(mean), invstd_=ptr(invstd), M_=M, C_=C,
            dz_=ptr(dz), lddz=C + 4, dgamma_=ptr(dgamma), dbeta_=ptr(dbeta), dw_=ptr(dw), dbias_=ptr(dbias), ws_=ptr(ws), wsb=need):
        return L.p2w_bn_relu_rowdot_bwd(g_, z_, ldz, gamma_, beta_, w_, mean_, invstd_, M_, C_, dz_, lddz, dgamma_, dbeta_, dw_, dbias_, ws_,
                                        wsb, s)

    for name in ("z_", "gamma_", "beta_", "w_", "bias_", "rm_", "rv_", "logit_", "mean_", "invstd_", "ws_"):
        assert fwd(**{name: None}) == ENULL, name
    for name in ("g_", "z_", "gamma_", "beta_", "w_", "mean_", "invstd_", "dz_", "dgamma_", "dbeta_", "dw_", "dbias_", "ws_"):
        assert bwd(**{name: None}) == ENULL, name
    assert fwd(ws_=ptr(ws) + 4) == EALIGN and bwd(ws_=ptr(ws) + 8) == EALIGN
    assert fwd(M_=1) == EINVAL and fwd(C_=0) == EINVAL and fwd(ldz=C - 1) == EINVAL and fwd(M_=-3) == EINVAL
    assert fwd(eps=-1.0) == EINVAL and fwd(mom=1.5) == EINVAL and fwd(mom=NAN) == EINVAL
    assert bwd(M_=1) == EINVAL and bwd(C_=0) == EINVAL and bwd(ldz=4) == EINVAL and bwd(lddz=C - 1) == EINVAL
    assert fwd(wsb=need - 1) == EWORKSPACE and fwd(wsb=0) == EWORKSPACE and bwd(wsb=need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    for t in (dz, logit, mean, invstd, dgamma, dbeta, dw, dbias):
        assert bool(torch.isnan(t).all())
    assert bool((rm == 0).all()) and bool((rv == 1).all())
    assert fwd() == 0
    assert bwd() == 0
    torch.cuda.synchronize()
    for t in (dz[:, :C], logit, mean, invstd, dgamma, dbeta, dw, dbias):
        assert bool(torch.isfinite(t).all())
    assert bool(torch.isnan(dz[:, C:]).all())
    assert bool((rm != 0).any()) and bool((rv != 1).any())
    assert abs(float(dbias) - float(g.double().sum())) <= 1e-5 * float(g.abs().sum())


# ------------------------------------------------------------------------------------------------ the operator
def _modules(c, dtype=torch.float32, **kw):
    C = c["z"].shape[1]
    bn = torch.nn.BatchNorm1d(C, **kw).cuda()
    conv2 = torch.nn.Conv1d(C, 1, 1).cuda()
    with torch.no_grad():
        if bn.affine:
            bn.weight.copy_(c["gamma"]), bn.bias.copy_(c["beta"])
        if bn.track_running_stats:
            bn.running_mean.copy_(c["rm"]), bn.running_var.copy_(c["rv"])
        conv2.weight.copy_(c["w"].reshape(1, C, 1)), conv2.bias.copy_(c["bias"])
    return bn.to(dtype), conv2.to(dtype)


@pytest.mark.parametrize("M,C", [(33, 67), (257, 132)])
def test_operator_equals_the_abi(H, L, M, C):
    """ops.bn_relu_rowdot under autograd: the logits, the running statistics, num_batches_tracked and the five gradients are the C
    ABI's, in the parameters' shapes ([1, C, 1] for conv2.weight)."""
    c = R.case(M, C)
    want = _run(L, c, C)
    bn, conv2 = _modules(c)
    z = c["z"].cuda().requires_grad_()
    out = H.bn_relu_rowdot(z, bn, conv2.weight, conv2.bias)
    assert out.shape == (M,) and out.dtype == torch.float32
    out.backward(c["g"].cuda())
    assert _same_bits(out.detach().cpu(), want["logit"])
    assert conv2.weight.grad.shape == (1, C, 1) and conv2.bias.grad.shape == (1,)
    for got, k in ((z.grad, "dz"), (bn.weight.grad, "dgamma"), (bn.bias.grad, "dbeta"), (conv2.weight.grad.reshape(-1), "dw"),
                   (conv2.bias.grad, "dbias"), (bn.running_mean, "running_mean"), (bn.running_var, "running_var")):
        assert _same_bits(got.detach().cpu(), want[k]), k
    assert int(bn.num_batches_tracked) == 1


def test_operator_modes_and_errors(H):
    c = R.case(33, 67)
    z = c["z"].cuda()
    # fp16 z under autocast: fp32 compute, an fp16 gradient
    bn, conv2 = _modules(c)
    zh = z.half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = H.bn_relu_rowdot(zh, bn, conv2.weight, conv2.bias)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert zh.grad.dtype == torch.float16 and bn.weight.grad.dtype == torch.float32 and conv2.weight.grad.dtype == torch.float32
    bn2, conv2b = _modules(c)
    ref = H.bn_relu_rowdot(zh.detach().float().requires_grad_(), bn2, conv2b.weight, conv2b.bias)
    assert _same_bits(out.detach().cpu(), ref.detach().cpu())
    # no_grad: nothing saved, the statistics move
    bn2, conv2b = _modules(c)
    ref = H.bn_relu_rowdot(z.clone().requires_grad_(), bn2, conv2b.weight, conv2b.bias)
    assert ref.grad_fn is not None
    bn, conv2 = _modules(c)
    with torch.no_grad():
        out = H.bn_relu_rowdot(z.clone().requires_grad_(), bn, conv2.weight, conv2.bias)
    assert out.grad_fn is None and not out.requires_grad
    assert int(bn.num_batches_tracked) == 1 and not torch.equal(bn.running_mean.cpu(), c["rm"])
    assert _same_bits(out.cpu(), ref.detach().cpu())
    # weight [1, C] is accepted
    bn, conv2 = _modules(c)
    out2 = H.bn_relu_rowdot(z, bn, conv2.weight[:, :, 0], conv2.bias)
    assert _same_bits(out2.detach().cpu(), ref.detach().cpu())
    # eval mode: the plain composition on the running statistics
    bn, conv2 = _modules(c)
    bn.eval()
    got = H.bn_relu_rowdot(z, bn, conv2.weight, conv2.bias)
    want = torch.nn.functional.linear(torch.relu(bn(z)), conv2.weight[:, :, 0], conv2.bias)[:, 0]
    assert torch.equal(got, want) and int(bn.num_batches_tracked) == 0
    # what it refuses
    for kw in (dict(affine=False), dict(track_running_stats=False), dict(momentum=None)):
        bn, conv2 = _modules(c, **kw)
        with pytest.raises(NotImplementedError):
            H.bn_relu_rowdot(z, bn, conv2.weight, conv2.bias)
    bn, conv2 = _modules(c)
    with pytest.raises(ValueError):
        H.bn_relu_rowdot(z[:1], bn, conv2.weight, conv2.bias)
    with pytest.raises(RuntimeError):
        H.bn_relu_rowdot(z[:, :8], bn, conv2.weight, conv2.bias)
    with pytest.raises(RuntimeError):
        H.bn_relu_rowdot(z, bn, torch.zeros(2, 67, device="cuda"), torch.zeros(2, device="cuda"))
    with pytest.raises(TypeError):
        H.bn_relu_rowdot(z, torch.nn.Identity(), conv2.weight, conv2.bias)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_operator_no_worse_than_the_plain_composition(H):
    """Against float64 (head64 on the same fp32 inputs): the relative L2 error of the logits and of each gradient is at most 8 x the
    plain fp32 composition's own error on the GPU - the project's rule for a fused route (tests/test_gpu_bn_chain.py)."""
    M, C = 257, 132
    c = R.case(M, C)
    r64 = R.head64(c["z"], c["gamma"], c["beta"], c["w"], c["bias"], c["g"])
    res = {}
    for fused in (True, False):
        bn, conv2 = _modules(c)
        z = c["z"].cuda().requires_grad_()
        if fused:
            out = H.bn_relu_rowdot(z, bn, conv2.weight, conv2.bias)
        else:
            out = torch.nn.functional.linear(torch.relu(bn(z)), conv2.weight[:, :, 0], conv2.bias)[:, 0]
        out.backward(c["g"].cuda())
        res[fused] = dict(logit=out.detach(), dz=z.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, dw=conv2.weight.grad.reshape(-1),
                          dbias=conv2.bias.grad)
    for k in res[True]:
        e_f, e_p = _rel_l2(res[True][k].cpu(), r64[k]), _rel_l2(res[False][k].cpu(), r64[k])
        print(f"HEAD_OP_ERR {k} fused {e_f:.3e} plain {e_p:.3e}")
        assert e_f <= 8 * e_p, (k, e_f, e_p)
