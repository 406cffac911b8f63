"""p2w_bn_chain / p2w_bn_chain_bwd (csrc/p2w_bnchain.hip) through the C ABI against the float64 references and caps of
tests/bn_chain_ref.py, ops.bn_chain against the plain composition under ordinary autograd, and ops.InvertedResidualBlock against the
float64 composition over oracle/net.py's row-major form with training-mode BatchNorm."""
import copy
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import bn_chain_ref as R
from tests.test_gpu_conv_train import _pitched
from tests.test_gpu_ops_backward import _rel_l2

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


def _pitch(C):
    """A row pitch larger than C that keeps the access width of C."""
    return C + 8 if C % 4 == 0 else C + 3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _device_stages(c):
    """The stages' vectors on the device (the running statistics with a NaN behind them) and the host array the ABI takes."""
    BnStage, ptr, _ = _abi()
    dev, arr = [], (BnStage * len(c["stages"]))()
    for t, st in enumerate(c["stages"]):
        d = {k: None if st[k] is None else st[k].cuda() for k in ("a", "b", "gamma", "beta")}
        d["rm"], d["rv"] = (torch.cat([st[k], torch.full((1,), NAN)]).cuda() for k in ("running_mean", "running_var"))
        arr[t] = BnStage(ptr(d["a"]), ptr(d["b"]), ptr(d["gamma"]), ptr(d["beta"]), ptr(d["rm"]), ptr(d["rv"]), R.MOMENTUM, R.BN_EPS, int(st["relu"]))
        dev.append(d)
    return dev, arr


def _forward(L, c, ld):
    """One call of p2w_bn_chain on case c with every [M, C] tensor pitched to ld (NaN in the padding).  Every output has one row or
    element more than the kernel may write, filled with NaN; returns them on the CPU."""
    _, ptr, stream = _abi()
    (M, C), nL = c["z"].shape, len(c["stages"])
    dev, arr = _device_stages(c)
    z, res = _pitched(c["z"], ld), None if c["res"] is None else _pitched(c["res"], ld)
    out = torch.full((M + 1, ld), NAN, device="cuda")
    mean, invstd = (torch.full((nL * C + 1,), NAN, device="cuda") for _ in range(2))
    need = int(L.p2w_bn_chain_ws_size(M, C, nL))
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_bn_chain(ptr(z), ld, ptr(res), ld, arr, nL, M, C, ptr(out), ld, ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[M]).all()) and bool(torch.isnan(out[:, C:]).all()) and bool(torch.isnan(z[:, C:]).all())
    assert bool(torch.isnan(mean[nL * C])) and bool(torch.isnan(invstd[nL * C]))
    assert all(bool(torch.isnan(d["rm"][C])) and bool(torch.isnan(d["rv"][C])) for d in dev)
    got = dict(out=out[:M, :C], mean=mean[:nL * C].view(nL, C), invstd=invstd[:nL * C].view(nL, C),
               running_mean=torch.stack([d["rm"][:C] for d in dev]), running_var=torch.stack([d["rv"][:C] for d in dev]))
    return {k: v.cpu() for k, v in got.items()}


def _backward(L, c, ld, fwd):
    _, ptr, stream = _abi()
    (M, C), nL = c["z"].shape, len(c["stages"])
    dev, arr = _device_stages(c)
    has_res = c["res"] is not None
    g, z = _pitched(c["g"], ld), _pitched(c["z"], ld)
    outp = _pitched(fwd["out"], ld) if has_res else None
    dz = torch.full((M + 1, ld), NAN, device="cuda")
    dres = torch.full((M + 1, ld), NAN, device="cuda") if has_res else None
    mean, invstd = fwd["mean"].reshape(-1).cuda(), fwd["invstd"].reshape(-1).cuda()
    vecs = [torch.full((nL * C + 1,), NAN, device="cuda") for _ in range(4)]
    need = int(L.p2w_bn_chain_ws_size(M, C, nL))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_bn_chain_bwd(ptr(g), ld, ptr(z), ld, ptr(outp), ld, arr, nL, ptr(mean), ptr(invstd), M, C, ptr(dz), ld, ptr(dres), ld,
                              *[ptr(v) for v in vecs], ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    for t in (dz, dres):
        assert t is None or (bool(torch.isnan(t[M]).all()) and bool(torch.isnan(t[:, C:]).all()))
    assert all(bool(torch.isnan(v[nL * C])) for v in vecs)
    got = dict(dz=dz[:M, :C].cpu(), dres=None if dres is None else dres[:M, :C].cpu())
    got.update({k: v[:nL * C].view(nL, C).cpu() for k, v in zip(("dgamma", "dbeta", "ddw_w", "ddw_b"), vecs)})
    return got


_gpu_fwd = {}


def _forward_once(L, name, C, M):
    if (name, C, M) not in _gpu_fwd:
        _gpu_fwd[name, C, M] = _forward(L, R.case(name, C, M), _pitch(C))
    return _gpu_fwd[name, C, M]


CASES = [(n, C, R.M_ROWS) for n in R.PATTERNS for C in R.WIDTHS] + [(n, C, 2) for n in ("middle", "two_res") for C in (6, 16)]


@pytest.mark.parametrize("name,C,M", CASES)
def test_kernel_forward_against_fp64(L, name, C, M):
    """p2w_bn_chain through the ABI on bn_chain_ref's case (4 133 rows in 130 work items, the last one partial and the reduction's
    second batch entered, or 2 rows; rows pitched with NaN behind them; an all-negative, a constant, a gamma < 0, a gamma = 0, a
    depthwise-weight = 0 and a negative-depthwise-weight column): mean, invstd, the running statistics and out within the caps derived
    in bn_chain_ref's docstring; nothing is written behind the last row or element.  A second call, and one with dense rows, give
    the same bits."""
    c = R.case(name, C, M)
    got = _forward_once(L, name, C, M)
    ref, caps = R.forward_reference(c["z"], c["stages"], c["res"], got["mean"], got["invstd"])
    ratios = {k: R.ratio(got[k], ref[k], caps[k]) for k in ("mean", "invstd", "running_mean", "running_var", "out")}
    last = R.replay32(c["z"], c["stages"], got["mean"], got["invstd"])[-1]["out"]
    if c["res"] is not None:
        t = last + c["res"]
        last = torch.where(t < 0, torch.zeros_like(t), t)
    print(f"BNCHAIN_RATIO forward {name} C={C} M={M} " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + f" replay_equal {torch.equal(_bits(last), _bits(got['out']))}")
    assert max(ratios.values()) <= 1.0
    st = c["stages"]
    if st[0]["a"] is None:
        assert float(got["mean"][0, R.CONST]) == float(c["z"][0, R.CONST])
    if st[0]["relu"] and len(st) > 1 and st[1]["a"] is None:                 # the all-negative column: stage 2 sees zeros
        assert float(got["mean"][1, R.ALL_NEG]) == 0.0
        assert float(got["invstd"][1, R.ALL_NEG]) == float(torch.tensor(1.0 / (R.BN_EPS ** 0.5), dtype=torch.float64).float())
    for other in (_forward(L, c, _pitch(C)), _forward(L, c, C)):
        for k in got:
            assert torch.equal(_bits(got[k]), _bits(other[k])), k


@pytest.mark.parametrize("name,C,M", CASES)
def test_kernel_backward_against_fp64(L, name, C, M):
    """p2w_bn_chain_bwd through the ABI on the GPU forward's own out, mean and invstd: dz, dres, dgamma, dbeta and ddw_w within their caps
    (bn_chain_ref's docstring) of the float64 reference on the same fp32 tensors; ddw_b exactly 0; dz exactly 0 in the gamma = 0 column;
    every row written and nothing behind them.  A second call, and one with dense rows, give the same bits."""
    c = R.case(name, C, M)
    fwd = _forward_once(L, name, C, M)
    has_res = c["res"] is not None
    ref, caps = R.backward_reference(c["g"], c["z"], c["stages"], fwd["out"] if has_res else None, fwd["mean"], fwd["invstd"])
    got = _backward(L, c, _pitch(C), fwd)
    keys = ["dz", "dgamma", "dbeta", "ddw_w"] + (["dres"] if has_res else [])
    ratios = {k: R.ratio(got[k], ref[k], caps[k]) for k in keys}
    print(f"BNCHAIN_RATIO backward {name} C={C} M={M} " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0
    assert bool((got["ddw_b"] == 0).all()) and (has_res or got["dres"] is None)
    assert bool((got["dz"][:, R.GAMMA_ZERO] == 0).all()) and float(got["dz"].abs().max()) > 0 and float(got["dgamma"].abs().max()) > 0
    for s, st in enumerate(c["stages"]):
        if st["a"] is None:
            assert bool((got["ddw_w"][s] == 0).all())
        elif M > 2:
            assert float(got["ddw_w"][s].abs().max()) > 0
    for other in (_backward(L, c, _pitch(C), fwd), _backward(L, c, C, fwd)):
        for k in got:
            assert (got[k] is None and other[k] is None) or torch.equal(_bits(got[k]), _bits(other[k])), k


def test_access_widths_give_the_same_bits(L):
    """C = 16 with an odd pitch takes the 4-byte lanes: the same bits as the 16-byte lanes, forward and backward."""
    c = R.case("three_res", 16)
    fwd = _forward_once(L, "three_res", 16, R.M_ROWS)
    odd = _forward(L, c, 19)
    for k in fwd:
        assert torch.equal(_bits(fwd[k]), _bits(odd[k])), k
    a, b = _backward(L, c, _pitch(16), fwd), _backward(L, c, 19, fwd)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


# ------------------------------------------------------------------------------------------------ ABI guards
def test_abi_guards_return_their_codes_and_launch_nothing(L):
    """M = 1, L = 0, L = 4, pitches below C, a depthwise weight without its bias, a negative eps and a momentum above 1 (-1), NULL
    pointers (-2), a workspace off 16 bytes (-3) and one that is too small (-4): checked before anything is launched, so the
    NaN-filled outputs stay NaN and the running statistics stay put.  Then the good calls write them."""
    BnStage, ptr, stream = _abi()
    M, C, nL = 14, 8, 2
    z, g, res = (torch.randn(M, C + 4, device="cuda") for _ in range(3))
    vec = {k: torch.rand(C, device="cuda") + 0.5 for k in ("a", "b", "g0", "b0", "g1", "b1")}
    rm, rv = torch.zeros(2, C, device="cuda"), torch.ones(2, C, device="cuda")
    out, dz, dres = (torch.full((M, C + 4), NAN, device="cuda") for _ in range(3))
    mean, invstd, dgamma, dbeta, ddw_w, ddw_b = (torch.full((nL * C,), NAN, device="cuda") for _ in range(6))

    def stages(**kw):
        arr = (BnStage * 3)()
        arr[0] = BnStage(None, None, ptr(vec["g0"]), ptr(vec["b0"]), ptr(rm[0]), ptr(rv[0]), 0.1, 1e-5, 1)
        arr[1] = BnStage(ptr(vec["a"]), ptr(vec["b"]), ptr(vec["g1"]), ptr(vec["b1"]), ptr(rm[1]), ptr(rv[1]), 0.1, 1e-5, 0)
        arr[2] = arr[0]
        for k, v in kw.items():
            setattr(arr[1], k, v)
        return arr

    need = int(L.p2w_bn_chain_ws_size(M, C, nL))
    assert need > 0 and need % 256 == 0
    assert L.p2w_bn_chain_ws_size(1, C, nL) == 0 and L.p2w_bn_chain_ws_size(M, 0, nL) == 0 and L.p2w_bn_chain_ws_size(M, C, 0) == 0
    assert L.p2w_bn_chain_ws_size(M, C, 4) == 0 and L.p2w_bn_chain_ws_size(M, C, 3) >= need
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    s = stream()

    def fwd(z_=ptr(z), ldz=C + 4, res_=ptr(res), ldr=C + 4, st=None, L_=nL, M_=M, C_=C, out_=ptr(out), ldo=C + 4, mean_=ptr(mean),
            invstd_=ptr(invstd), ws_=ptr(ws), wsb=need):
        return L.p2w_bn_chain(z_, ldz, res_, ldr, stages() if st is None else st, L_, M_, C_, out_, ldo, mean_, invstd_, ws_, wsb, s)

    def bwd(g_=ptr(g), ldg=C + 4, z_=ptr(z), ldz=C + 4, out_=ptr(out), ldo=C + 4, st=None, L_=nL, mean_=ptr(mean), invstd_=ptr(invstd), M_=M, C_=C,
            dz_=ptr(dz), lddz=C + 4, dres_=ptr(dres), lddr=C + 4, dgamma_=ptr(dgamma), dbeta_=ptr(dbeta), ddw_w_=ptr(ddw_w), ddw_b_=ptr(ddw_b),
            ws_=ptr(ws), wsb=need):
        return L.p2w_bn_chain_bwd(g_, ldg, z_, ldz, out_, ldo, stages() if st is None else st, L_, mean_, invstd_, M_, C_, dz_, lddz, dres_, lddr,
                                  dgamma_, dbeta_, ddw_w_, ddw_b_, ws_, wsb, s)

    for name in ("z_", "out_", "mean_", "invstd_", "ws_"):
        assert fwd(**{name: None}) == ENULL, name
    for k in ("gamma", "beta", "running_mean", "running_var"):
        assert fwd(st=stages(**{k: None})) == ENULL, k
    for name in ("g_", "z_", "mean_", "invstd_", "dz_", "dgamma_", "dbeta_", "ddw_w_", "ddw_b_", "ws_"):
        assert bwd(**{name: None}) == ENULL, name
    assert bwd(st=stages(gamma=None)) == ENULL
    assert fwd(ws_=ptr(ws) + 4) == EALIGN and bwd(ws_=ptr(ws) + 8) == EALIGN
    assert fwd(M_=1) == EINVAL and fwd(L_=0) == EINVAL and fwd(L_=4) == EINVAL and fwd(C_=0) == EINVAL
    assert fwd(ldz=C - 1) == EINVAL and fwd(ldo=C - 1) == EINVAL and fwd(ldr=C - 4) == EINVAL
    assert fwd(st=stages(dw_b=None)) == EINVAL and fwd(st=stages(eps=-1.0)) == EINVAL and fwd(st=stages(momentum=1.5)) == EINVAL
    assert bwd(M_=1) == EINVAL and bwd(L_=0) == EINVAL and bwd(L_=4) == EINVAL and bwd(ldg=C - 1) == EINVAL and bwd(ldz=4) == EINVAL
    assert bwd(lddz=C - 1) == EINVAL and bwd(ldo=C - 1) == EINVAL and bwd(lddr=C - 1) == EINVAL and bwd(out_=None) == EINVAL   # dres needs out
    assert fwd(wsb=need - 1) == EWORKSPACE and fwd(wsb=0) == EWORKSPACE and bwd(wsb=need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    for t in (out, dz, dres, mean, invstd, dgamma, dbeta, ddw_w, ddw_b):
        assert bool(torch.isnan(t).all())
    assert bool((rm == 0).all()) and bool((rv == 1).all())
    assert fwd() == 0
    assert bwd() == 0
    assert bwd(out_=None, dres_=None) == 0                   # a chain without a residual
    torch.cuda.synchronize()
    for t in (out[:, :C], dz[:, :C], dres[:, :C], mean, invstd, dgamma, dbeta, ddw_w, ddw_b):
        assert bool(torch.isfinite(t).all())
    assert bool(torch.isnan(out[:, C:]).all()) and bool(torch.isnan(dz[:, C:]).all()) and bool((out[:, :C] >= 0).all())
    assert bool((rm != 0).any()) and bool((rv != 1).any()) and bool((ddw_b == 0).all()) and bool((ddw_w[:C] == 0).all())


# ------------------------------------------------------------------------------------------------ the operator
def _modules(c, dtype=torch.float32, **bn_kw):
    """The case's stages as (BatchNorm1d, relu, depthwise Conv1d or None) on the GPU, in training mode."""
    C, out = c["z"].shape[1], []
    for st in c["stages"]:
        bn = torch.nn.BatchNorm1d(C, eps=R.BN_EPS, momentum=R.MOMENTUM, **bn_kw).to(dtype)
        with torch.no_grad():
            if bn.affine:
                bn.weight.copy_(st["gamma"]), bn.bias.copy_(st["beta"])
            if bn.track_running_stats:
                bn.running_mean.copy_(st["running_mean"]), bn.running_var.copy_(st["running_var"])
        dw = None
        if st["a"] is not None:
            dw = torch.nn.Conv1d(C, C, 1, groups=C).to(dtype)
            with torch.no_grad():
                dw.weight.copy_(st["a"].view(C, 1, 1)), dw.bias.copy_(st["b"])
        out.append((bn.cuda().train(), st["relu"], None if dw is None else dw.cuda()))
    return out


def _plain(z, mods, res=None):
    """The literal composition with the modules' own tensors under ordinary autograd."""
    x = z
    for bn, relu, dw in mods:
        if dw is not None:
            x = x * dw.weight.reshape(-1) + dw.bias
        x = bn(x)
        if relu:
            x = torch.relu(x)
    return x if res is None else torch.relu(x + res)


def _route(fn, mods, c):
    z = c["z"].cuda().requires_grad_()
    res = None if c["res"] is None else c["res"].cuda().requires_grad_()
    out = fn(z, mods, res)
    (out * c["g"].cuda()).sum().backward()
    r = dict(out=out.detach(), dz=z.grad, tracked=[int(bn.num_batches_tracked) for bn, _, _ in mods])
    if res is not None:
        r["dres"] = res.grad
    for s, (bn, _, dw) in enumerate(mods):
        r.update({f"dgamma{s}": bn.weight.grad, f"dbeta{s}": bn.bias.grad, f"running_mean{s}": bn.running_mean, f"running_var{s}": bn.running_var})
        if dw is not None:
            r.update({f"ddw_w{s}": dw.weight.grad.reshape(-1), f"ddw_b{s}": dw.bias.grad})
    return {k: v.cpu() if torch.is_tensor(v) else v for k, v in r.items()}


@pytest.mark.parametrize("name", ["expand", "middle", "tail", "project", "three_res"])
def test_operator_against_the_plain_route(H, name):
    """ops.bn_chain against the plain composition on the GPU with cloned modules and ordinary autograd, both against bn_chain_ref's
    float64 chain: the output, every gradient and the running statistics as relative L2; the fused route may not be worse than 8 x
    the plain route's own error (the bar of test_gpu_bn_max).  Where the plain route's error is 0 the fused route is held to the
    derived caps instead (their norm over the reference's; the caps are taken on the float64 statistics rounded to fp32).  The
    depthwise bias has the exact gradient 0, which the fused route returns; num_batches_tracked moves by one per stage."""
    C = 16
    c = R.case(name, C)
    mods = _modules(c)
    fused = _route(lambda z, m, r: H.bn_chain(z, [(bn, relu, dw) if dw is not None else (bn, relu) for bn, relu, dw in m], r), copy.deepcopy(mods), c)
    plain = _route(_plain, copy.deepcopy(mods), c)
    ref = R.chain64(c["z"], c["stages"], c["res"], c["g"])
    mean32, invstd32 = torch.stack(ref["mean"]).float(), torch.stack(ref["invstd"]).float()
    _, fcap = R.forward_reference(c["z"], c["stages"], c["res"], mean32, invstd32)
    _, bcap = R.backward_reference(c["g"], c["z"], c["stages"], None if c["res"] is None else ref["out"].float(), mean32, invstd32)
    want, cap = dict(out=ref["out"], dz=ref["dz"]), dict(out=fcap["out"], dz=bcap["dz"])
    if c["res"] is not None:
        want["dres"], cap["dres"] = ref["dres"], bcap["dres"]
    for s, st in enumerate(c["stages"]):
        for k in ("dgamma", "dbeta", "running_mean", "running_var"):
            want[f"{k}{s}"], cap[f"{k}{s}"] = ref[k][s], (bcap if k[0] == "d" else fcap)[k][s]
        if st["a"] is not None:
            want[f"ddw_w{s}"], cap[f"ddw_w{s}"] = ref["ddw_w"][s], bcap["ddw_w"][s]
            assert bool((fused[f"ddw_b{s}"] == 0).all())
    for k in want:
        ef, ep = _rel_l2(fused[k], want[k]), _rel_l2(plain[k], want[k])
        print(f"BNCHAIN_OP {name} {k}: fused {ef:.3e} plain {ep:.3e}")
        if ep > 0:
            assert ef <= 8 * ep, (k, ef, ep)
        else:
            assert ef <= float(cap[k].norm() / want[k].double().norm()), (k, ef)
    assert fused["tracked"] == plain["tracked"] == [1] * len(mods)
    assert fused["out"].dtype == torch.float32 and fused["out"].shape == c["z"].shape


def test_operator_modes_and_errors(H):
    """no_grad: the same output bits, no graph, the running statistics and num_batches_tracked move as with gradients tracked.
    autocast(float16): fp32 output, gradients in their inputs' dtypes.  Eval mode: the composition on the running statistics bit for
    bit, which stay put.  affine=False, track_running_stats=False, momentum=None and a depthwise convolution without a bias raise
    NotImplementedError, fewer than two rows PyTorch's ValueError, mixed modes and four stages a RuntimeError."""
    c = R.case("three_res", 16)
    z, res = c["z"].cuda(), c["res"].cuda()
    a, b = _modules(c), _modules(c)
    tracked = H.bn_chain(z.clone().requires_grad_(), a, res)
    assert tracked.grad_fn is not None
    with torch.no_grad():
        plain = H.bn_chain(z.clone().requires_grad_(), b, res)
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(_bits(plain), _bits(tracked.detach()))
    for (x, _, _), (y, _, _), st in zip(a, b, c["stages"]):
        assert torch.equal(x.running_mean, y.running_mean) and torch.equal(x.running_var, y.running_var)
        assert int(x.num_batches_tracked) == int(y.num_batches_tracked) == 1
        assert not torch.equal(x.running_mean.cpu(), st["running_mean"])
    h = _modules(c)
    zh = z.half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = H.bn_chain(zh, h, res)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert zh.grad.dtype == torch.float16 and h[0][0].weight.grad.dtype == torch.float32 and h[0][2].weight.grad.dtype == torch.float32
    assert h[0][2].weight.grad.shape == h[0][2].weight.shape and bool((h[0][2].bias.grad == 0).all())
    e = [(bn.eval(), relu, dw) for bn, relu, dw in _modules(c)]
    before = [(bn.running_mean.clone(), bn.running_var.clone()) for bn, _, _ in e]
    got, want = H.bn_chain(z, e, res), _plain(z, e, res)
    assert torch.equal(_bits(got.detach()), _bits(want.detach()))
    for (bn, _, _), (m0, v0) in zip(e, before):
        assert torch.equal(bn.running_mean, m0) and torch.equal(bn.running_var, v0) and int(bn.num_batches_tracked) == 0
    one = R.case("one", 16)
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        with pytest.raises(NotImplementedError):
            H.bn_chain(z, _modules(one, **kw))
    none = _modules(one)
    none[0][0].momentum = None
    with pytest.raises(NotImplementedError):
        H.bn_chain(z, none)
    bn = _modules(one)[0][0]
    with pytest.raises(NotImplementedError, match="bias"):
        H.bn_chain(z, [(bn, True, torch.nn.Conv1d(16, 16, 1, groups=16, bias=False).cuda())])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        H.bn_chain(z[:1], _modules(one))
    mixed = _modules(c)
    mixed[1][0].eval()
    with pytest.raises(RuntimeError, match="same mode"):
        H.bn_chain(z, mixed, res)
    with pytest.raises(RuntimeError, match="stages"):
        H.bn_chain(z, _modules(c) + _modules(one))


# ------------------------------------------------------------------------------------------------ the module
M_BLOCK = 600


def _conv(sd, p, x):
    return F.linear(x, sd[p + ".weight"][:, :, 0], sd[p + ".bias"])


def _bn_train(sd, p, x, stats):
    stats[p] = (x.mean(0).detach(), x.var(0, unbiased=True).detach())
    return F.batch_norm(x, None, None, sd[p + ".weight"], sd[p + ".bias"], True, 0.0, 1e-5)


def _train_resblock(sd, x, stats):
    """oracle/net.py's _resblock (the row-major form of model.py:75-85) with training-mode BatchNorm, plus the shortcut branch."""
    def dsc(p, t):
        t = t * sd[p + ".depthwise_conv.weight"][:, 0, 0] + sd[p + ".depthwise_conv.bias"]
        t = F.relu(_bn_train(sd, p + ".depthwise_bn", t, stats))
        return F.relu(_bn_train(sd, p + ".pointwise_bn", _conv(sd, p + ".pointwise_conv", t), stats))
    out = F.relu(_bn_train(sd, "expand.1", _conv(sd, "expand.0", x), stats))
    out = dsc("conv.0", out)
    out = F.relu(_bn_train(sd, "conv.1", out, stats))
    out = dsc("conv.3", out)
    out = _bn_train(sd, "conv.4", out, stats)
    out = _bn_train(sd, "project.1", _conv(sd, "project.0", out), stats)
    res = _bn_train(sd, "shortcut.1", _conv(sd, "shortcut.0", x), stats) if "shortcut.0.weight" in sd else x
    return F.relu(out + res)


def _block_state(cin, cout):
    """A state dict of the block with every parameter and running statistic drawn at random (fp32)."""
    from pointstowood_amd import ops
    g = torch.Generator().manual_seed(17 * cin + cout)
    sd = ops.InvertedResidualBlock(cin, cout).state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("weight") and v.dim() == 1:
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        else:
            v.copy_(torch.randn(v.shape, generator=g) * (0.3 if v.dim() == 3 and v.shape[1] > 1 else 0.5))
    x = torch.randn(M_BLOCK, cin, generator=g)
    return sd, x, torch.randn(M_BLOCK, cout, generator=g)


def _oracle_train(sd, x, g, dtype, lr=None):
    """One training step of the oracle form in `dtype` on the CPU: output, gradients by state-dict name, the batch statistics of every
    BatchNorm; with lr, the parameters after one AdamW step."""
    leaf = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    xx, stats = x.to(dtype).clone().requires_grad_(), {}
    out = _train_resblock(leaf, xx, stats)
    (out * g.to(dtype)).sum().backward()
    r = dict(out=out.detach(), x=xx.grad, **{k: v.grad for k, v in leaf.items()})
    for p, (mu, var) in stats.items():
        r[p + ".running_mean"] = 0.9 * sd[p + ".running_mean"].to(dtype) + 0.1 * mu
        r[p + ".running_var"] = 0.9 * sd[p + ".running_var"].to(dtype) + 0.1 * var
    if lr is not None:
        opt = torch.optim.AdamW(list(leaf.values()), lr=lr)
        opt.step()
        r.update({"step." + k: v.detach().clone() for k, v in leaf.items()})
    return r


def _block_train(H, sd, x, g, lr=None):
    cin, cout = x.shape[1], g.shape[1]
    block = H.InvertedResidualBlock(cin, cout)
    block.load_state_dict(sd)
    block = block.cuda().train()
    xx = x.cuda().requires_grad_()
    out = block(xx)
    (out * g.cuda()).sum().backward()
    r = dict(out=out.detach(), x=xx.grad, **{k: p.grad for k, p in block.named_parameters()})
    r.update({k: v.clone() for k, v in block.state_dict().items() if "running" in k})
    tracked = {k: int(v) for k, v in block.state_dict().items() if k.endswith("num_batches_tracked")}
    if lr is not None:
        torch.optim.AdamW(block.parameters(), lr=lr).step()
        r.update({"step." + k: p.detach().clone() for k, p in block.named_parameters()})
    return {k: v.cpu() for k, v in r.items()}, tracked


def test_block_has_the_reference_state_dict():
    """ops.InvertedResidualBlock(128, 128): the keys, their order and the shapes of sa1_module.residual_block.* in the recorded
    state dict of the reference's Net (tests/golden/host/load_model.json); with other widths in and out, the shortcut's keys follow."""
    from pointstowood_amd import ops
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host", "load_model.json")))["loaded"]
    prefix = "sa1_module.residual_block."
    want = [(k[len(prefix):], list(v[2])) for k, v in golden.items() if k.startswith(prefix)]
    assert len(want) == 52
    sd = ops.InvertedResidualBlock(128, 128).state_dict()
    assert [(k, list(v.shape)) for k, v in sd.items()] == want
    extra = [k for k in ops.InvertedResidualBlock(8, 12).state_dict() if k not in ops.InvertedResidualBlock(8, 8).state_dict()]
    assert extra == [f"shortcut.{k}" for k in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var", "1.num_batches_tracked")]


@pytest.mark.parametrize("cin,cout", [(8, 8), (8, 12)])
def test_block_trains_like_the_oracle_form(H, cin, cout):
    """Training-mode ops.InvertedResidualBlock at M = 600 against the float64 composition over oracle/net.py's row-major form with
    training-mode BatchNorm: the output, the gradient to x, every parameter gradient and every running statistic, relative L2 <= 8 x
    the oracle form's own fp32-against-fp64 noise per tensor (the bar of tests/test_gpu_conv_train.py, the noise taken here on the CPU).
    The depthwise biases' gradients are exactly 0 (the float64 form's are its summation noise).  Then one AdamW step: every parameter
    lands within the same bar of the float64 form's.  num_batches_tracked is 1 everywhere.  A second run from the same state gives
    the same bits in the output and in every gradient."""
    sd, x, g = _block_state(cin, cout)
    ref, noise = _oracle_train(sd, x, g, torch.float64, lr=1e-3), _oracle_train(sd, x, g, torch.float32, lr=1e-3)
    got, tracked = _block_train(H, sd, x, g, lr=1e-3)
    assert set(got) == set(ref) and set(tracked.values()) == {1} and len(tracked) == (9 if cin != cout else 8)
    for k in ref:
        if k.endswith("depthwise_conv.bias") and not k.startswith("step."):
            assert bool((got[k] == 0).all()), k
            continue
        e, n = _rel_l2(got[k], ref[k]), _rel_l2(noise[k], ref[k])
        print(f"block {cin}->{cout} {k}: rel L2 {e:.3e}, noise {n:.3e}")
        assert e <= 8 * n, (k, e, n)
    again, _ = _block_train(H, sd, x, g)
    for k in again:
        assert torch.equal(_bits(again[k]), _bits(got[k])), k


def test_block_eval_mode_is_the_oracle_block(H):
    """Eval mode on the GPU against oracle.net._resblock on the same state dict: relative L2 against its float64 run <= 8 x its own
    fp32-against-fp64 noise; the running statistics stay put."""
    from oracle import net as N
    sd, x, _ = _block_state(8, 8)
    block = H.InvertedResidualBlock(8, 8)
    block.load_state_dict(sd)
    block = block.cuda().eval()
    with torch.no_grad():
        got = block(x.cuda()).cpu()
    pre = {"b." + k: v for k, v in sd.items()}
    ref = N._resblock({k: v.double() if v.is_floating_point() else v for k, v in pre.items()}, "b", x.double())
    noise = _rel_l2(N._resblock(pre, "b", x), ref)
    err = _rel_l2(got, ref)
    print(f"block eval: rel L2 {err:.3e}, noise {noise:.3e}")
    assert err <= 8 * noise
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in block.state_dict().items())
