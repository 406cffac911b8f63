"""p2w_relu_bn_max / p2w_relu_bn_max_bwd (csrc/p2w_bnmax.hip) through the C ABI against the float64 references and caps of
tests/bn_max_ref.py, ops.relu_bn_max against scatter_max(bn(relu(z))), and ops.PointNetConv with fused_bn_max against the float64
oracle layer of tests/test_gpu_conv_train.py."""
import copy
import json

import pytest
import torch

from tests import bn_max_ref as R
from tests.test_gpu_conv_train import NOISE_JSON, _layer_case, _layer_results, _oracle_layer, _pitched
from tests.test_gpu_ops_backward import _mlp, _rel_l2

pytestmark = pytest.mark.gpu

EINVAL, ENULL, EALIGN, EWORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def H():
    from pointstowood_amd import ops
    return ops


@pytest.fixture(scope="module")
def L():
    from pointstowood_amd._lib import lib
    return lib()


def _abi():
    from pointstowood_amd._lib import ptr, stream
    return ptr, stream


def _pitch(C2):
    """A row pitch larger than C2 that keeps the access width of C2."""
    return C2 + 8 if C2 % 4 == 0 else C2 + 3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _forward(L, C2, ldz):
    """One call of p2w_relu_bn_max on the case at width C2 with z pitched to ldz (NaN in the padding).  Every output has one row or
    element more than the kernel may write, filled with NaN (-7 for arg); returns them on the CPU with the device inputs."""
    ptr, stream = _abi()
    c, d = R.targets(), R.columns(C2)
    M, E = R.M_DST, c["E"]
    dev = dict(z=_pitched(d["z"], ldz), ptr=c["ptr"].cuda(), gamma=d["gamma"].cuda(), beta=d["beta"].cuda())
    rm, rv = (torch.cat([d[k], torch.full((1,), float("nan"))]).cuda() for k in ("running_mean", "running_var"))
    out, ext = (torch.full((M + 1, C2), float("nan"), device="cuda") for _ in range(2))
    arg = torch.full((M + 1, C2), -7, dtype=torch.int32, device="cuda")
    mean, invstd = (torch.full((C2 + 1,), float("nan"), device="cuda") for _ in range(2))
    need = int(L.p2w_relu_bn_max_ws_bytes(E, M, C2))
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_relu_bn_max(ptr(dev["z"]), ldz, ptr(dev["ptr"]), ptr(dev["gamma"]), ptr(dev["beta"]), ptr(rm), ptr(rv), R.MOMENTUM, R.BN_EPS,
                             E, M, C2, ptr(out), ptr(ext), ptr(arg), ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[M]).all()) and bool(torch.isnan(ext[M]).all()) and bool((arg[M] == -7).all())       # the row after the last
    assert bool(torch.isnan(mean[C2])) and bool(torch.isnan(invstd[C2])) and bool(torch.isnan(rm[C2])) and bool(torch.isnan(rv[C2]))
    assert bool(torch.isnan(dev["z"][:, C2:]).all())
    got = dict(out=out[:M], ext=ext[:M], arg=arg[:M], mean=mean[:C2], invstd=invstd[:C2], running_mean=rm[:C2], running_var=rv[:C2])
    return {k: v.cpu() for k, v in got.items()}, dev


_gpu_fwd = {}


def _forward_once(L, C2):
    if C2 not in _gpu_fwd:
        _gpu_fwd[C2] = _forward(L, C2, _pitch(C2))
    return _gpu_fwd[C2]


_ref_fwd = {}


def _reference(C2):
    if C2 not in _ref_fwd:
        c, d = R.targets(), R.columns(C2)
        _ref_fwd[C2] = R.forward_reference(d["z"], c["index"], R.M_DST, d["gamma"], d["beta"], d["running_mean"], d["running_var"])
    return _ref_fwd[C2]


@pytest.mark.parametrize("C2", R.WIDTHS)
def test_kernel_forward_against_fp64(L, C2):
    """p2w_relu_bn_max through the ABI on bn_max_ref's case (1100 targets in 69 groups, degrees 0 .. 1500, nine trailing empty targets,
    odd E, rows pitched with NaN behind them; an all-negative, a constant, a gamma < 0 and a gamma = 0 column, an all-tie target): ext
    and arg bit for bit, mean, invstd, the running statistics and out within the caps derived in bn_max_ref's docstring; out equals
    beta exactly in the all-negative column; empty targets give 0 and -1; nothing is written behind the last row or element.  A
    second call, and one with dense rows, give the same bits."""
    c, d = R.targets(), R.columns(C2)
    ref, caps = _reference(C2)
    got, _ = _forward_once(L, C2)
    assert torch.equal(got["arg"].long(), ref["arg"])
    assert torch.equal(got["ext"].double(), ref["ext"]) and not bool(torch.signbit(got["ext"]).any())
    ratios = {k: R.ratio(got[k], ref[k], caps[k]) for k in ("mean", "invstd", "running_mean", "running_var")}
    ratios["out"] = R.ratio(got["out"], ref["out"], R.out_cap(ref, caps, d["gamma"], d["beta"]))
    print(f"BNMAX_RATIO forward C2={C2} " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0
    live = c["deg"] > 0
    assert int((~live).sum()) >= R.TRAILING_EMPTY + 1
    assert bool((got["out"][~live] == 0).all()) and bool((got["ext"][~live] == 0).all()) and bool((got["arg"][~live] == -1).all())
    assert bool((got["out"][live][:, R.ALL_NEG] == d["beta"][R.ALL_NEG]).all())
    assert float(got["mean"][R.ALL_NEG]) == 0.0 and float(got["mean"][R.CONST]) == float(d["z"][0, R.CONST])
    first = int(c["ptr"][R.TIE_TARGET])
    assert bool((got["arg"][R.TIE_TARGET, 4:] == first).all()) and int(got["arg"][R.TIE_TARGET, R.ALL_NEG]) == first
    assert float(got["ext"][5, R.GAMMA_NEG]) == 0.0 and float(got["ext"][5, 4]) > 0.0          # 1500 rows: the minimum and the maximum
    for other, _ in (_forward(L, C2, _pitch(C2)), _forward(L, C2, C2)):
        for k in got:
            assert torch.equal(_bits(got[k]), _bits(other[k])), k


def _backward(L, C2, ldz, fwd, dev, g):
    ptr, stream = _abi()
    c = R.targets()
    M, E = R.M_DST, c["E"]
    z = dev["z"] if dev["z"].shape[1] == ldz else _pitched(R.columns(C2)["z"], ldz)
    f = {k: fwd[k].cuda() for k in ("arg", "ext", "mean", "invstd")}
    gd = g.cuda()
    dz = torch.full((E + 1, ldz), float("nan"), device="cuda")
    dgamma, dbeta = (torch.full((C2 + 1,), float("nan"), device="cuda") for _ in range(2))
    need = int(L.p2w_relu_bn_max_ws_bytes(E, M, C2))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_relu_bn_max_bwd(ptr(gd), ptr(z), ldz, ptr(dev["ptr"]), ptr(f["arg"]), ptr(f["ext"]), ptr(f["mean"]), ptr(f["invstd"]),
                                 ptr(dev["gamma"]), E, M, C2, ptr(dz), ldz, ptr(dgamma), ptr(dbeta), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz[E]).all()) and bool(torch.isnan(dz[:, C2:]).all()) and bool(torch.isnan(dgamma[C2])) and bool(torch.isnan(dbeta[C2]))
    return dz[:E, :C2].cpu(), dgamma[:C2].cpu(), dbeta[:C2].cpu()


@pytest.mark.parametrize("C2", R.WIDTHS)
def test_kernel_backward_against_fp64(L, C2):
    """p2w_relu_bn_max_bwd through the ABI on the GPU forward's own arg, ext, mean and invstd: dz, dgamma and dbeta within their caps
    (bn_max_ref's docstring) of the float64 reference on the same fp32 tensors; dz exactly 0 where z <= 0 (the whole all-negative
    column with it) and in the gamma = 0 column, every row written and nothing behind them.  A second call, and one with dense rows,
    give the same bits."""
    c, d = R.targets(), R.columns(C2)
    fwd, dev = _forward_once(L, C2)
    ref, caps = R.backward_reference(d["g"], d["z"], c["index"], fwd["arg"].long(), fwd["ext"], fwd["mean"], fwd["invstd"], d["gamma"])
    got = _backward(L, C2, _pitch(C2), fwd, dev, d["g"])
    ratios = [R.ratio(a, b, cap) for a, b, cap in zip(got, ref, caps)]
    print(f"BNMAX_RATIO backward C2={C2} dz {ratios[0]:.3f} dgamma {ratios[1]:.3f} dbeta {ratios[2]:.3f}")
    assert max(ratios) <= 1.0
    dz = got[0]
    assert bool((dz[d["z"] <= 0] == 0).all()) and bool((dz[:, R.ALL_NEG] == 0).all()) and bool((dz[:, R.GAMMA_ZERO] == 0).all())
    assert float(dz[:, R.GAMMA_NEG].abs().max()) > 0 and float(dz[:, 4].abs().max()) > 0 and float(got[1].abs().max()) > 0
    for other in (_backward(L, C2, _pitch(C2), fwd, dev, d["g"]), _backward(L, C2, C2, fwd, dev, d["g"])):
        for a, b in zip(got, other):
            assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ ABI guards
def test_abi_guards_return_their_codes_and_launch_nothing(L):
    """NULL pointers (-2), a workspace off 16 bytes (-3), E < 2, M < 1, C2 < 1, pitches below C2, a negative eps and a momentum outside
    [0, 1] (-1), a workspace that is too small (-4): checked before anything is launched, so the NaN-filled outputs stay NaN and the
    running statistics stay put.  Then the good calls write them."""
    ptr, stream = _abi()
    E, M, C2 = 14, 5, 8
    csr = torch.tensor([0, 3, 3, 10, 11, 14], dtype=torch.int32, device="cuda")
    z, g = torch.randn(E, C2 + 4, device="cuda"), torch.randn(M, C2, device="cuda")
    gamma, beta = torch.rand(C2, device="cuda") + 0.5, torch.randn(C2, device="cuda")
    rm, rv = torch.zeros(C2, device="cuda"), torch.ones(C2, device="cuda")
    out, ext = (torch.full((M, C2), float("nan"), device="cuda") for _ in range(2))
    arg = torch.full((M, C2), -7, dtype=torch.int32, device="cuda")
    mean, invstd, dgamma, dbeta = (torch.full((C2,), float("nan"), device="cuda") for _ in range(4))
    dz = torch.full((E, C2 + 4), float("nan"), device="cuda")
    need = int(L.p2w_relu_bn_max_ws_bytes(E, M, C2))
    assert need > 0 and need % 256 == 0
    assert L.p2w_relu_bn_max_ws_bytes(1, M, C2) == 0 and L.p2w_relu_bn_max_ws_bytes(E, 0, C2) == 0 and L.p2w_relu_bn_max_ws_bytes(E, M, 0) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    s = stream()

    def fwd(z_=ptr(z), ldz=C2 + 4, csr_=ptr(csr), gamma_=ptr(gamma), beta_=ptr(beta), rm_=ptr(rm), rv_=ptr(rv), mom=0.1, eps=1e-5, E_=E, M_=M,
            C2_=C2, out_=ptr(out), ext_=ptr(ext), arg_=ptr(arg), mean_=ptr(mean), invstd_=ptr(invstd), ws_=ptr(ws), wsb=need):
        return L.p2w_relu_bn_max(z_, ldz, csr_, gamma_, beta_, rm_, rv_, mom, eps, E_, M_, C2_, out_, ext_, arg_, mean_, invstd_, ws_, wsb, s)

    def bwd(g_=ptr(g), z_=ptr(z), ldz=C2 + 4, csr_=ptr(csr), arg_=ptr(arg), ext_=ptr(ext), mean_=ptr(mean), invstd_=ptr(invstd),
            gamma_=ptr(gamma), E_=E, M_=M, C2_=C2, dz_=ptr(dz), lddz=C2 + 4, dgamma_=ptr(dgamma), dbeta_=ptr(dbeta), ws_=ptr(ws), wsb=need):
        return L.p2w_relu_bn_max_bwd(g_, z_, ldz, csr_, arg_, ext_, mean_, invstd_, gamma_, E_, M_, C2_, dz_, lddz, dgamma_, dbeta_, ws_, wsb, s)

    for name in ("z_", "csr_", "gamma_", "beta_", "rm_", "rv_", "out_", "ext_", "arg_", "mean_", "invstd_", "ws_"):
        assert fwd(**{name: None}) == ENULL, name
    for name in ("g_", "z_", "csr_", "arg_", "ext_", "mean_", "invstd_", "gamma_", "dz_", "dgamma_", "dbeta_", "ws_"):
        assert bwd(**{name: None}) == ENULL, name
    assert fwd(ws_=ptr(ws) + 4) == EALIGN and bwd(ws_=ptr(ws) + 8) == EALIGN
    assert fwd(E_=1) == EINVAL and fwd(E_=-1) == EINVAL and fwd(M_=0) == EINVAL and fwd(C2_=0) == EINVAL and fwd(ldz=C2 - 1) == EINVAL
    assert fwd(eps=-1.0) == EINVAL and fwd(mom=1.5) == EINVAL and fwd(mom=-0.1) == EINVAL and fwd(eps=float("nan")) == EINVAL
    assert bwd(E_=1) == EINVAL and bwd(M_=-3) == EINVAL and bwd(C2_=0) == EINVAL and bwd(ldz=C2 - 4) == EINVAL and bwd(lddz=4) == EINVAL
    assert fwd(wsb=need - 1) == EWORKSPACE and fwd(wsb=0) == EWORKSPACE and bwd(wsb=need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    for t in (out, ext, mean, invstd, dgamma, dbeta, dz):
        assert bool(torch.isnan(t).all())
    assert bool((arg == -7).all()) and bool((rm == 0).all()) and bool((rv == 1).all())
    assert fwd() == 0
    assert bwd() == 0
    torch.cuda.synchronize()
    for t in (out, ext, mean, invstd, dgamma, dbeta, dz[:, :C2]):
        assert bool(torch.isfinite(t).all())
    assert bool(torch.isnan(dz[:, C2:]).all()) and bool((arg[1] == -1).all()) and bool((out[1] == 0).all()) and bool((arg[0] >= 0).all())
    assert bool((rm != 0).any()) and bool((rv != 1).any())
    # pointers off 16 bytes and an odd pitch take the 4-byte path: the same bits
    z1 = torch.full((E * (C2 + 5) + 1,), float("nan"), device="cuda")
    zo = z1[1:].view(E, C2 + 5)
    zo[:, :C2] = z[:, :C2]
    out2, ext2 = torch.empty_like(out), torch.empty_like(ext)
    arg2, mean2, invstd2 = torch.empty_like(arg), torch.empty_like(mean), torch.empty_like(invstd)
    rm2, rv2 = torch.zeros(C2, device="cuda"), torch.ones(C2, device="cuda")
    assert zo.data_ptr() % 16 == 4
    assert fwd(z_=ptr(zo), ldz=C2 + 5, rm_=ptr(rm2), rv_=ptr(rv2), out_=ptr(out2), ext_=ptr(ext2), arg_=ptr(arg2), mean_=ptr(mean2),
               invstd_=ptr(invstd2)) == 0
    dz2, dgamma2, dbeta2 = torch.full((E, C2 + 5), float("nan"), device="cuda"), torch.empty_like(dgamma), torch.empty_like(dbeta)
    assert bwd(z_=ptr(zo), ldz=C2 + 5, dz_=ptr(dz2), lddz=C2 + 5, dgamma_=ptr(dgamma2), dbeta_=ptr(dbeta2)) == 0
    torch.cuda.synchronize()
    for a, b in ((out, out2), (ext, ext2), (arg, arg2), (mean, mean2), (invstd, invstd2), (rm, rm2), (rv, rv2), (dz[:, :C2], dz2[:, :C2]),
                 (dgamma, dgamma2), (dbeta, dbeta2)):
        assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the operator
def _bn_for(C2, dtype=torch.float32, **kw):
    d = R.columns(C2)
    bn = torch.nn.BatchNorm1d(C2, eps=R.BN_EPS, momentum=R.MOMENTUM, **kw).to(dtype)
    with torch.no_grad():
        if bn.affine:
            bn.weight.copy_(d["gamma"])
            bn.bias.copy_(d["beta"])
        if bn.track_running_stats:
            bn.running_mean.copy_(d["running_mean"])
            bn.running_var.copy_(d["running_var"])
    return bn.train()


def _route(fn, bn, z, index, g):
    zz = z.detach().clone().requires_grad_()
    out = fn(zz, index, bn)
    (out * g).sum().backward()
    return dict(out=out.detach().cpu(), z=zz.grad.cpu(), gamma=bn.weight.grad.cpu(), beta=bn.bias.grad.cpu(), running_mean=bn.running_mean.cpu(),
                running_var=bn.running_var.cpu(), tracked=int(bn.num_batches_tracked))


@pytest.mark.parametrize("C2", [16, 128])
def test_operator_against_the_plain_route(H, C2):
    """ops.relu_bn_max against ops.scatter_max(bn(relu(z))) on the GPU with cloned BatchNorms, on bn_max_ref's case: the output and
    the three gradients as relative L2 against the float64 reference, for both routes; the fused route may not be worse than 8 x the
    plain route's own error (the project's margin over fp32 noise).  In the gamma = 0 column the plain route's winner is the target's
    first row (every row ties after BatchNorm) and its gradient with respect to gamma follows that row, the fused route's the
    maximum: the float64 reference sides with the fused route there, so gamma's gradient is held to the same bar a second time without
    that column.  num_batches_tracked and the running statistics move the same way."""
    c, d = R.targets(), R.columns(C2)
    M = R.M_DST
    z, index, g = d["z"].cuda(), c["index"].cuda(), d["g"].cuda()
    bn0 = _bn_for(C2)
    fused = _route(lambda zz, i, bn: H.relu_bn_max(zz, i, bn, M), copy.deepcopy(bn0).cuda(), z, index, g)
    plain = _route(lambda zz, i, bn: H.scatter_max(bn(torch.relu(zz)), i, dim=0, dim_size=M)[0], copy.deepcopy(bn0).cuda(), z, index, g)
    fr, _ = _reference(C2)
    (dz, dgamma, dbeta), _ = R.backward_reference(d["g"], d["z"], c["index"], fr["arg"], fr["ext"], fr["mean"], fr["invstd"], d["gamma"])
    keep = torch.arange(C2) != R.GAMMA_ZERO
    ref = dict(out=fr["out"], z=dz, gamma=dgamma, beta=dbeta, gamma_nonzero=dgamma[keep], running_mean=fr["running_mean"],
               running_var=fr["running_var"])
    for r in (fused, plain):
        r["gamma_nonzero"] = r["gamma"][keep]
    for k in ("out", "z", "gamma", "beta", "gamma_nonzero", "running_mean", "running_var"):
        ef, ep = _rel_l2(fused[k], ref[k]), _rel_l2(plain[k], ref[k])
        print(f"BNMAX_OP C2={C2} {k}: fused {ef:.3e} plain {ep:.3e}")
        assert ef <= 8 * ep, (k, ef, ep)
    assert fused["tracked"] == plain["tracked"] == 1
    assert fused["out"].dtype == torch.float32 and fused["out"].shape == (M, C2)


def test_operator_modes_and_errors(H):
    """no_grad: the same output bits, no graph, the running statistics and num_batches_tracked move as with gradients tracked.
    autocast(float16): fp32 output, gradients in their inputs' dtypes.  Eval mode: the composition on the running statistics, which
    stay put.  dim_size defaults to index.max() + 1.  affine=False, track_running_stats=False and momentum=None raise
    NotImplementedError, fewer than two rows PyTorch's ValueError, an index that descends a RuntimeError."""
    C2 = 16
    c, d = R.targets(), R.columns(C2)
    M = R.M_DST
    z, index = d["z"].cuda(), c["index"].cuda()
    a, b = _bn_for(C2).cuda(), _bn_for(C2).cuda()
    tracked = H.relu_bn_max(z.clone().requires_grad_(), index, a, M)
    assert tracked.grad_fn is not None
    with torch.no_grad():
        plain = H.relu_bn_max(z.clone().requires_grad_(), index, b, M)
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(_bits(plain), _bits(tracked.detach()))
    assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
    assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 1
    assert not torch.equal(a.running_mean.cpu(), d["running_mean"])
    short = H.relu_bn_max(z, index, _bn_for(C2).cuda())
    assert short.shape[0] == M - R.TRAILING_EMPTY and torch.equal(_bits(short), _bits(plain[:M - R.TRAILING_EMPTY]))
    zh, bh = z.half().requires_grad_(), _bn_for(C2).cuda()
    with torch.autocast("cuda", dtype=torch.float16):
        out = H.relu_bn_max(zh, index, bh, M)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert zh.grad.dtype == torch.float16 and bh.weight.grad.dtype == torch.float32 and bh.bias.grad.dtype == torch.float32
    e = _bn_for(C2).cuda().eval()
    before = (e.running_mean.clone(), e.running_var.clone())
    got = H.relu_bn_max(z, index, e, M)
    want = H.scatter_max(e(torch.relu(z)), index, dim=0, dim_size=M)[0]
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(e.running_mean, before[0]) and torch.equal(e.running_var, before[1])
    assert int(e.num_batches_tracked) == 0
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        with pytest.raises(NotImplementedError):
            H.relu_bn_max(z, index, _bn_for(C2, **kw).cuda(), M)
    none = _bn_for(C2).cuda()
    none.momentum = None
    with pytest.raises(NotImplementedError):
        H.relu_bn_max(z, index, none, M)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        H.relu_bn_max(z[:1], index[:1], _bn_for(C2).cuda(), M)
    with pytest.raises(RuntimeError, match="ascending"):
        H.relu_bn_max(z, index.flip(0), _bn_for(C2).cuda(), M)


# ------------------------------------------------------------------------------------------------ the layer
def test_layer_with_fused_bn_max_trains_like_the_oracle_layer(H):
    """ops.PointNetConv with fused_bn_max = True on the shape case of test_layer_trains_like_the_oracle_layer, held to that test's
    bar: output, gradients to x, pos_src[:, 3] and every parameter and BatchNorm's running statistics, relative L2 <= 8 x the oracle
    layer's fp32-against-fp64 noise (tests/golden/conv_train/noise.json, read only) against the float64 oracle layer.  With the flag
    False the layer gives the bits of an instance that never had the attribute set."""
    noise = json.load(open(NOISE_JSON))["rel_l2"]
    c = _layer_case(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    ref = _oracle_layer(c, torch.float64)
    conv = H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), global_nn=None, add_self_loops=False).cuda()
    assert conv.fused_bn_max is False and H.PointNetConv.fused_bn_max is False
    conv.fused_bn_max = True
    got = _layer_results(conv, c, "cuda")
    assert int(conv.local_nn[1][2].num_batches_tracked) == 1
    assert set(got) == set(ref) == set(noise)
    errs = {k: _rel_l2(got[k], ref[k]) for k in ref}
    for k in ref:
        print(f"fused layer {k}: rel L2 {errs[k]:.3e}, noise {noise[k]:.3e}, ratio {errs[k] / noise[k]:.2f}")
    for k in ref:
        assert errs[k] <= 8 * noise[k], (k, errs[k], noise[k])
    again = _layer_results(H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), global_nn=None, add_self_loops=False).cuda(), c, "cuda")
    off = H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), global_nn=None, add_self_loops=False).cuda()
    off.fused_bn_max = False
    same = _layer_results(off, c, "cuda")
    for k in again:
        assert torch.equal(_bits(again[k]), _bits(same[k])), k
