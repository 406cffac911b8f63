"""relu_bn_max on float16 and bfloat16 tensors: p2w_relu_bn_max_io / p2w_relu_bn_max_bwd_io (csrc/p2w_bnmax.hip) through the C ABI,
ops.relu_bn_max and ops.PointNetConv(fused_bn_max) under autocast with ops.half_io on against off, one whole step of train.Net and
trainer.SemanticTraining with fused_bn_max set.

Only the element type at the loads of z and at the store of dz differs from the fp32 entry points, so nothing here has a tolerance.
The expected values are always the fp32 entry points p2w_relu_bn_max / p2w_relu_bn_max_bwd fed z16.float() on bn_max_ref's case:
every fp32 / int32 result is compared bit for bit, and the 16-bit dz is that fp32 dz rounded ON THE CPU (torch.Tensor.half() /
.bfloat16(), which tests/test_bn_max_io_cpu.py pins to tests/half_io_ref.py / tests/bf16_io_ref.py).  A NaN is compared as a NaN.
Rows are pitched with NaN behind them and one NaN guard row behind the last."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch

from tests import bn_max_ref as R

pytestmark = pytest.mark.gpu

EINVAL, ENULL, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
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
    from pointstowood_amd._lib import ptr, stream
    return ptr, stream


def _ibits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _same(a, b):
    """Equal dtype, shape and bit patterns; NaNs at the same places, whatever their payload."""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_ibits(a)[~na], _ibits(b)[~nb])


def _buf(rows, ld, dtype, off=0):
    """[rows, ld] of NaN in `dtype` that starts `off` elements into its allocation."""
    flat = torch.full((rows * ld + off,), NAN, dtype=dtype, device="cuda")
    return flat[off:].view(rows, ld)


def _pitched(t, ld, dtype, off=0):
    buf = _buf(t.shape[0], ld, dtype, off)
    buf[:, :t.shape[1]] = t.to(dtype).cuda()
    return buf


def _pitch(C2):
    """A row pitch larger than C2 that keeps the access width of C2."""
    return C2 + 8 if C2 % 4 == 0 else C2 + 3


def _widths(C2):
    """(pitch, offset in elements) of z and dz.  Where C2 allows 4 columns per lane: the 8-byte accesses on a 16-byte aligned base and
    on one that is 8-byte aligned only (4 elements in), then the ways to one column per lane - an odd pitch, and a base one element
    (2 bytes) off.  Otherwise one column per lane on an aligned and on an offset base."""
    if C2 % 4 == 0:
        return [(_pitch(C2), 0), (_pitch(C2), 4), (C2 + 3, 0), (_pitch(C2), 1)]
    return [(_pitch(C2), 0), (_pitch(C2), 1)]


def _run(L, C2, tz, ld, off, z, g, io=True):
    """Forward and backward on bn_max_ref's case at width C2: z (fp32 values, stored in DT[tz]) and dz pitched to ld and shifted by off
    elements, through the _io entry points (io False: through p2w_relu_bn_max / _bwd, tz = F32).  Every output has a guard row or
    element of NaN (-7 for arg) behind it.  -> the results on the CPU."""
    ptr, stream = _abi()
    c, d = R.targets(), R.columns(C2)
    M, E = R.M_DST, c["E"]
    zd, csr, gamma, beta, gd = _pitched(z, ld, DT[tz], off), c["ptr"].cuda(), d["gamma"].cuda(), d["beta"].cuda(), g.cuda()
    rm, rv = (torch.cat([d[k], torch.full((1,), NAN)]).cuda() for k in ("running_mean", "running_var"))
    out, ext = (torch.full((M + 1, C2), NAN, device="cuda") for _ in range(2))
    arg = torch.full((M + 1, C2), -7, dtype=torch.int32, device="cuda")
    mean, invstd, dgamma, dbeta = (torch.full((C2 + 1,), NAN, device="cuda") for _ in range(4))
    dz = _buf(E + 1, ld, DT[tz], off)
    need = int(L.p2w_relu_bn_max_ws_bytes(E, M, C2))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = stream()
    if io:
        assert L.p2w_relu_bn_max_io(ptr(zd), tz, ld, ptr(csr), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), R.MOMENTUM, R.BN_EPS, E, M, C2, ptr(out),
                                    ptr(ext), ptr(arg), ptr(mean), ptr(invstd), ptr(ws), need, s) == 0
        assert L.p2w_relu_bn_max_bwd_io(ptr(gd), ptr(zd), tz, ld, ptr(csr), ptr(arg), ptr(ext), ptr(mean), ptr(invstd), ptr(gamma), E, M, C2,
                                        ptr(dz), ld, ptr(dgamma), ptr(dbeta), ptr(ws), need, s) == 0
    else:
        assert tz == F32
        assert L.p2w_relu_bn_max(ptr(zd), ld, ptr(csr), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), R.MOMENTUM, R.BN_EPS, E, M, C2, ptr(out), ptr(ext),
                                 ptr(arg), ptr(mean), ptr(invstd), ptr(ws), need, s) == 0
        assert L.p2w_relu_bn_max_bwd(ptr(gd), ptr(zd), ld, ptr(csr), ptr(arg), ptr(ext), ptr(mean), ptr(invstd), ptr(gamma), E, M, C2, ptr(dz), ld,
                                     ptr(dgamma), ptr(dbeta), ptr(ws), need, s) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[M]).all()) and bool(torch.isnan(ext[M]).all()) and bool((arg[M] == -7).all())
    for t in (mean, invstd, dgamma, dbeta, rm, rv):
        assert bool(torch.isnan(t[C2]))
    assert bool(torch.isnan(zd[:, C2:]).all())
    assert dz.dtype == DT[tz] and bool(torch.isnan(dz[E]).all()) and bool(torch.isnan(dz[:, C2:]).all())      # the padding is untouched
    got = dict(out=out[:M], ext=ext[:M], arg=arg[:M], mean=mean[:C2], invstd=invstd[:C2], running_mean=rm[:C2], running_var=rv[:C2],
               dz=dz[:E, :C2], dgamma=dgamma[:C2], dbeta=dbeta[:C2])
    return {k: v.contiguous().cpu() for k, v in got.items()}


_refs = {}


def _reference(L, C2, tz):
    """(z16 as fp32 values, the fp32 entry points' results on it), once per width and element type, left unchanged."""
    if (C2, tz) not in _refs:
        z = R.columns(C2)["z"].to(DT[tz]).float()
        _refs[C2, tz] = (z, _run(L, C2, F32, _pitch(C2), 0, z, R.columns(C2)["g"], io=False))
    return _refs[C2, tz]


def _check(got, ref, tz):
    for k in ref:
        if k != "dz":
            assert _same(got[k], ref[k]), k
    assert got["dz"].dtype == DT[tz] and _same(got["dz"], ref["dz"].to(DT[tz])), "dz"


# ------------------------------------------------------------------------------------------------ the kernels through the ABI
@pytest.mark.parametrize("C2", R.WIDTHS)
@pytest.mark.parametrize("tz", [F16, BF16])
def test_kernels_equal_the_fp32_entry_points(L, tz, C2):
    """p2w_relu_bn_max_io / _bwd_io on a 16-bit z on bn_max_ref's case (1100 targets, degrees 0 .. 1500, empty and all-tie targets, odd
    E, the planted columns): out, ext, arg, mean, invstd, the running statistics, dgamma and dbeta are p2w_relu_bn_max / _bwd's bits on
    z16.float(); dz, in z's type, is their dz rounded once on the CPU, exactly 0 where z <= 0.  Both access widths (8-byte accesses
    on a 16- and on an 8-byte aligned base; one column per lane forced by an odd pitch and by a base 2 bytes off) give those bits; the
    NaN padding of the pitched dz and the guard rows stay untouched."""
    z, ref = _reference(L, C2, tz)
    g = R.columns(C2)["g"]
    assert float(ref["dz"].abs().max()) > 0 and bool((ref["dz"][z <= 0] == 0).all())
    for ld, off in _widths(C2):
        got = _run(L, C2, tz, ld, off, z, g)
        _check(got, ref, tz)
        assert bool((_ibits(got["dz"])[z <= 0] == 0).all()), (ld, off)                     # +0: not -0, not a rounding's leftover
        assert bool((got["dz"][:, R.ALL_NEG] == 0).all()) and bool((got["dz"][:, R.GAMMA_ZERO] == 0).all())


@pytest.mark.parametrize("C2", [6, 16])
def test_fp32_code_through_the_io_entry_points(L, C2):
    """tz = P2W_F32 through p2w_relu_bn_max_io / _bwd_io is p2w_relu_bn_max / _bwd bit for bit, at both widths."""
    z, g = R.columns(C2)["z"], R.columns(C2)["g"]
    ref = _run(L, C2, F32, _pitch(C2), 0, z, g, io=False)
    for ld, off in ((_pitch(C2), 0), (C2 + 3, 0), (_pitch(C2), 1)):
        _check(_run(L, C2, F32, ld, off, z, g), ref, F32)


@pytest.mark.parametrize("tz,up,down", [(F16, 20, -20), (BF16, 0, -128)])
def test_dz_store_reaches_overflow_and_subnormals(L, tz, up, down):
    """g scaled by 2^up in a third of the columns and by 2^down in another third (finite in fp32 everywhere).  float16: a winner's
    |dz| of the order 2^20 overflows to +-inf (from 65520 on: the fp32 dz there is finite) and one of the order 2^-20 lands among the
    subnormals (below 2^-14) - at least 100 elements of each kind.  bfloat16 has fp32's exponent, so only the lower end exists: 2^-128
    puts dz among the subnormals the two formats share (below 2^-126; nothing may be flushed on the way), at least 100 of them.  dz
    still equals the fp32 route's dz rounded on the CPU, at both access widths."""
    C2 = 16
    z, _ = _reference(L, C2, tz)
    scale = torch.ones(C2)
    scale[torch.arange(C2) % 3 == 1], scale[torch.arange(C2) % 3 == 2] = 2.0 ** up, 2.0 ** down
    g = R.columns(C2)["g"] * scale
    assert bool(torch.isfinite(g).all())
    ref = _run(L, C2, F32, _pitch(C2), 0, z, g, io=False)
    assert bool(torch.isfinite(ref["dz"]).all())
    for ld, off in _widths(C2):
        got = _run(L, C2, tz, ld, off, z, g)
        _check(got, ref, tz)
    dz = got["dz"].float()
    tiny = 2.0 ** -14 if tz == F16 else 2.0 ** -126
    sub, inf = int(((dz != 0) & (dz.abs() < tiny)).sum()), int(torch.isinf(dz).sum())
    print(f"BNMAXIO dz tz={tz}: {sub} subnormal, {inf} infinite of {dz.numel()}")
    assert sub >= 100 and (inf >= 100 if tz == F16 else inf == 0)


def test_refusals_launch_nothing(L):
    """The unknown codes 3 and -1: P2W_EUNSUPPORTED from both entry points ahead of every other check.  On float16 and bfloat16
    tensors the namesake's refusals come back unchanged - null pointers (-2), a workspace off 16 bytes (-3), bad sizes, pitches, eps
    and momentum (-1), a workspace that is too small (-4).  Nothing is launched: the NaN-filled outputs stay NaN and the running
    statistics stay put.  Then the good calls write them."""
    ptr, stream = _abi()
    E, M, C2, ld = 14, 5, 8, 12
    csr = torch.tensor([0, 3, 3, 10, 11, 14], dtype=torch.int32, device="cuda")
    g = torch.randn(M, C2, device="cuda")
    gamma, beta = torch.rand(C2, device="cuda") + 0.5, torch.randn(C2, device="cuda")
    need = int(L.p2w_relu_bn_max_ws_bytes(E, M, C2))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    s = stream()
    for tz in (F16, BF16):
        z = _pitched(torch.randn(E, C2), ld, DT[tz])
        rm, rv = torch.zeros(C2, device="cuda"), torch.ones(C2, device="cuda")
        out, ext = (torch.full((M, C2), NAN, device="cuda") for _ in range(2))
        arg = torch.full((M, C2), -7, dtype=torch.int32, device="cuda")
        mean, invstd, dgamma, dbeta = (torch.full((C2,), NAN, device="cuda") for _ in range(4))
        dz = _buf(E, ld, DT[tz])

        def fwd(tz_=tz, z_=ptr(z), ldz=ld, csr_=ptr(csr), gamma_=ptr(gamma), beta_=ptr(beta), rm_=ptr(rm), rv_=ptr(rv), mom=0.1, eps=1e-5, E_=E,
                M_=M, C2_=C2, out_=ptr(out), ext_=ptr(ext), arg_=ptr(arg), mean_=ptr(mean), invstd_=ptr(invstd), ws_=ptr(ws), wsb=need):
            return L.p2w_relu_bn_max_io(z_, tz_, ldz, csr_, gamma_, beta_, rm_, rv_, mom, eps, E_, M_, C2_, out_, ext_, arg_, mean_, invstd_, ws_,
                                        wsb, s)

        def bwd(tz_=tz, g_=ptr(g), z_=ptr(z), ldz=ld, csr_=ptr(csr), arg_=ptr(arg), ext_=ptr(ext), mean_=ptr(mean), invstd_=ptr(invstd),
                gamma_=ptr(gamma), E_=E, M_=M, C2_=C2, dz_=ptr(dz), lddz=ld, dgamma_=ptr(dgamma), dbeta_=ptr(dbeta), ws_=ptr(ws), wsb=need):
            return L.p2w_relu_bn_max_bwd_io(g_, z_, tz_, ldz, csr_, arg_, ext_, mean_, invstd_, gamma_, E_, M_, C2_, dz_, lddz, dgamma_, dbeta_,
                                            ws_, wsb, s)

        for code in (3, -1):
            assert fwd(tz_=code) == EUNSUPPORTED and bwd(tz_=code) == EUNSUPPORTED
            assert fwd(tz_=code, z_=None) == EUNSUPPORTED and fwd(tz_=code, E_=1) == EUNSUPPORTED and fwd(tz_=code, wsb=0) == EUNSUPPORTED
            assert fwd(tz_=code, ws_=ptr(ws) + 4) == EUNSUPPORTED                          # ... ahead of every other check
            assert bwd(tz_=code, dz_=None) == EUNSUPPORTED and bwd(tz_=code, lddz=1) == EUNSUPPORTED and bwd(tz_=code, wsb=0) == EUNSUPPORTED
        for name in ("z_", "csr_", "gamma_", "beta_", "rm_", "rv_", "out_", "ext_", "arg_", "mean_", "invstd_", "ws_"):
            assert fwd(**{name: None}) == ENULL, name
        for name in ("g_", "z_", "csr_", "arg_", "ext_", "mean_", "invstd_", "gamma_", "dz_", "dgamma_", "dbeta_", "ws_"):
            assert bwd(**{name: None}) == ENULL, name
        assert fwd(ws_=ptr(ws) + 4) == EALIGN and bwd(ws_=ptr(ws) + 8) == EALIGN
        assert fwd(E_=1) == EINVAL and fwd(E_=-1) == EINVAL and fwd(M_=0) == EINVAL and fwd(C2_=0) == EINVAL and fwd(ldz=C2 - 1) == EINVAL
        assert fwd(eps=-1.0) == EINVAL and fwd(mom=1.5) == EINVAL and fwd(mom=-0.1) == EINVAL and fwd(eps=NAN) == EINVAL
        assert bwd(E_=1) == EINVAL and bwd(M_=-3) == EINVAL and bwd(C2_=0) == EINVAL and bwd(ldz=C2 - 4) == EINVAL and bwd(lddz=4) == EINVAL
        assert fwd(wsb=need - 1) == EWORKSPACE and fwd(wsb=0) == EWORKSPACE and bwd(wsb=need - 1) == EWORKSPACE
        torch.cuda.synchronize()
        for t in (out, ext, mean, invstd, dgamma, dbeta, dz):
            assert bool(torch.isnan(t).all())
        assert bool((arg == -7).all()) and bool((rm == 0).all()) and bool((rv == 1).all())
        assert fwd() == 0 and bwd() == 0
        torch.cuda.synchronize()
        for t in (out, ext, mean, invstd, dgamma, dbeta, dz[:, :C2]):
            assert bool(torch.isfinite(t).all())
        assert bool(torch.isnan(dz[:, C2:]).all()) and bool((arg[1] == -1).all()) and bool((out[1] == 0).all()) and bool((arg[0] >= 0).all())
        assert bool((rm != 0).any()) and bool((rv != 1).any())


# ------------------------------------------------------------------------------------------------ the operator under autocast
class _Saved:
    """saved_tensors_hooks that record what an operator keeps for its backward."""

    def __init__(self):
        self.kept = []

    def __enter__(self):
        self.ctx = torch.autograd.graph.saved_tensors_hooks(self._pack, lambda t: t)
        self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)

    def _pack(self, t):
        self.kept.append((t.dtype, tuple(t.shape), t.data_ptr()))
        return t


def _bn_for(C2):
    d = R.columns(C2)
    bn = torch.nn.BatchNorm1d(C2, eps=R.BN_EPS, momentum=R.MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]), bn.bias.copy_(d["beta"]), bn.running_mean.copy_(d["running_mean"]), bn.running_var.copy_(d["running_var"])
    return bn.train()


def _operator_route(H, on, dtype, z16, index, bn0, g, grad=True):
    """ops.relu_bn_max under autocast(dtype) with ops.half_io = on, on a cloned leaf z and a cloned BatchNorm."""
    old, H.half_io = H.half_io, on
    try:
        bn = copy.deepcopy(bn0).cuda()
        z = z16.clone().cuda().requires_grad_()
        with torch.autocast("cuda", dtype=dtype), _Saved() as saved, torch.set_grad_enabled(grad):
            out = H.relu_bn_max(z, index, bn, R.M_DST)
        if grad:
            (out * g).sum().backward()
    finally:
        H.half_io = old
    r = dict(out=out.detach(), dz=z.grad, **{k: p.grad for k, p in bn.named_parameters()}, **{k: b.clone() for k, b in bn.named_buffers()})
    return r, saved.kept, z


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_operator_half_io_on_against_off(H, dtype):
    """ops.relu_bn_max under autocast of either dtype on a 16-bit z, C2 = 16, half_io on against off on cloned BatchNorms: the output
    (fp32), dz (z's dtype), the gradients of gamma and beta, the running statistics and num_batches_tracked bit for bit.  On: the
    caller's own 16-bit storage is what is saved and no fp32 [E, C2] tensor is; off: exactly one fp32 [E, C2] tensor is saved.  Under
    no_grad the output bits are the same, the statistics move identically and nothing is saved."""
    C2 = 16
    c, d = R.targets(), R.columns(C2)
    z16, index, g, bn0 = d["z"].to(dtype), c["index"].cuda(), d["g"].cuda(), _bn_for(C2)
    on, kept_on, z_on = _operator_route(H, True, dtype, z16, index, bn0, g)
    off, kept_off, _ = _operator_route(H, False, dtype, z16, index, bn0, g)
    assert set(on) == set(off) == {"out", "dz", "weight", "bias", "running_mean", "running_var", "num_batches_tracked"}
    for k in on:
        assert _same(on[k], off[k]), k
    assert on["out"].dtype == torch.float32 and on["out"].shape == (R.M_DST, C2) and on["dz"].dtype == dtype
    assert on["weight"].dtype == torch.float32 and on["bias"].dtype == torch.float32 and int(on["num_batches_tracked"]) == 1
    assert float(on["dz"].float().abs().max()) > 0 and not torch.equal(on["running_mean"].cpu(), d["running_mean"])
    big = tuple(z16.shape)
    assert sum(1 for dt, shape, _ in kept_on if dt == torch.float32 and shape == big) == 0, kept_on
    assert sum(1 for dt, shape, _ in kept_off if dt == torch.float32 and shape == big) == 1, kept_off
    assert (dtype, big, z_on.data_ptr()) in kept_on
    ng_on, kept, _ = _operator_route(H, True, dtype, z16, index, bn0, g, grad=False)
    ng_off, _, _ = _operator_route(H, False, dtype, z16, index, bn0, g, grad=False)
    assert not kept and ng_on["dz"] is None
    for k in ("out", "running_mean", "running_var", "num_batches_tracked"):
        assert _same(ng_on[k], ng_off[k]) and _same(ng_on[k], on[k]), k


# ------------------------------------------------------------------------------------------------ the layer
def _layer_route(H, on, dtype, c):
    from tests.test_gpu_ops_backward import _mlp
    old, H.half_io = H.half_io, on
    try:
        conv = H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), global_nn=None, add_self_loops=False).cuda().train()
        conv.fused_bn_max = True
        x, ps = c["x"].cuda().requires_grad_(), c["pos_src"].cuda().requires_grad_()
        with torch.autocast("cuda", dtype=dtype):
            out = conv(x, (ps, c["pos_dst"].cuda()), c["ei"].cuda())
        (out.float() * c["g"].cuda()).sum().backward()
    finally:
        H.half_io = old
    bn = conv.local_nn[1][2]
    return dict(out=out.detach(), x=x.grad, pos_src=ps.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                **{k: p.grad.clone() for k, p in conv.named_parameters()})


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layer_with_fused_bn_max_under_autocast(H, dtype, monkeypatch):
    """ops.PointNetConv(local_nn=MLP([12, 16, 32])) with fused_bn_max = True under autocast on the layer case of
    tests/test_gpu_bn_max.py: half_io on against off, the output, every gradient and the running statistics bit for bit; the layer-2
    GEMM's 16-bit output is what relu_bn_max is handed."""
    from tests.test_gpu_conv_train import _layer_case
    c = _layer_case(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    seen, inner = [], H._relu_bn_max_sorted
    monkeypatch.setattr(H, "_relu_bn_max_sorted", lambda z, *a: (seen.append(z.dtype), inner(z, *a))[1])
    on, off = _layer_route(H, True, dtype, c), _layer_route(H, False, dtype, c)
    assert seen == [dtype, dtype]
    assert set(on) == set(off) and len(on) >= 11
    for k in on:
        assert _same(on[k], off[k]), k
        assert bool(torch.isfinite(on[k]).all()), k
    assert on["out"].dtype == torch.float32 and float(on["x"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the whole network
def _net_step(H, dtype, on, flag, calls):
    """tests/test_gpu_train_net.py's training step (a freshly initialised train.Net(1, 8), two voxels of 600 and 200 points, the
    injected samples) as trainer.SemanticTraining takes it: float16 with GradScaler(512), bfloat16 with the scaler disabled."""
    from pointstowood_amd.loss import Poly1FocalLoss
    from pointstowood_amd.trainer import finish_step, set_fused_bn_max
    from tests import net_train_ref as NR
    from tests import test_gpu_train_net as TN
    old, H.half_io = H.half_io, on
    try:
        torch.manual_seed(TN.SEED)
        d = TN._data(NR.inputs(TN.SEED))
        net = TN._net(None)
        if flag:
            assert set_fused_bn_max(net) == 3
        criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
        optimizer = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
        scaler = torch.amp.GradScaler("cuda", init_scale=512, enabled=dtype == torch.float16)
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        optimizer.zero_grad()
        n0 = len(calls)
        with torch.autocast("cuda", dtype=dtype):
            outputs = net(d)
            loss, _ = criterion(outputs, d.y)
        scaler.scale(loss).backward()
        n_calls = len(calls) - n0
        skipped = finish_step(net, optimizer, scaler, "fp16" if dtype == torch.float16 else "bf16")
    finally:
        H.half_io = old
    r = dict(logits=outputs.detach(), loss=loss.detach(), **{"grad." + k: p.grad.clone() for k, p in net.named_parameters()},
             **{"state." + k: v.detach().clone() for k, v in net.state_dict().items()})
    moved = sum(1 for k, p in net.named_parameters() if not torch.equal(p.detach(), before[k]))
    return r, n_calls, skipped, moved


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_net_training_step_with_fused_bn_max(H, dtype, monkeypatch):
    """One whole step of train.Net with fused_bn_max set on its three PointNetConvs, under autocast with AdamW, ops.half_io on against
    off: the logits, the loss, every gradient (unscaled and clipped), every BatchNorm buffer and every parameter after the step bit
    for bit.  ops.relu_bn_max's worker is entered 3 times per step with the flag set, each time on a z of the autocast dtype, and
    never without the flag."""
    calls, inner = [], H._relu_bn_max_sorted
    monkeypatch.setattr(H, "_relu_bn_max_sorted", lambda z, *a: (calls.append(z.dtype), inner(z, *a))[1])
    on, n_on, skipped_on, moved = _net_step(H, dtype, True, True, calls)
    off, n_off, skipped_off, _ = _net_step(H, dtype, False, True, calls)
    assert n_on == n_off == 3 and calls == [dtype] * 6
    assert set(on) == set(off) and len([k for k in on if k.startswith("grad.")]) == 158
    for k in on:
        assert _same(on[k], off[k]), k
    assert on["logits"].dtype == torch.float32 and bool(torch.isfinite(on["logits"]).all()) and bool(torch.isfinite(on["loss"]))
    assert all(bool(torch.isfinite(v).all()) for k, v in on.items() if k.startswith("grad."))
    assert skipped_on == skipped_off == 0 and moved > 100
    plain, n_plain, _, _ = _net_step(H, dtype, True, False, calls)
    assert n_plain == 0 and len(calls) == 6 and set(plain) == set(on)


# ------------------------------------------------------------------------------------------------ the trainer
_vox = []


def _voxels():
    """The 8 synthetic labelled voxels of 200 - 487 points that the feed's end-to-end test trains on."""
    if not _vox:
        from pointstowood_amd import synthetic_voxels as synth
        for i in range(8):
            n = 200 + 41 * i
            p, refl = synth.uniform_points(2.0, n, 50 + i, reflectance=True)
            label = (torch.rand(n, generator=torch.Generator().manual_seed(i)) < 0.3).float()
            _vox.append(torch.cat([p, refl[:, None], label[:, None]], 1))
    return _vox


def _training_run(wdir, vox, **extra):
    from pointstowood_amd.trainer import SemanticTraining
    for part, which in (("train", range(8)), ("test", range(4, 8))):
        d = os.path.join(wdir, "data", part, "voxels")
        os.makedirs(d)
        for k, i in enumerate(which):
            torch.save(vox[i].clone(), os.path.join(d, f"voxel_{k}.pt"))
    args = argparse.Namespace(wdir=str(wdir), model="model.pth", trfile=os.path.join(wdir, "data", "train", "voxels"),
                              tefile=os.path.join(wdir, "data", "test", "voxels"), batch_size=4, num_epochs=2,
                              checkpoints=np.arange(0, 3, 2), augmentation=True, test=True, tune=False, stop_early=False, wandb=False,
                              seed=5, C=8, max_pts=16384, **extra)
    SemanticTraining(args)
    return open(os.path.join(wdir, "model", "model_history.csv"), "rb").read()


def test_semantic_training_with_fused_bn_max(H, tmp_path, monkeypatch):
    """trainer.SemanticTraining on 8 synthetic voxels (C = 8, batch_size 4, 2 epochs, --test --augmentation) with fused_bn_max=True:
    the fused operator runs, the 2 x 11 history is finite, a second run gives the same history bits, and the final checkpoint loads
    into route A with strict=True.  The class attribute stays False."""
    import pointstowood_amd
    calls, inner = [], H._relu_bn_max_sorted
    monkeypatch.setattr(H, "_relu_bn_max_sorted", lambda z, *a: (calls.append(z.dtype), inner(z, *a))[1])
    vox = _voxels()
    first = _training_run(str(tmp_path / "a"), vox, fused_bn_max=True)
    assert len(calls) == 3 * 2 * 2 and set(calls) == {torch.float16}                    # 3 levels x 2 training batches x 2 epochs
    h = np.loadtxt(tmp_path / "a" / "model" / "model_history.csv")
    assert h.shape == (2, 11) and np.isfinite(h).all() and h[:, 0].tolist() == [1.0, 2.0]
    assert (h[:, 1] > 0).all() and (h[:, 2] > 0).all() and ((h[:, 3:] >= 0) & (h[:, 3:] <= 1)).all()
    ck = torch.load(tmp_path / "a" / "model" / "model.pth", map_location="cpu")
    missing, unexpected = pointstowood_amd.Net(1, C=8).load_state_dict(ck["model_state_dict"], strict=True)
    assert not missing and not unexpected
    assert _training_run(str(tmp_path / "b"), vox, fused_bn_max=True) == first
    assert H.PointNetConv.fused_bn_max is False


def test_semantic_training_without_the_flag_is_unchanged(H, tmp_path, monkeypatch):
    """fused_bn_max=False gives the history bits of a namespace that never had the attribute, and relu_bn_max is never entered."""
    calls, inner = [], H._relu_bn_max_sorted
    monkeypatch.setattr(H, "_relu_bn_max_sorted", lambda z, *a: (calls.append(z.dtype), inner(z, *a))[1])
    vox = _voxels()
    absent = _training_run(str(tmp_path / "a"), vox)
    assert _training_run(str(tmp_path / "b"), vox, fused_bn_max=False) == absent
    assert not calls
