"""The bfloat16 element type of the training operators (include/p2w.h: P2W_BF16 in p2w_bn_chain_io, p2w_relu_bn_io and their backwards;
p2w_bn_relu_rowdot_bf16, p2w_segment_max_arg_bf16 and their backwards), ops.half_io on bfloat16 tensors, and the trainer under bfloat16 autocast (trainer.SemanticTraining with amp = "bf16", train.py --amp).

As in tests/test_gpu_half_io.py, whose cases, shapes and dtype-blind helpers these are: only the element type at the loads and stores
differs from the fp32 entry points, so nothing here has a tolerance.  The expected values are always the EXISTING fp32 entry point fed
z.bfloat16().float() (and g likewise); its fp32 results are compared bit for bit, and where the new code writes bfloat16 its result is
that fp32 result rounded to bfloat16 ON THE CPU (torch.Tensor.bfloat16(), pinned in tests/test_bf16_io_ref_cpu.py).  A NaN is compared
as a NaN, not by payload.  Outputs are pitched, NaN behind every row and one guard row in the output's own dtype behind the last."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import bf16_io_ref as BR
from tests import bn_chain_ref as R
from tests import head_ref as HD
from tests import test_gpu_bn_chain as TC
from tests import test_gpu_half_io as TF
from tests import test_gpu_head as TH
from tests.test_gpu_bn_chain import _pitch
from tests.test_gpu_half_io import _Saved, _buf, _chain_modules, _ibits, _pitched, _same, _widths

pytestmark = pytest.mark.gpu

EINVAL, ENULL, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
NAN = float("nan")
BF = torch.bfloat16
DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


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


def _bf_case(c):
    """The case with z and g rounded to bfloat16 (kept as fp32 tensors of those values: what the fp32 entry point is fed)."""
    return dict(c, z=c["z"].bfloat16().float(), g=c["g"].bfloat16().float())


# ------------------------------------------------------------------------------------------------ the chain
def _chain_forward(L, c, ld, tz, to, off=0, pre=False):
    """p2w_bn_chain_io (pre: p2w_relu_bn_io on the one stage) with z in DT[tz] and out in DT[to], pitched to ld, shifted by off elements."""
    _, ptr, stream = _abi()
    (M, C), nL = c["z"].shape, len(c["stages"])
    dev, arr = TC._device_stages(c)
    z = _pitched(c["z"], ld, DT[tz], off)
    res = None if c["res"] is None else _pitched(c["res"], ld, torch.float32)
    out = _buf(M + 1, ld, DT[to], off)
    mean, invstd = (torch.full((nL * C + 1,), NAN, device="cuda") for _ in range(2))
    need = int(L.p2w_relu_bn_ws_size(M, C) if pre else L.p2w_bn_chain_ws_size(M, C, nL))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if pre:
        d = dev[0]
        st = L.p2w_relu_bn_io(ptr(z), tz, ld, ptr(d["gamma"]), ptr(d["beta"]), ptr(d["rm"]), ptr(d["rv"]), R.MOMENTUM, R.BN_EPS, M, C, ptr(out), to, ld,
                              ptr(mean), ptr(invstd), ptr(ws), need, stream())
    else:
        st = L.p2w_bn_chain_io(ptr(z), tz, ld, ptr(res), ld, arr, nL, M, C, ptr(out), to, ld, ptr(mean), ptr(invstd), ptr(ws), need, stream())
    assert st == 0
    torch.cuda.synchronize()
    assert out.dtype == DT[to] and bool(torch.isnan(out[M]).all()) and bool(torch.isnan(out[:, C:]).all()) and bool(torch.isnan(z[:, C:]).all())
    assert bool(torch.isnan(mean[nL * C])) and bool(torch.isnan(invstd[nL * C]))
    assert all(bool(torch.isnan(d["rm"][C])) and bool(torch.isnan(d["rv"][C])) for d in dev)
    got = dict(out=out[:M, :C], mean=mean[:nL * C].view(nL, C), invstd=invstd[:nL * C].view(nL, C),
               running_mean=torch.stack([d["rm"][:C] for d in dev]), running_var=torch.stack([d["rv"][:C] for d in dev]))
    return {k: v.cpu() for k, v in got.items()}


def _chain_backward(L, c, ld, fwd, tz, to, off=0, pre=False):
    """p2w_bn_chain_bwd_io / p2w_relu_bn_bwd_io on the fp32 forward's out, mean and invstd: g in DT[to], z and dz in DT[tz]."""
    _, ptr, stream = _abi()
    (M, C), nL = c["z"].shape, len(c["stages"])
    dev, arr = TC._device_stages(c)
    has_res = c["res"] is not None
    g, z = _pitched(c["g"], ld, DT[to], off), _pitched(c["z"], ld, DT[tz], off)
    outp = _pitched(fwd["out"], ld, torch.float32) if has_res else None
    dz = _buf(M + 1, ld, DT[tz], off)
    dres = _buf(M + 1, ld, torch.float32) if has_res else None
    mean, invstd = fwd["mean"].reshape(-1).cuda(), fwd["invstd"].reshape(-1).cuda()
    vecs = [torch.full((nL * C + 1,), NAN, device="cuda") for _ in range(4)]
    need = int(L.p2w_bn_chain_ws_size(M, C, nL))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if pre:
        st = L.p2w_relu_bn_bwd_io(ptr(g), to, ld, ptr(z), tz, ld, ptr(dev[0]["gamma"]), ptr(mean), ptr(invstd), M, C, ptr(dz), ld, ptr(vecs[0]),
                                  ptr(vecs[1]), ptr(ws), need, stream())
    else:
        st = L.p2w_bn_chain_bwd_io(ptr(g), to, ld, ptr(z), tz, ld, ptr(outp), ld, arr, nL, ptr(mean), ptr(invstd), M, C, ptr(dz), ld, ptr(dres), ld,
                                   *[ptr(v) for v in vecs], ptr(ws), need, stream())
    assert st == 0
    torch.cuda.synchronize()
    for t in (dz, dres):
        assert t is None or (bool(torch.isnan(t[M]).all()) and bool(torch.isnan(t[:, C:]).all()))
    assert all(bool(torch.isnan(v[nL * C])) for v in vecs)
    got = dict(dz=dz[:M, :C].cpu(), dres=None if dres is None else dres[:M, :C].cpu())
    names = ("dgamma", "dbeta") if pre else ("dgamma", "dbeta", "ddw_w", "ddw_b")
    got.update({k: v[:nL * C].view(nL, C).cpu() for k, v in zip(names, vecs)})
    return got


_refs = {}


def _chain_reference(L, name, C, M):
    """The fp32 entry points on the bfloat16-valued case, once per case: (case, forward, backward)."""
    if (name, C, M) not in _refs:
        c = _bf_case(R.case(name, C, M))
        fwd = TC._forward(L, c, _pitch(C))
        _refs[name, C, M] = (c, fwd, TC._backward(L, c, _pitch(C), fwd))
    return _refs[name, C, M]


def _check_forward(got, ref, to):
    for k in ("mean", "invstd", "running_mean", "running_var"):
        assert _same(got[k], ref[k]), k
    assert _same(got["out"], ref["out"] if to == F32 else ref["out"].bfloat16()), "out"


def _check_backward(got, ref, tz):
    for k in ref:
        if k != "dz":
            assert _same(got[k], ref[k]), k
    assert _same(got["dz"], ref["dz"] if tz == F32 else ref["dz"].bfloat16()), "dz"


CASES = TC.CASES


@pytest.mark.parametrize("name,C,M", CASES)
def test_chain_forward(L, name, C, M):
    """p2w_bn_chain_io on a bfloat16 z, out in fp32 and in bfloat16: mean, invstd, the running statistics and the fp32 out are the fp32
    entry point's bits on the widened z; the bfloat16 out is its fp32 out rounded on the CPU.  Both access widths (the narrow one
    forced by an odd pitch and by a pointer one element off) and a second call give the same bits; nothing is written behind a row."""
    c, ref, _ = _chain_reference(L, name, C, M)
    for to in (F32, BF16):
        for ld, off in _widths(C) + [(_pitch(C), 0)]:
            _check_forward(_chain_forward(L, c, ld, BF16, to, off), ref, to)


@pytest.mark.parametrize("name,C,M", CASES)
def test_chain_backward(L, name, C, M):
    """p2w_bn_chain_bwd_io with g in bfloat16 (and in fp32, the chain whose result stayed fp32): dgamma, dbeta, ddw_w, ddw_b (exactly
    0) and dres are the fp32 route's bits, the bfloat16 dz is its dz rounded on the CPU; both widths, and a second call."""
    c, fwd, ref = _chain_reference(L, name, C, M)
    assert bool((ref["ddw_b"] == 0).all())
    for to in (BF16, F32):
        for ld, off in _widths(C) + [(_pitch(C), 0)]:
            _check_backward(_chain_backward(L, c, ld, fwd, BF16, to, off), ref, BF16)


@pytest.mark.parametrize("name,C,up", [("tail", 16, 114), ("project", 132, 124)])
def test_chain_backward_reaches_subnormals_and_infinities(L, name, C, up):
    """g scaled by 2^-128 in a third of the columns and by 2^up in another third (|g| stays finite in bfloat16).  The bfloat16 dz then
    holds subnormal elements (below 2^-126: bfloat16's and fp32's subnormals share their range, so nothing may be flushed on the way)
    and infinite ones, at least 100 of each, and still equals the fp32 route's dz rounded on the CPU, at the 8-byte and at the 2-byte
    access width.  The infinities are column CONST's: its variance is 0, so every stage multiplies its gradient by gamma / sqrt(eps)
    = 316 gamma.  2^up is the largest power at which only the LAST multiplication of dz leaves fp32's range there (one stage: 2^124
    x 316 gamma; two: 2^114 x 316^2 gamma gamma') - were a stage's result infinite before the last one, its column mean would be too
    and the column would be inf - inf = NaN; the float64 chain on the CPU puts about 2 000 and 1 600 of the column's 4 133 elements
    past 2^128 at these two powers."""
    c = R.case(name, C)
    scale = torch.ones(C)
    scale[torch.arange(C) % 3 == 1], scale[torch.arange(C) % 3 == 2] = 2.0 ** up, 2.0 ** -128
    assert R.CONST % 3 == 1
    c = _bf_case(dict(c, g=c["g"] * scale))
    assert bool(torch.isfinite(c["g"]).all())
    fwd = TC._forward(L, c, _pitch(C))
    ref = TC._backward(L, c, _pitch(C), fwd)
    for ld, off in _widths(C):
        got = _chain_backward(L, c, ld, fwd, BF16, BF16, off)
        _check_backward(got, ref, BF16)
    dz = got["dz"].float()
    sub, inf = int(((dz != 0) & (dz.abs() < 2.0 ** -126)).sum()), int(torch.isinf(dz).sum())
    print(f"BF16IO dz {name} C={C}: {sub} subnormal, {inf} infinite of {dz.numel()}")
    assert sub >= 100 and inf >= 100


@pytest.mark.parametrize("C", R.WIDTHS)
def test_the_store_rounds_the_whole_table(L, C):
    """One stage, no ReLU, gamma = 0 in every column: out[:, c] == beta[c] exactly, and beta carries tests/bf16_io_ref.py's table, C
    values per call - every tie, the carry to infinity, every subnormal case, the zeros, the infinities and the NaNs (those with a
    payload in the low 16 bits only among them) go through the kernels' one store helper, at both access widths.  The bfloat16 out is
    held to the fp32 entry point's out rounded on the CPU and to the table's own bits."""
    M = 70
    table = torch.from_numpy(BR.TABLE32.copy())
    want16 = torch.from_numpy(BR.TABLE16.view(np.int16).copy())
    assert np.array_equal(table.numpy().view(np.uint32)[~np.isnan(BR.TABLE32)], BR.TABLE32.view(np.uint32)[~np.isnan(BR.TABLE32)])
    base = R.case("one", C, M)
    for lo in range(0, len(table), C):
        idx = (torch.arange(C) + lo) % len(table)
        st = dict(base["stages"][0], a=None, b=None, gamma=torch.zeros(C), beta=table[idx].clone(), relu=False)
        z = base["z"].clone()
        z[:, R.CONST] = torch.linspace(-1, 1, M)
        c = _bf_case(dict(base, z=z, stages=[st], res=None))
        ref = TC._forward(L, c, _pitch(C))
        live = ~torch.isnan(st["beta"])
        assert torch.equal(_ibits(ref["out"])[:, live & (st["beta"] != 0)], _ibits(st["beta"])[live & (st["beta"] != 0)].expand(M, -1))
        assert bool((ref["out"][:, live] == st["beta"][live]).all()) and bool(torch.isnan(ref["out"][:, ~live]).all())
        for ld, off in _widths(C):
            _check_forward(_chain_forward(L, c, ld, BF16, F32, off), ref, F32)
            got = _chain_forward(L, c, ld, BF16, BF16, off)
            _check_forward(got, ref, BF16)
            pin = live & (st["beta"] != 0)                                         # (a zero's sign is xhat's: it is in the comparison above)
            assert torch.equal(_ibits(got["out"])[:, pin], want16[idx][pin].expand(M, -1)), lo
            assert bool(torch.isnan(got["out"][:, ~live]).all())


def _relu_bn_case(C, M):
    """bn_chain_ref's one-stage case without the depthwise convolution, column ALL_NEG of z all negative (relu(z) is constant 0 there)."""
    c = R.case("one", C, M)
    z = c["z"].clone()
    z[:, R.ALL_NEG] = -z[:, R.ALL_NEG].abs() - 0.125
    return _bf_case(dict(c, z=z, stages=[dict(c["stages"][0], a=None, b=None, relu=False)], res=None))


@pytest.mark.parametrize("C,M", [(C, R.M_ROWS) for C in R.WIDTHS] + [(6, 2), (16, 2)])
def test_relu_bn(L, C, M):
    """p2w_relu_bn_io / p2w_relu_bn_bwd_io (the PRE instantiations) as the two chain tests, against p2w_relu_bn / p2w_relu_bn_bwd; the
    all-negative column has mean 0, invstd 1 / sqrt(eps) and dz exactly 0."""
    c = _relu_bn_case(C, M)
    fwd, bwd = TF._relu_bn_reference(L, c, _pitch(C))
    assert float(fwd["mean"][0, R.ALL_NEG]) == 0.0 and bool((bwd["dz"][:, R.ALL_NEG] == 0).all()) and float(bwd["dz"].abs().max()) > 0
    for to in (F32, BF16):
        for ld, off in _widths(C) + [(_pitch(C), 0)]:
            _check_forward(_chain_forward(L, c, ld, BF16, to, off, pre=True), fwd, to)
            _check_backward(_chain_backward(L, c, ld, fwd, BF16, to, off, pre=True), bwd, BF16)


# ------------------------------------------------------------------------------------------------ the head
def _head_run(L, c, ld, off=0):
    """p2w_bn_relu_rowdot_bf16 / _bwd_bf16 on z in bfloat16, dz in bfloat16."""
    _, ptr, stream = _abi()
    M, C = c["z"].shape
    z = _pitched(c["z"], ld, BF, off)
    gamma, beta, w, bias, g = (c[k].cuda() for k in ("gamma", "beta", "w", "bias", "g"))
    rm, rv = (torch.cat([c[k], torch.full((1,), NAN)]).cuda() for k in ("rm", "rv"))
    dz = _buf(M + 1, ld, BF, off)
    mean, invstd, dgamma, dbeta, dw = (torch.full((C + 1,), NAN, device="cuda") for _ in range(5))
    dbias, logit = torch.full((2,), NAN, device="cuda"), torch.full((M + 1,), NAN, device="cuda")
    need = int(L.p2w_bn_relu_rowdot_ws_size(M, C))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_bn_relu_rowdot_bf16(ptr(z), ld, ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(rm), ptr(rv), HD.MOMENTUM, HD.BN_EPS, M, C,
                                   ptr(logit), ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
    assert L.p2w_bn_relu_rowdot_bwd_bf16(ptr(g), ptr(z), ld, ptr(gamma), ptr(beta), ptr(w), ptr(mean), ptr(invstd), M, C, ptr(dz), ld,
                                       ptr(dgamma), ptr(dbeta), ptr(dw), ptr(dbias), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(logit[M])) and bool(torch.isnan(dw[C])) and bool(torch.isnan(dbias[1]))
    assert bool(torch.isnan(dz[M]).all()) and bool(torch.isnan(dz[:, C:]).all())
    for t in (mean, invstd, dgamma, dbeta, rm, rv):
        assert bool(torch.isnan(t[C]))
    r = dict(logit=logit[:M], dw=dw[:C], dbias=dbias[:1], dz=dz[:M, :C], mean=mean[:C], invstd=invstd[:C], dgamma=dgamma[:C], dbeta=dbeta[:C],
             running_mean=rm[:C], running_var=rv[:C])
    return {k: v.contiguous().cpu() for k, v in r.items()}


@pytest.mark.parametrize("C", [6, 16, 512])
@pytest.mark.parametrize("M", [2, 15, R.M_ROWS])
def test_head(L, M, C):
    """p2w_bn_relu_rowdot_bf16 / _bwd_bf16 on a bfloat16 z (C = 512: two 256-column passes of the row sums): the logits, mean, invstd, the
    running statistics, dgamma, dbeta, dw and dbias are p2w_bn_relu_rowdot / _bwd's bits on the widened z; the bfloat16 dz is their dz
    rounded on the CPU; both access widths."""
    c = HD.case(M, C)
    c = dict(c, z=c["z"].bfloat16().float())
    ref = TH._run(L, c, _pitch(C))
    for ld, off in _widths(C):
        got = _head_run(L, c, ld, off)
        for k in ref:
            assert _same(got[k], ref[k].bfloat16() if k == "dz" else ref[k]), (k, ld, off)


# ------------------------------------------------------------------------------------------------ the segment max
N_SEG = TF.N_SEG


def _segmax_case(F, many):
    """The float16 file's case (a planted tie, +-inf, -0 against +0, a NaN among numbers, columns of NaN and of -inf only, an empty
    segment), its values rounded to bfloat16: the planted ones are exact in it."""
    ptr_, x, gout = TF._segmax_case(F, many)
    return ptr_, x.float().bfloat16(), gout


def _segmax_run(L, ptr_, x, gout, ld, off=0):
    from pointstowood_amd._lib import ptr, stream
    (n, F), B = x.shape, ptr_.numel() - 1
    xp = _pitched(x, ld, BF, off)
    csr, go = ptr_.cuda(), _pitched(gout, F + 4, torch.float32)
    out, arg = torch.full((B * F + 1,), NAN, device="cuda"), torch.full((B * F + 1,), -7, dtype=torch.int32, device="cuda")
    gx = _buf(n + 1, ld, BF, off)
    assert L.p2w_segment_max_arg_bf16(ptr(xp), ld, F, ptr(csr), B, ptr(out), ptr(arg), stream()) == 0
    assert L.p2w_segment_max_bwd_bf16(ptr(go), F + 4, ptr(arg), ptr(csr), B, F, ptr(gx), ld, n, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * F])) and int(arg[B * F]) == -7 and bool(torch.isnan(gx[n]).all()) and bool(torch.isnan(gx[:, F:]).all())
    return dict(out=out[:B * F].view(B, F).cpu(), arg=arg[:B * F].view(B, F).cpu(), grad_x=gx[:n, :F].cpu())


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("F", [6, 16, 132])
def test_segment_max(L, F, many):
    """p2w_segment_max_arg_bf16 / p2w_segment_max_bwd_bf16 on a bfloat16 x, on both routes of the forward: out and arg are the fp32 entry
    point's on the widened x (NaN handling is whatever that kernel does); grad_x is its grad_x rounded on the CPU, in bfloat16, exact
    zeros on every losing row; pitched rows, guard rows, both access widths."""
    ptr_, x, gout = _segmax_case(F, many)
    ref = TF._segmax_reference(L, ptr_, x, gout, _pitch(F))
    B = ptr_.numel() - 1
    assert int(ref["arg"][6, 0]) == int(ptr_[6]) + 5 and int(ref["arg"][4, 5]) == -1 and float(ref["out"][6, 1]) == float("inf")
    assert bool((ref["arg"][0] == -1).all()) and bool((ref["out"][0] == 0).all())                     # the empty segment
    assert int((ref["grad_x"] != 0).sum()) <= B * F and int((ref["grad_x"] != 0).sum()) > B * F // 2
    for ld, off in _widths(F):
        got = _segmax_run(L, ptr_, x, gout, ld, off)
        assert _same(got["out"], ref["out"]) and torch.equal(got["arg"], ref["arg"]), (ld, off)
        assert got["grad_x"].dtype == BF and _same(got["grad_x"], ref["grad_x"].bfloat16()), (ld, off)
        win = torch.zeros(N_SEG, F, dtype=torch.bool)
        rows, cols = ref["arg"].clamp_min(0), torch.arange(F).expand(B, F)
        win[rows[ref["arg"] >= 0], cols[ref["arg"] >= 0]] = True
        assert bool((_ibits(got["grad_x"])[~win] == 0).all())                                         # +0, not -0, not a rounding's leftover


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(L):
    """A float16 / bfloat16 mix either way, a bfloat16 out (or g) with an fp32 z and the unknown code 3: P2W_EUNSUPPORTED from the four
    chain entry points, ahead of every other check; then the null, size, alignment and workspace refusals of the namesakes from the
    chain entry points on bfloat16 tensors and from the head's and the segment max's bfloat16 entry points.  Nothing is launched:
    the NaN-filled outputs stay NaN and the running statistics stay put.  Then the good calls write them."""
    BnStage, ptr, stream = _abi()
    M, C, ld = 14, 8, 12
    z16, g16, out16, dz16 = (torch.full((M, ld), NAN, dtype=BF, device="cuda") for _ in range(4))
    z16[:, :C], g16[:, :C] = torch.randn(M, C).bfloat16().cuda(), torch.randn(M, C).bfloat16().cuda()
    gamma, beta, w = (torch.rand(C, device="cuda") + 0.5 for _ in range(3))
    bias, gl = torch.zeros(1, device="cuda"), torch.randn(M, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    mean, invstd, dgamma, dbeta, dw, logit = (torch.full((n,), NAN, device="cuda") for n in (C, C, C, C, C, M))
    dbias = torch.full((1,), NAN, device="cuda")
    arr = (BnStage * 1)()
    arr[0] = BnStage(None, None, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5, 1)
    need = max(int(L.p2w_bn_chain_ws_size(M, C, 1)), int(L.p2w_bn_relu_rowdot_ws_size(M, C)))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    csr = torch.tensor([0, 5, M], dtype=torch.int32, device="cuda")
    sout, sarg = torch.full((2, C), NAN, device="cuda"), torch.full((2, C), -7, dtype=torch.int32, device="cuda")
    sgo, gx16 = torch.randn(2, ld, device="cuda"), torch.full((M, ld), NAN, dtype=BF, device="cuda")
    s = stream()

    def chain(z=ptr(z16), tz=BF16, out=ptr(out16), to=BF16, M_=M, ldz=ld, ws_=ptr(ws), wsb=need, mean_=ptr(mean)):
        return L.p2w_bn_chain_io(z, tz, ldz, None, 0, arr, 1, M_, C, out, to, ld, mean_, ptr(invstd), ws_, wsb, s)

    def chain_bwd(g=ptr(g16), to=BF16, tz=BF16, dz=ptr(dz16), wsb=need, ws_=ptr(ws), lddz=ld):
        return L.p2w_bn_chain_bwd_io(g, to, ld, ptr(z16), tz, ld, None, 0, arr, 1, ptr(mean), ptr(invstd), M, C, dz, lddz, None, 0, ptr(dgamma),
                                     ptr(dbeta), None, None, ws_, wsb, s)

    def relu_bn(tz=BF16, to=BF16, out=ptr(out16)):
        return L.p2w_relu_bn_io(ptr(z16), tz, ld, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5, M, C, out, to, ld, ptr(mean), ptr(invstd),
                                ptr(ws), need, s)

    def relu_bn_bwd(to=BF16, tz=BF16, dz=ptr(dz16)):
        return L.p2w_relu_bn_bwd_io(ptr(g16), to, ld, ptr(z16), tz, ld, ptr(gamma), ptr(mean), ptr(invstd), M, C, dz, ld, ptr(dgamma), ptr(dbeta),
                                    ptr(ws), need, s)

    def head(z=ptr(z16), wsb=need):
        return L.p2w_bn_relu_rowdot_bf16(z, ld, ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(rm), ptr(rv), 0.1, 1e-5, M, C, ptr(logit), ptr(mean),
                                       ptr(invstd), ptr(ws), wsb, s)

    def head_bwd(dz=ptr(dz16), ws_=ptr(ws)):
        return L.p2w_bn_relu_rowdot_bwd_bf16(ptr(gl), ptr(z16), ld, ptr(gamma), ptr(beta), ptr(w), ptr(mean), ptr(invstd), M, C, dz, ld,
                                           ptr(dgamma), ptr(dbeta), ptr(dw), ptr(dbias), ws_, need, s)

    def seg(x=ptr(z16), ldx=ld):
        return L.p2w_segment_max_arg_bf16(x, ldx, C, ptr(csr), 2, ptr(sout), ptr(sarg), s)

    def seg_bwd(gx=ptr(gx16)):
        return L.p2w_segment_max_bwd_bf16(ptr(sgo), ld, ptr(sarg), ptr(csr), 2, C, gx, ld, M, s)

    for tz, to in ((BF16, F16), (F16, BF16), (F32, BF16), (BF16, 3), (3, BF16), (3, F32), (3, 3)):
        assert chain(tz=tz, to=to) == EUNSUPPORTED and chain_bwd(tz=tz, to=to) == EUNSUPPORTED, (tz, to)
        assert relu_bn(tz=tz, to=to) == EUNSUPPORTED and relu_bn_bwd(tz=tz, to=to) == EUNSUPPORTED, (tz, to)
    assert chain(tz=BF16, to=F16, z=None) == EUNSUPPORTED and chain(tz=3, z=None) == EUNSUPPORTED        # ... ahead of every other check
    assert chain(z=None) == ENULL and chain(out=None) == ENULL and chain(mean_=None) == ENULL and chain_bwd(g=None) == ENULL
    assert chain_bwd(dz=None) == ENULL and head(z=None) == ENULL and head_bwd(dz=None) == ENULL and seg(x=None) == ENULL and seg_bwd(gx=None) == ENULL
    assert chain(M_=1) == EINVAL and chain(ldz=C - 1) == EINVAL and chain_bwd(lddz=C - 1) == EINVAL and seg(ldx=C - 1) == EINVAL
    assert chain(ws_=ptr(ws) + 8) == EALIGN and chain_bwd(ws_=ptr(ws) + 4) == EALIGN and head_bwd(ws_=ptr(ws) + 8) == EALIGN
    assert chain(wsb=need - 1 - 256) == EWORKSPACE and chain_bwd(wsb=0) == EWORKSPACE and head(wsb=16) == EWORKSPACE
    torch.cuda.synchronize()
    for t in (out16, dz16, gx16, mean, invstd, dgamma, dbeta, dw, logit, dbias, sout):
        assert bool(torch.isnan(t).all())
    assert bool((rm == 0).all()) and bool((rv == 1).all()) and bool((sarg == -7).all())
    assert chain() == 0 and chain_bwd() == 0 and relu_bn() == 0 and relu_bn_bwd() == 0 and head() == 0 and head_bwd() == 0
    assert seg() == 0 and seg_bwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out16[:, :C]).all()) and bool(torch.isfinite(dz16[:, :C]).all()) and bool(torch.isnan(out16[:, C:]).all())
    assert bool(torch.isnan(dz16[:, C:]).all()) and bool(torch.isfinite(logit).all()) and bool((rm != 0).any()) and bool((sarg >= 0).all())
    assert bool(torch.isfinite(gx16[:, :C]).all()) and bool(torch.isnan(gx16[:, C:]).all()) and int((gx16[:, :C] != 0).sum()) == 2 * C


# ------------------------------------------------------------------------------------------------ the operators under autocast
def _operator_route(H, on, run, z16, extra=()):
    """run(z, *extra leaves) -> (out, modules) under bfloat16 autocast with ops.half_io = on; z16 and the extra tensors are cloned
    leaves.  Returns the output, every gradient, the BatchNorms' buffers and what was saved."""
    old = H.half_io
    H.half_io = on
    try:
        z = z16.clone().cuda().requires_grad_()
        leaves = [t.clone().cuda().requires_grad_() for t in extra]
        with torch.autocast("cuda", dtype=BF), _Saved() as saved:
            out, mods = run(z, *leaves)
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(out.dtype).cuda()
        (out.float() * cot.float()).sum().backward()
    finally:
        H.half_io = old
    r = dict(out=out.detach(), dz=z.grad)
    r.update({f"leaf{i}": t.grad for i, t in enumerate(leaves)})
    for i, m in enumerate(mods):
        r.update({f"m{i}.{k}": p.grad for k, p in m.named_parameters()})
        r.update({f"m{i}.{k}": b.clone() for k, b in m.named_buffers()})
    return r, saved.kept, z


def _compare_routes(H, run, z16, extra=(), out_dtype=torch.float32, fp32_saves=0):
    """on against off: the same bits everywhere; on saves the caller's bfloat16 z and no fp32 tensor of its shape (but `fp32_saves`:
    the residual chain's out), off saves the fp32 copy."""
    on, kept_on, z_on = _operator_route(H, True, run, z16, extra)
    off, kept_off, _ = _operator_route(H, False, run, z16, extra)
    assert set(on) == set(off)
    for k in on:
        assert _same(on[k], off[k]), k
    assert on["out"].dtype == out_dtype and on["dz"].dtype == BF and float(on["dz"].float().abs().nan_to_num().max()) > 0
    big = tuple(z16.shape)
    assert sum(1 for dt, shape, _ in kept_on if dt == torch.float32 and shape == big) == fp32_saves, kept_on
    assert sum(1 for dt, shape, _ in kept_off if dt == torch.float32 and shape == big) == fp32_saves + 1, kept_off
    assert (BF, big, z_on.data_ptr()) in kept_on
    return on, kept_on, z_on


@pytest.mark.parametrize("name,bf_out", [("one", False), ("one", True), ("expand", True), ("tail", False), ("middle", True), ("middle", False),
                                         ("project", False), ("two_res", False), ("three_res", False)])
def test_operator_bn_chain(H, name, bf_out):
    """ops.bn_chain under bfloat16 autocast on a bfloat16 z, L = 1, 2, 3, with and without a residual, out_dtype None and bfloat16:
    half_io on against off on cloned inputs and modules - the output, every gradient, the running statistics and num_batches_tracked
    bit for bit.  On: z's own storage is what is saved, and no fp32 [M, C] tensor but the residual chain's out; off: the fp32 copy is
    there.  out_dtype must be z's own dtype."""
    c = R.case(name, 16)
    has_res = c["res"] is not None

    def run(z, *res):
        mods = _chain_modules(c)
        out = H.bn_chain(z, mods, res[0] if res else None, out_dtype=BF if bf_out else None)
        return out, [m for st in mods for m in st if isinstance(m, torch.nn.Module)]

    on, _, _ = _compare_routes(H, run, c["z"].bfloat16(), (c["res"],) if has_res else (), BF if bf_out else torch.float32,
                               fp32_saves=1 if has_res else 0)
    assert all(int(v) == 1 for k, v in on.items() if k.endswith("num_batches_tracked"))
    if has_res:
        assert on["leaf0"].dtype == torch.float32
        with pytest.raises(RuntimeError, match="residual"):
            H.bn_chain(c["z"].bfloat16().cuda(), _chain_modules(c), c["res"].cuda(), out_dtype=BF)
    for z in (c["z"].cuda(), c["z"].half().cuda()):
        with pytest.raises(RuntimeError, match="bfloat16"):
            H.bn_chain(z, _chain_modules(c), out_dtype=BF)
    with pytest.raises(RuntimeError, match="float16"):
        H.bn_chain(c["z"].bfloat16().cuda(), _chain_modules(c), out_dtype=torch.float16)


def test_operator_relu_bn(H):
    c = _relu_bn_case(16, R.M_ROWS)
    for bf_out in (False, True):
        def run(z):
            bn = TC._modules(c)[0][0]
            return H.relu_bn(z, bn, out_dtype=BF if bf_out else None), [bn]
        _compare_routes(H, run, c["z"].bfloat16(), out_dtype=BF if bf_out else torch.float32)


def test_operator_bn_relu_rowdot(H):
    c = HD.case(257, 16)

    def run(z):
        bn = torch.nn.BatchNorm1d(16, eps=HD.BN_EPS, momentum=HD.MOMENTUM).cuda().train()
        conv = torch.nn.Conv1d(16, 1, 1).cuda()
        with torch.no_grad():
            bn.weight.copy_(c["gamma"]), bn.bias.copy_(c["beta"]), bn.running_mean.copy_(c["rm"]), bn.running_var.copy_(c["rv"])
            conv.weight.copy_(c["w"].view(1, 16, 1)), conv.bias.copy_(c["bias"])
        return H.bn_relu_rowdot(z, bn, conv.weight, conv.bias), [bn, conv]

    _compare_routes(H, run, c["z"].bfloat16())


@pytest.mark.parametrize("many", [False, True])
def test_operator_scatter_max(H, many):
    """ops.scatter_max fed a bfloat16 tensor under autocast, on both routes of the forward: on against off bit for bit; the output is
    fp32, the gradient bfloat16.  Neither route saves x (only the winners), so - as in the float16 file - what shows that on took the
    bfloat16 kernels is the peak memory of a forward and backward: off allocates an fp32 copy of x [n, F] in the forward and an fp32
    grad_x [n, F] next to its rounding in the backward, on allocates neither, so off's peak is 4 n F bytes above on's (less the
    caching allocator's rounding of a block to 512 bytes, once per route)."""
    ptr_, x, _ = _segmax_case(16, many)
    nb = ptr_.numel() - 1
    index = torch.repeat_interleave(torch.arange(nb), (ptr_[1:] - ptr_[:-1]).long()).cuda()

    def run(z):
        return H.scatter_max(z, index, dim=0, dim_size=nb)[0], []

    on, kept_on, _ = _operator_route(H, True, run, x)
    off, kept_off, _ = _operator_route(H, False, run, x)
    for k in on:
        assert _same(on[k], off[k]), k
    assert on["out"].dtype == torch.float32 and on["dz"].dtype == BF
    assert not any(shape == tuple(x.shape) for _, shape, _ in kept_on + kept_off)

    cot = torch.randn(nb, x.shape[1], device="cuda")
    peak = {}
    for route in (True, False):
        old, H.half_io = H.half_io, route
        try:
            z = x.clone().cuda().requires_grad_()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with torch.autocast("cuda", dtype=BF):
                out = run(z)[0]
            out.backward(cot)
            torch.cuda.synchronize()
            peak[route] = torch.cuda.max_memory_allocated() - base
            del out, z
        finally:
            H.half_io = old
    print(f"BF16IO_SCATTER_PEAK on {peak[True]} off {peak[False]} fp32 x {4 * x.numel()}")
    assert peak[False] - peak[True] >= 4 * x.numel() - 2 * 512


def test_gemm_dtype_follows_the_running_autocast_dtype(H):
    """ops._gemm_dtype: z's dtype where it is the running autocast dtype and half_io is on, None otherwise."""
    zb, zh = torch.zeros(2, 4, dtype=BF, device="cuda"), torch.zeros(2, 4, dtype=torch.float16, device="cuda")
    assert H._gemm_dtype(zb) is None and H._gemm_dtype(zh) is None
    with torch.autocast("cuda", dtype=BF):
        assert H._gemm_dtype(zb) == BF and H._gemm_dtype(zh) is None and H._gemm_dtype(zb.float()) is None
    with torch.autocast("cuda", dtype=torch.float16):
        assert H._gemm_dtype(zh) == torch.float16 and H._gemm_dtype(zb) is None
    old, H.half_io = H.half_io, False
    try:
        with torch.autocast("cuda", dtype=BF):
            assert H._gemm_dtype(zb) is None
    finally:
        H.half_io = old


# ------------------------------------------------------------------------------------------------ the whole network
def _train_step_bf16():
    """tests/test_gpu_train_net.py's training step under bfloat16 autocast, as trainer.SemanticTraining takes it with amp = "bf16": the
    scaler disabled, clip_grad_norm_, AdamW through trainer.finish_step."""
    from pointstowood_amd.loss import Poly1FocalLoss
    from pointstowood_amd.trainer import finish_step
    from tests import net_train_ref as NR
    from tests import test_gpu_train_net as TN
    torch.manual_seed(TN.SEED)
    d = TN._data(NR.inputs(TN.SEED))
    net = TN._net(None)
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    optimizer = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=512, enabled=False)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    optimizer.zero_grad()
    with torch.autocast("cuda", dtype=BF):
        outputs = net(d)
        loss, _ = criterion(outputs, d.y)
    scaler.scale(loss).backward()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    assert finish_step(net, optimizer, scaler, "bf16") == 0
    return net, outputs.detach(), loss.detach(), grads, before


def test_net_training_step_is_the_same_with_the_switch_on_and_off(H):
    """One whole step of train.Net (C = 8, voxels of 600 and 200 points, the injected samples) under bfloat16 autocast with AdamW,
    ops.half_io off and on: the logits, the loss, every gradient, every running statistic and every parameter after the step bit for
    bit; on a second time gives the same bits again; the step moved the parameters."""
    runs = []
    for on in (False, True, True):
        old = H.half_io
        H.half_io = on
        try:
            net, logits, loss, grads, before = _train_step_bf16()
        finally:
            H.half_io = old
        runs.append(dict(logits=logits, loss=loss, **{"grad." + k: v for k, v in grads.items()},
                         **{"state." + k: v.detach().clone() for k, v in net.state_dict().items()}))
        moved = sum(1 for k, p in net.named_parameters() if not torch.equal(p.detach(), before[k]))
        del net
    off, on, again = runs
    assert set(off) == set(on) and len([k for k in on if k.startswith("grad.")]) == 158 and moved > 100
    for k in off:
        assert _same(on[k], off[k]), k
        assert _same(on[k], again[k]), k
    assert on["logits"].dtype == torch.float32 and bool(torch.isfinite(on["logits"]).all()) and bool(torch.isfinite(on["loss"]))
    assert all(v is not None and bool(torch.isfinite(v).all()) for k, v in on.items() if k.startswith("grad."))


def test_unfused_head_under_bfloat16_and_the_loss_on_bfloat16_logits():
    """train.Net with fused = False under bfloat16 autocast: the head's last convolution runs in bfloat16 and the forward ends, as the
    reference's, with .to(torch.float) - fp32 logits, as the fused head gives; the loss is fp32 and every parameter gradient finite.
    loss.Poly1FocalLoss on bfloat16 logits themselves (a caller without that cast): the loss and the gradient are those of the widened
    logits, the gradient back in bfloat16, rounded once."""
    from pointstowood_amd.loss import Poly1FocalLoss
    from tests import net_train_ref as NR
    from tests import test_gpu_train_net as TN
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    torch.manual_seed(TN.SEED)
    d = TN._data(NR.inputs(TN.SEED))
    net = TN._net(None, fused=False)
    with torch.autocast("cuda", dtype=BF):
        logits = net(d)
        loss, _ = criterion(logits, d.y)
    assert logits.dtype == torch.float32 and logits.shape == (800,) and loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())

    g = torch.Generator().manual_seed(9)
    x16 = (torch.randn(777, generator=g) * 3).bfloat16().cuda()
    y = (torch.rand(777, generator=g) < 0.3).float().cuda()
    a, b = x16.clone().requires_grad_(), x16.float().requires_grad_()
    la, _ = criterion(a, y)
    lb, _ = criterion(b, y)
    la.backward(), lb.backward()
    assert la.dtype == torch.float32 and _same(la.detach(), lb.detach())
    assert a.grad.dtype == BF and _same(a.grad, b.grad.bfloat16())


# ------------------------------------------------------------------------------------------------ the trainer
_vox = []


def _voxels():
    """The 8 synthetic labelled voxels of 200 - 487 points that the feed's end-to-end test trains on (the recipe of
    tests/test_gpu_train_feed.py's _ten, built here: that module's cache is its own)."""
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


def test_semantic_training_under_bfloat16(tmp_path, capsys):
    """The feed's end-to-end run (8 synthetic labelled voxels, C = 8, batch_size 4, 2 epochs, --test --augmentation) with amp = "bf16":
    a 2 x 11 history of finite values, the skipped count on the epoch line, a final checkpoint that loads into route A with strict=True
    (the parameters stay fp32), and the same history bits from a second run."""
    import pointstowood_amd
    vox = _voxels()
    first = _training_run(str(tmp_path / "a"), vox, amp="bf16")
    printed = capsys.readouterr().out
    assert printed.count("  Skipped ") == 2
    h = np.loadtxt(tmp_path / "a" / "model" / "model_history.csv")
    assert h.shape == (2, 11) and np.isfinite(h).all() and h[:, 0].tolist() == [1.0, 2.0]
    assert (h[:, 1] > 0).all() and (h[:, 2] > 0).all() and ((h[:, 3:] >= 0) & (h[:, 3:] <= 1)).all()
    for path in (tmp_path / "a" / "checkpoints" / "epoch_2.pth", tmp_path / "a" / "model" / "model.pth"):
        ck = torch.load(path, map_location="cpu")
        assert list(ck) == ["model_state_dict"]
        assert all(v.dtype == torch.float32 for v in ck["model_state_dict"].values() if v.is_floating_point())
        missing, unexpected = pointstowood_amd.Net(1, C=8).load_state_dict(ck["model_state_dict"], strict=True)
        assert not missing and not unexpected
    assert _training_run(str(tmp_path / "b"), vox, amp="bf16") == first


def test_semantic_training_without_amp_is_fp16(tmp_path, capsys):
    """amp absent from the namespace gives the history bits that amp = "fp16" gives, and no skipped count is printed; another value is
    refused before anything is built."""
    from pointstowood_amd.trainer import SemanticTraining
    vox = _voxels()
    absent = _training_run(str(tmp_path / "a"), vox)
    assert _training_run(str(tmp_path / "b"), vox, amp="fp16") == absent
    assert "Skipped" not in capsys.readouterr().out
    with pytest.raises(ValueError, match="amp"):
        SemanticTraining(argparse.Namespace(amp="fp8", wandb=False))


def test_a_planted_non_finite_gradient_skips_the_step():
    """trainer.finish_step, the loop's own statements behind backward(): with one inf written into one gradient the bfloat16 mode
    returns 1 (the loop adds it to the skipped count), every parameter and the optimizer's state stay bit-unchanged; the same
    gradients without the inf take the step and return 0."""
    from pointstowood_amd.trainer import finish_step
    torch.manual_seed(1)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 1)).cuda()
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=512, enabled=False)
    x = torch.randn(16, 5, device="cuda")

    def backward():
        optimizer.zero_grad()
        with torch.autocast("cuda", dtype=BF):
            loss = model(x).float().square().mean()
        scaler.scale(loss).backward()

    skipped = 0
    backward()
    skipped += finish_step(model, optimizer, scaler, "bf16")                  # a good step first: AdamW has its moments
    assert skipped == 0
    before = [p.detach().clone() for p in model.parameters()]
    state = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizer.state[p].items()} for p in model.parameters()]
    for planted in (float("inf"), float("nan")):
        backward()
        model[0].weight.grad[3, 2] = planted
        skipped += finish_step(model, optimizer, scaler, "bf16")
        for p, b, st in zip(model.parameters(), before, state):
            assert torch.equal(_ibits(p), _ibits(b))
            assert all(torch.equal(v, st[k]) if torch.is_tensor(v) else v == st[k] for k, v in optimizer.state[p].items())
    assert skipped == 2
    backward()
    assert finish_step(model, optimizer, scaler, "bf16") == 0
    assert all(not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
