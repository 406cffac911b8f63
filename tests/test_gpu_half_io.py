"""The float16 entry points of the training operators (include/p2w.h: p2w_*_io) and ops.half_io on the GPU.

Only the element type at the loads and stores differs from the fp32 entry points, so nothing here has a tolerance: the expected values
are always the EXISTING fp32 entry point fed z16.float() (and g16.float()); its fp32 results are compared bit for bit, and where the
new entry point writes float16 its result is that fp32 result rounded to float16 ON THE CPU (torch.Tensor.half(), pinned in
tests/test_half_io_ref_cpu.py).  A NaN is compared as a NaN, not by payload.  Outputs are pitched, NaN behind every row and one guard
row in the output's own dtype behind the last.  The cases are tests/bn_chain_ref.py's and tests/head_ref.py's."""

import numpy as np
import pytest
import torch

from tests import bn_chain_ref as R
from tests import half_io_ref as HR
from tests import head_ref as HD
from tests import test_gpu_bn_chain as TC
from tests import test_gpu_head as TH
from tests.test_gpu_bn_chain import _pitch

pytestmark = pytest.mark.gpu

EINVAL, ENULL, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4, -5
F32, F16 = 0, 1
NAN = float("nan")
DT = {F32: torch.float32, F16: torch.float16}


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
    """[rows, ld] of NaN in `dtype` that starts `off` elements into its allocation (off = 1: no 4-column access is aligned)."""
    flat = torch.full((rows * ld + off,), NAN, dtype=dtype, device="cuda")
    return flat[off:].view(rows, ld)


def _pitched(t, ld, dtype, off=0):
    buf = _buf(t.shape[0], ld, dtype, off)
    buf[:, :t.shape[1]] = t.to(dtype).cuda()
    return buf


def _half_case(c):
    """The case with z and g rounded to float16 (kept as fp32 tensors of those values: what the fp32 entry point is fed)."""
    return dict(c, z=c["z"].half().float(), g=c["g"].half().float())


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


def _relu_bn_reference(L, c, ld):
    """The fp32 entry points p2w_relu_bn / p2w_relu_bn_bwd on the (one-stage) case: forward and backward dicts."""
    _, ptr, stream = _abi()
    M, C = c["z"].shape
    dev, _ = TC._device_stages(c)
    d = dev[0]
    z, g = _pitched(c["z"], ld, torch.float32), _pitched(c["g"], ld, torch.float32)
    out, dz = _buf(M + 1, ld, torch.float32), _buf(M + 1, ld, torch.float32)
    mean, invstd, dgamma, dbeta = (torch.full((C + 1,), NAN, device="cuda") for _ in range(4))
    need = int(L.p2w_relu_bn_ws_size(M, C))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_relu_bn(ptr(z), ld, ptr(d["gamma"]), ptr(d["beta"]), ptr(d["rm"]), ptr(d["rv"]), R.MOMENTUM, R.BN_EPS, M, C, ptr(out), ld, ptr(mean),
                         ptr(invstd), ptr(ws), need, stream()) == 0
    assert L.p2w_relu_bn_bwd(ptr(g), ld, ptr(z), ld, ptr(d["gamma"]), ptr(mean), ptr(invstd), M, C, ptr(dz), ld, ptr(dgamma), ptr(dbeta), ptr(ws),
                             need, stream()) == 0
    torch.cuda.synchronize()
    fwd = dict(out=out[:M, :C], mean=mean[:C].view(1, C), invstd=invstd[:C].view(1, C), running_mean=d["rm"][:C].view(1, C),
               running_var=d["rv"][:C].view(1, C))
    bwd = dict(dz=dz[:M, :C], dres=None, dgamma=dgamma[:C].view(1, C), dbeta=dbeta[:C].view(1, C))
    return {k: v.cpu() for k, v in fwd.items()}, {k: None if v is None else v.cpu() for k, v in bwd.items()}


_refs = {}


def _chain_reference(L, name, C, M):
    """The fp32 entry points on the float16-valued case, once per case: (case, forward, backward)."""
    if (name, C, M) not in _refs:
        c = _half_case(R.case(name, C, M))
        fwd = TC._forward(L, c, _pitch(C))
        _refs[name, C, M] = (c, fwd, TC._backward(L, c, _pitch(C), fwd))
    return _refs[name, C, M]


def _check_forward(got, ref, to):
    for k in ("mean", "invstd", "running_mean", "running_var"):
        assert _same(got[k], ref[k]), k
    assert _same(got["out"], ref["out"] if to == F32 else ref["out"].half()), "out"


def _check_backward(got, ref, tz):
    for k in ref:
        if k != "dz":
            assert _same(got[k], ref[k]), k
    assert _same(got["dz"], ref["dz"] if tz == F32 else ref["dz"].half()), "dz"


def _widths(C):
    """(pitch, offset) of the 4-column lanes (where C allows them), then the ways to the 1-column lanes: an odd pitch, and a pointer
    one element off."""
    return ([(_pitch(C), 0), (C + 3, 0), (_pitch(C), 1)] if C % 4 == 0 else [(_pitch(C), 0), (_pitch(C), 1)])


CASES = TC.CASES


@pytest.mark.parametrize("name,C,M", CASES)
def test_chain_forward(L, name, C, M):
    """p2w_bn_chain_io on a float16 z, out in fp32 and in float16: mean, invstd, the running statistics and the fp32 out are the fp32
    entry point's bits on z16.float(); the float16 out is its fp32 out rounded on the CPU.  Both access widths (the narrow one forced
    by an odd pitch and by a pointer one element off) and a second call give the same bits; nothing is written behind a row."""
    c, ref, _ = _chain_reference(L, name, C, M)
    for to in (F32, F16):
        for ld, off in _widths(C) + [(_pitch(C), 0)]:
            _check_forward(_chain_forward(L, c, ld, F16, to, off), ref, to)
    _check_forward(_chain_forward(L, c, _pitch(C), F32, F32), ref, F32)             # the codes of the fp32 entry point itself


@pytest.mark.parametrize("name,C,M", CASES)
def test_chain_backward(L, name, C, M):
    """p2w_bn_chain_bwd_io with g in float16 (and in fp32, the chain whose result stayed fp32): dgamma, dbeta, ddw_w, ddw_b (exactly
    0) and dres are the fp32 route's bits, the float16 dz is its dz rounded on the CPU; both widths, and a second call."""
    c, fwd, ref = _chain_reference(L, name, C, M)
    assert bool((ref["ddw_b"] == 0).all())
    for to in (F16, F32):
        for ld, off in _widths(C) + [(_pitch(C), 0)]:
            _check_backward(_chain_backward(L, c, ld, fwd, F16, to, off), ref, F16)
    _check_backward(_chain_backward(L, c, _pitch(C), fwd, F32, F32), ref, F32)


@pytest.mark.parametrize("name,C", [("tail", 16), ("project", 132)])
def test_chain_backward_reaches_subnormals_and_infinities(L, name, C):
    """g scaled by 2^-14 in a third of the columns and by 2^12 in another third (column CONST, whose variance is 0 and whose invstd is
    1 / sqrt(eps), among them): the float16 dz then holds subnormal and infinite elements, at least 100 of each, and still equals the
    fp32 route's dz rounded on the CPU."""
    c = R.case(name, C)
    scale = torch.ones(C)
    scale[torch.arange(C) % 3 == 1], scale[torch.arange(C) % 3 == 2] = 2.0 ** 12, 2.0 ** -14
    c = _half_case(dict(c, g=c["g"] * scale))
    assert bool(torch.isfinite(c["g"]).all())
    fwd = TC._forward(L, c, _pitch(C))
    ref = TC._backward(L, c, _pitch(C), fwd)
    for ld, off in _widths(C):
        got = _chain_backward(L, c, ld, fwd, F16, F16, off)
        _check_backward(got, ref, F16)
    dz = got["dz"].float()
    sub, inf = int(((dz != 0) & (dz.abs() < 2.0 ** -14)).sum()), int(torch.isinf(dz).sum())
    print(f"HALFIO dz {name} C={C}: {sub} subnormal, {inf} infinite of {dz.numel()}")
    assert sub >= 100 and inf >= 100


@pytest.mark.parametrize("C", R.WIDTHS)
def test_the_store_rounds_the_whole_table(L, C):
    """One stage, no ReLU, gamma = 0 in every column: out[:, c] == beta[c] exactly, and beta carries tests/half_io_ref.py's table, C
    values per call - every tie, overflow, subnormal, zero, infinity and the NaN goes through the kernels' one store helper, at both
    access widths.  The float16 out is held to the fp32 entry point's out rounded on the CPU and to the table's own bits."""
    M = 70
    table = torch.from_numpy(HR.TABLE32.copy())
    want16 = torch.from_numpy(HR.TABLE16.view(np.int16).copy())
    base = R.case("one", C, M)
    for lo in range(0, len(table), C):
        idx = (torch.arange(C) + lo) % len(table)
        st = dict(base["stages"][0], a=None, b=None, gamma=torch.zeros(C), beta=table[idx].clone(), relu=False)
        z = base["z"].clone()
        z[:, R.CONST] = torch.linspace(-1, 1, M)
        c = _half_case(dict(base, z=z, stages=[st], res=None))
        ref = TC._forward(L, c, _pitch(C))
        live = ~torch.isnan(st["beta"])
        assert bool((ref["out"][:, live] == st["beta"][live]).all()) and bool(torch.isnan(ref["out"][:, ~live]).all())
        for ld, off in _widths(C):
            _check_forward(_chain_forward(L, c, ld, F16, F32, off), ref, F32)
            got = _chain_forward(L, c, ld, F16, F16, off)
            _check_forward(got, ref, F16)
            pin = live & (st["beta"] != 0)                                         # (a zero's sign is xhat's: it is in the comparison above)
            assert torch.equal(_ibits(got["out"])[:, pin], want16[idx][pin].expand(M, -1)), lo
            assert bool(torch.isnan(got["out"][:, ~live]).all())


def _relu_bn_case(C, M):
    """bn_chain_ref's one-stage case without the depthwise convolution, column ALL_NEG of z all negative (relu(z) is constant 0 there)."""
    c = R.case("one", C, M)
    z = c["z"].clone()
    z[:, R.ALL_NEG] = -z[:, R.ALL_NEG].abs() - 0.125
    return _half_case(dict(c, z=z, stages=[dict(c["stages"][0], a=None, b=None, relu=False)], res=None))


@pytest.mark.parametrize("C,M", [(C, R.M_ROWS) for C in R.WIDTHS] + [(6, 2), (16, 2)])
def test_relu_bn(L, C, M):
    """p2w_relu_bn_io / p2w_relu_bn_bwd_io (the PRE instantiations) as the two chain tests, against p2w_relu_bn / p2w_relu_bn_bwd; the
    all-negative column has mean 0, invstd 1 / sqrt(eps) and dz exactly 0."""
    c = _relu_bn_case(C, M)
    fwd, bwd = _relu_bn_reference(L, c, _pitch(C))
    assert float(fwd["mean"][0, R.ALL_NEG]) == 0.0 and bool((bwd["dz"][:, R.ALL_NEG] == 0).all()) and float(bwd["dz"].abs().max()) > 0
    for to in (F32, F16):
        for ld, off in _widths(C) + [(_pitch(C), 0)]:
            _check_forward(_chain_forward(L, c, ld, F16, to, off, pre=True), fwd, to)
            _check_backward(_chain_backward(L, c, ld, fwd, F16, to, off, pre=True), bwd, F16)
    _check_forward(_chain_forward(L, c, _pitch(C), F32, F32, pre=True), fwd, F32)
    _check_backward(_chain_backward(L, c, _pitch(C), fwd, F32, F32, pre=True), bwd, F32)


# ------------------------------------------------------------------------------------------------ the head
def _head_run(L, c, ld, tz, off=0):
    _, ptr, stream = _abi()
    M, C = c["z"].shape
    z = _pitched(c["z"], ld, DT[tz], off)
    gamma, beta, w, bias, g = (c[k].cuda() for k in ("gamma", "beta", "w", "bias", "g"))
    rm, rv = (torch.cat([c[k], torch.full((1,), NAN)]).cuda() for k in ("rm", "rv"))
    dz = _buf(M + 1, ld, DT[tz], off)
    mean, invstd, dgamma, dbeta, dw = (torch.full((C + 1,), NAN, device="cuda") for _ in range(5))
    dbias, logit = torch.full((2,), NAN, device="cuda"), torch.full((M + 1,), NAN, device="cuda")
    need = int(L.p2w_bn_relu_rowdot_ws_size(M, C))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_bn_relu_rowdot_io(ptr(z), tz, ld, ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(rm), ptr(rv), HD.MOMENTUM, HD.BN_EPS, M, C,
                                   ptr(logit), ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
    assert L.p2w_bn_relu_rowdot_bwd_io(ptr(g), ptr(z), tz, ld, ptr(gamma), ptr(beta), ptr(w), ptr(mean), ptr(invstd), M, C, ptr(dz), ld,
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
    """p2w_bn_relu_rowdot_io / _bwd_io on a float16 z (C = 512: two 256-column passes of the row sums): the logits, mean, invstd, the
    running statistics, dgamma, dbeta, dw and dbias are p2w_bn_relu_rowdot / _bwd's bits on z16.float(); the float16 dz is their dz
    rounded on the CPU; both access widths."""
    c = HD.case(M, C)
    c = dict(c, z=c["z"].half().float())
    ref = TH._run(L, c, _pitch(C))
    for ld, off in _widths(C):
        got = _head_run(L, c, ld, F16, off)
        for k in ref:
            assert _same(got[k], ref[k].half() if k == "dz" else ref[k]), (k, ld, off)
    got = _head_run(L, c, _pitch(C), F32)
    for k in ref:
        assert _same(got[k], ref[k]), k


# ------------------------------------------------------------------------------------------------ the segment max
N_SEG = 4133


def _segments(many):
    """Segment lengths 0, 1, 2, 31, 32, 33 and 2000, then the other 2034 rows as two segments (the few-segment route: values by
    integer atomics, winners in a second pass) or as segments of 8 rows (the one-block-per-segment route)."""
    lens = [0, 1, 2, 31, 32, 33, 2000]
    rest = N_SEG - sum(lens)
    lens += ([8] * (rest // 8) + [rest % 8]) if many else [1000, rest - 1000]
    ptr = torch.tensor([0] + lens).cumsum(0).to(torch.int32)
    assert int(ptr[-1]) == N_SEG
    return ptr


def _segmax_case(F, many):
    g = torch.Generator().manual_seed(100 * F + many)
    ptr = _segments(many)
    x = torch.randn(N_SEG, F, generator=g).half()
    s = [int(v) for v in ptr]
    big = 6                                                # the segment of 2000 rows
    x[s[big] + 5, 0] = x[s[big] + 1500, 0] = 9.0           # a planted tie: the lowest row wins
    x[s[big] + 7, 1], x[s[big] + 8, 2] = float("inf"), float("-inf")
    x[s[big]:s[big + 1], 3] = 0.0
    x[s[big] + 3, 3], x[s[big] + 4, 3] = -0.0, 0.0         # -0 against +0
    x[s[big] + 9, 4] = NAN                                 # a NaN among numbers
    x[s[4]:s[5], 5] = NAN                                  # a segment's column of NaNs only
    x[s[3]:s[4], 2] = float("-inf")                        # ... and one of -inf only
    x[s[5] + 2, 0] = x[s[5] + 30, 0] = 7.5
    return ptr, x, torch.randn(len(s) - 1, F, generator=g)


def _segmax_run(L, ptr_, x, gout, tx, ld, off=0):
    from pointstowood_amd._lib import ptr, stream
    (n, F), B = x.shape, ptr_.numel() - 1
    xp = _pitched(x, ld, DT[tx], off)
    csr, go = ptr_.cuda(), _pitched(gout, F + 4, torch.float32)
    out, arg = torch.full((B * F + 1,), NAN, device="cuda"), torch.full((B * F + 1,), -7, dtype=torch.int32, device="cuda")
    gx = _buf(n + 1, ld, DT[tx], off)
    assert L.p2w_segment_max_arg_io(ptr(xp), tx, ld, F, ptr(csr), B, ptr(out), ptr(arg), stream()) == 0
    assert L.p2w_segment_max_bwd_io(ptr(go), F + 4, ptr(arg), ptr(csr), B, F, ptr(gx), tx, ld, n, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * F])) and int(arg[B * F]) == -7 and bool(torch.isnan(gx[n]).all()) and bool(torch.isnan(gx[:, F:]).all())
    return dict(out=out[:B * F].view(B, F).cpu(), arg=arg[:B * F].view(B, F).cpu(), grad_x=gx[:n, :F].cpu())


def _segmax_reference(L, ptr_, x, gout, ld):
    """The fp32 entry points p2w_segment_max_arg / p2w_segment_max_bwd on x16.float()."""
    from pointstowood_amd._lib import ptr, stream
    (n, F), B = x.shape, ptr_.numel() - 1
    xp, csr, go = _pitched(x.float(), ld, torch.float32), ptr_.cuda(), _pitched(gout, F + 4, torch.float32)
    out, arg = torch.full((B, F), NAN, device="cuda"), torch.full((B, F), -7, dtype=torch.int32, device="cuda")
    gx = _buf(n, ld, torch.float32)
    assert L.p2w_segment_max_arg(ptr(xp), ld, F, ptr(csr), B, ptr(out), ptr(arg), stream()) == 0
    assert L.p2w_segment_max_bwd(ptr(go), F + 4, ptr(arg), ptr(csr), B, F, ptr(gx), ld, n, stream()) == 0
    torch.cuda.synchronize()
    return dict(out=out.cpu(), arg=arg.cpu(), grad_x=gx[:, :F].cpu())


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("F", [6, 16, 132])
def test_segment_max(L, F, many):
    """p2w_segment_max_arg_io / p2w_segment_max_bwd_io on a float16 x, on both routes of the forward: out and arg are the fp32 entry
    point's on x16.float() (NaN handling is whatever that kernel does); grad_x16 is its grad_x rounded on the CPU, exact zeros on every
    losing row; pitched rows, guard rows, both access widths."""
    ptr_, x, gout = _segmax_case(F, many)
    ref = _segmax_reference(L, ptr_, x, gout, _pitch(F))
    B = ptr_.numel() - 1
    assert int(ref["arg"][6, 0]) == int(ptr_[6]) + 5 and int(ref["arg"][4, 5]) == -1 and float(ref["out"][6, 1]) == float("inf")
    assert bool((ref["arg"][0] == -1).all()) and bool((ref["out"][0] == 0).all())                     # the empty segment
    assert int((ref["grad_x"] != 0).sum()) <= B * F and int((ref["grad_x"] != 0).sum()) > B * F // 2
    for ld, off in _widths(F):
        got = _segmax_run(L, ptr_, x, gout, F16, ld, off)
        assert _same(got["out"], ref["out"]) and torch.equal(got["arg"], ref["arg"]), (ld, off)
        assert got["grad_x"].dtype == torch.float16 and _same(got["grad_x"], ref["grad_x"].half()), (ld, off)
        win = torch.zeros(N_SEG, F, dtype=torch.bool)
        rows, cols = ref["arg"].clamp_min(0), torch.arange(F).expand(B, F)
        win[rows[ref["arg"] >= 0], cols[ref["arg"] >= 0]] = True
        assert bool((_ibits(got["grad_x"])[~win] == 0).all())                                         # +0, not -0, not a rounding's leftover
    got = _segmax_run(L, ptr_, x.float(), gout, F32, _pitch(F))
    assert _same(got["out"], ref["out"]) and torch.equal(got["arg"], ref["arg"]) and _same(got["grad_x"], ref["grad_x"])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(L):
    """An unknown dtype code and a float16 out (or g) with an fp32 z: P2W_EUNSUPPORTED from every _io entry point, ahead of every other
    check; then the null, size, alignment and workspace refusals of the fp32 entry points on float16 tensors.  Nothing is launched:
    the NaN-filled outputs stay NaN and the running statistics stay put.  Then the good calls write them."""
    BnStage, ptr, stream = _abi()
    M, C, ld = 14, 8, 12
    z16, g16, out16, dz16 = (torch.full((M, ld), NAN, dtype=torch.float16, device="cuda") for _ in range(4))
    z16[:, :C], g16[:, :C] = torch.randn(M, C).half().cuda(), torch.randn(M, C).half().cuda()
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
    sgo, gx16 = torch.randn(2, ld, device="cuda"), torch.full((M, ld), NAN, dtype=torch.float16, device="cuda")
    s = stream()

    def chain(z=ptr(z16), tz=F16, out=ptr(out16), to=F16, M_=M, ldz=ld, ws_=ptr(ws), wsb=need, mean_=ptr(mean)):
        return L.p2w_bn_chain_io(z, tz, ldz, None, 0, arr, 1, M_, C, out, to, ld, mean_, ptr(invstd), ws_, wsb, s)

    def chain_bwd(g=ptr(g16), to=F16, tz=F16, dz=ptr(dz16), wsb=need, ws_=ptr(ws), lddz=ld):
        return L.p2w_bn_chain_bwd_io(g, to, ld, ptr(z16), tz, ld, None, 0, arr, 1, ptr(mean), ptr(invstd), M, C, dz, lddz, None, 0, ptr(dgamma),
                                     ptr(dbeta), None, None, ws_, wsb, s)

    def relu_bn(tz=F16, to=F16, out=ptr(out16)):
        return L.p2w_relu_bn_io(ptr(z16), tz, ld, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5, M, C, out, to, ld, ptr(mean), ptr(invstd),
                                ptr(ws), need, s)

    def relu_bn_bwd(to=F16, tz=F16, dz=ptr(dz16)):
        return L.p2w_relu_bn_bwd_io(ptr(g16), to, ld, ptr(z16), tz, ld, ptr(gamma), ptr(mean), ptr(invstd), M, C, dz, ld, ptr(dgamma), ptr(dbeta),
                                    ptr(ws), need, s)

    def head(tz=F16, z=ptr(z16), wsb=need):
        return L.p2w_bn_relu_rowdot_io(z, tz, ld, ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(rm), ptr(rv), 0.1, 1e-5, M, C, ptr(logit), ptr(mean),
                                       ptr(invstd), ptr(ws), wsb, s)

    def head_bwd(tz=F16, dz=ptr(dz16), ws_=ptr(ws)):
        return L.p2w_bn_relu_rowdot_bwd_io(ptr(gl), ptr(z16), tz, ld, ptr(gamma), ptr(beta), ptr(w), ptr(mean), ptr(invstd), M, C, dz, ld,
                                           ptr(dgamma), ptr(dbeta), ptr(dw), ptr(dbias), ws_, need, s)

    def seg(tx=F16, x=ptr(z16), ldx=ld):
        return L.p2w_segment_max_arg_io(x, tx, ldx, C, ptr(csr), 2, ptr(sout), ptr(sarg), s)

    def seg_bwd(tx=F16, gx=ptr(gx16)):
        return L.p2w_segment_max_bwd_io(ptr(sgo), ld, ptr(sarg), ptr(csr), 2, C, gx, tx, ld, M, s)

    for code in (2, -1, 7):
        assert chain(tz=code) == EUNSUPPORTED and chain(to=code) == EUNSUPPORTED and chain_bwd(tz=code) == EUNSUPPORTED
        assert chain_bwd(to=code) == EUNSUPPORTED and relu_bn(tz=code) == EUNSUPPORTED and relu_bn(to=code) == EUNSUPPORTED
        assert relu_bn_bwd(tz=code) == EUNSUPPORTED and relu_bn_bwd(to=code) == EUNSUPPORTED and head(tz=code) == EUNSUPPORTED
        assert head_bwd(tz=code) == EUNSUPPORTED and seg(tx=code) == EUNSUPPORTED and seg_bwd(tx=code) == EUNSUPPORTED
    assert chain(tz=F32, to=F16) == EUNSUPPORTED and chain_bwd(tz=F32, to=F16) == EUNSUPPORTED            # a float16 out needs a float16 z
    assert relu_bn(tz=F32, to=F16) == EUNSUPPORTED and relu_bn_bwd(tz=F32, to=F16) == EUNSUPPORTED
    assert chain(tz=2, z=None) == EUNSUPPORTED                                                            # ... ahead of every other check
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


def _operator_route(H, on, run, z16, extra=()):
    """run(z, *extra leaves) -> (out, modules) under autocast with ops.half_io = on; z16 and the extra tensors are cloned leaves.
    Returns the output, every gradient, the BatchNorms' buffers and what was saved."""
    old = H.half_io
    H.half_io = on
    try:
        z = z16.clone().cuda().requires_grad_()
        leaves = [t.clone().cuda().requires_grad_() for t in extra]
        with torch.autocast("cuda", dtype=torch.float16), _Saved() as saved:
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
    """on against off: the same bits everywhere; on saves the caller's float16 z and no fp32 tensor of its shape (but `fp32_saves`:
    the residual chain's out), off saves the fp32 copy."""
    on, kept_on, z_on = _operator_route(H, True, run, z16, extra)
    off, kept_off, _ = _operator_route(H, False, run, z16, extra)
    assert set(on) == set(off)
    for k in on:
        assert _same(on[k], off[k]), k
    assert on["out"].dtype == out_dtype and on["dz"].dtype == torch.float16 and float(on["dz"].float().abs().nan_to_num().max()) > 0
    big = tuple(z16.shape)
    assert sum(1 for dt, shape, _ in kept_on if dt == torch.float32 and shape == big) == fp32_saves, kept_on
    assert sum(1 for dt, shape, _ in kept_off if dt == torch.float32 and shape == big) == fp32_saves + 1, kept_off
    return on, kept_on, z_on


def _chain_modules(c):
    return [(bn, relu, dw) if dw is not None else (bn, relu) for bn, relu, dw in TC._modules(c)]


@pytest.mark.parametrize("name,half_out", [("one", False), ("one", True), ("expand", True), ("tail", False), ("middle", True), ("middle", False),
                                           ("project", False), ("two_res", False), ("three_res", False)])
def test_operator_bn_chain(H, name, half_out):
    """ops.bn_chain under autocast on a float16 z, L = 1, 2, 3, with and without a residual, out_dtype None and float16: half_io on
    against off on cloned inputs and modules - the output, every gradient, the running statistics and num_batches_tracked bit for bit.
    On: z's own storage is what is saved, and no fp32 [M, C] tensor but the residual chain's out; off: the fp32 copy is there."""
    c = R.case(name, 16)
    has_res = c["res"] is not None

    def run(z, *res):
        mods = _chain_modules(c)
        out = H.bn_chain(z, mods, res[0] if res else None, out_dtype=torch.float16 if half_out else None)
        return out, [m for st in mods for m in st if isinstance(m, torch.nn.Module)]

    on, kept, z = _compare_routes(H, run, c["z"].half(), (c["res"],) if has_res else (), torch.float16 if half_out else torch.float32,
                                  fp32_saves=1 if has_res else 0)
    assert (torch.float16, tuple(z.shape), z.data_ptr()) in kept
    assert all(int(v) == 1 for k, v in on.items() if k.endswith("num_batches_tracked"))
    if has_res:
        assert on["leaf0"].dtype == torch.float32
    with pytest.raises(RuntimeError, match="float16"):
        H.bn_chain(c["z"].cuda(), _chain_modules(c), out_dtype=torch.float16)


def test_operator_relu_bn(H):
    c = _relu_bn_case(16, R.M_ROWS)
    for half_out in (False, True):
        def run(z):
            bn = TC._modules(c)[0][0]
            return H.relu_bn(z, bn, out_dtype=torch.float16 if half_out else None), [bn]
        _, kept, z = _compare_routes(H, run, c["z"].half(), out_dtype=torch.float16 if half_out else torch.float32)
        assert (torch.float16, tuple(z.shape), z.data_ptr()) in kept


def test_operator_bn_relu_rowdot(H):
    c = HD.case(257, 16)

    def run(z):
        bn = torch.nn.BatchNorm1d(16, eps=HD.BN_EPS, momentum=HD.MOMENTUM).cuda().train()
        conv = torch.nn.Conv1d(16, 1, 1).cuda()
        with torch.no_grad():
            bn.weight.copy_(c["gamma"]), bn.bias.copy_(c["beta"]), bn.running_mean.copy_(c["rm"]), bn.running_var.copy_(c["rv"])
            conv.weight.copy_(c["w"].view(1, 16, 1)), conv.bias.copy_(c["bias"])
        return H.bn_relu_rowdot(z, bn, conv.weight, conv.bias), [bn, conv]

    _, kept, z = _compare_routes(H, run, c["z"].half())
    assert (torch.float16, tuple(z.shape), z.data_ptr()) in kept


@pytest.mark.parametrize("many", [False, True])
def test_operator_scatter_max(H, many):
    """ops.scatter_max fed a float16 tensor under autocast (what PointNetConv's local_nn hands it), on both routes of the forward: on
    against off bit for bit; the output is fp32, the gradient float16.  Neither route saves x (only the winners), and off also
    hands back a float16 gradient, so what shows that on took the float16 kernels is the peak memory of a forward and backward:
    off allocates an fp32 copy of x [n, F] in the forward and an fp32 grad_x [n, F] next to its float16 rounding in the backward,
    on allocates neither and everything else is the same on both routes, so whichever phase holds the peak, off's is 4 n F bytes
    above on's (less the caching allocator's rounding of a block to 512 bytes, once per route)."""
    ptr_, x, _ = _segmax_case(16, many)
    nb = ptr_.numel() - 1
    index = torch.repeat_interleave(torch.arange(nb), (ptr_[1:] - ptr_[:-1]).long()).cuda()

    def run(z):
        return H.scatter_max(z, index, dim=0, dim_size=nb)[0], []

    on, kept_on, _ = _operator_route(H, True, run, x)
    off, kept_off, _ = _operator_route(H, False, run, x)
    for k in on:
        assert _same(on[k], off[k]), k
    assert on["out"].dtype == torch.float32 and on["dz"].dtype == torch.float16
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
            with torch.autocast("cuda", dtype=torch.float16):
                out = run(z)[0]
            out.backward(cot)
            torch.cuda.synchronize()
            peak[route] = torch.cuda.max_memory_allocated() - base
            del out, z
        finally:
            H.half_io = old
    print(f"HALFIO_SCATTER_PEAK on {peak[True]} off {peak[False]} fp32 x {4 * x.numel()}")
    assert peak[False] - peak[True] >= 4 * x.numel() - 2 * 512


# ------------------------------------------------------------------------------------------------ the whole network
def test_net_training_step_is_the_same_with_the_switch_on_and_off(H):
    """tests/test_gpu_train_net.py's training step (Net(1, 8) on voxels of 600 and 200 points, the injected samples, autocast,
    Poly1FocalLoss, GradScaler(512), unscale_, clip_grad_norm_, AdamW) with ops.half_io off and on: the logits, the loss, every
    gradient, every running statistic and every parameter after the step bit for bit; on a second time gives the same bits again.
    The peak memory of either step is printed, not judged, at this size."""
    from tests.test_gpu_train_net import _train_step
    runs, peaks = [], []
    for on in (False, True, True):
        old = H.half_io
        H.half_io = on
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            net, logits, loss, grads, _ = _train_step()
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated() - base)
        finally:
            H.half_io = old
        runs.append(dict(logits=logits, loss=loss, **{"grad." + k: v for k, v in grads.items()},
                         **{"state." + k: v.detach().clone() for k, v in net.state_dict().items()}))
        del net
    print(f"HALFIO_PEAK on {peaks[1]} off {peaks[0]}")
    off, on, again = runs
    assert set(off) == set(on) and len([k for k in on if k.startswith("grad.")]) == 158
    for k in off:
        assert _same(on[k], off[k]), k
        assert _same(on[k], again[k]), k
    assert bool(torch.isfinite(on["logits"]).all()) and bool(torch.isfinite(on["loss"]))
