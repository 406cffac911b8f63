"""The training route of the feature-propagation module on the GPU: p2w_interp_add_relu / _bwd (csrc/p2w_fp.hip) and p2w_relu_bn / _bwd
(csrc/p2w_bnchain.hip) through the C ABI, each held EXACTLY to a composition of entry points that are already tested against float64
(p2w_interp_concat + one torch add, p2w_interp_bwd, p2w_bn_chain on relu(z)); ops.interp_add_relu and ops.relu_bn under autograd
against those compositions; ops.FPModule against the float64 composition of tests/fp_ref.py.

"Equal" is equal values and equal NaN positions (_same), not equal bit patterns: an underflowing quotient can give -0, and
torch.relu's treatment of -0 is not pinned."""
import copy

import pytest
import torch

from tests import bn_chain_ref as BR
from tests import fp_ref as R
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


def _same(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ family 1 through the ABI
_kcases = {}


def _kcase(m, n_c, C, kw, long_runs=False):
    """Pc [n_c, C], S [m, C], g [m, C], positions, nbr [m, kw] and deg [m] given directly (unused slots hold -1).  Planted where m
    allows: row 0 has deg 0, row 1 deg 1, the last row a deg above kw (clamped), row 2 % m coincides with its first neighbour
    (d2 = 0), rows 3 % m and m // 2 of S are far below 0 (the whole row of H is 0), one NaN in Pc and one in S."""
    key = (m, n_c, C, kw, long_runs)
    if key not in _kcases:
        gen = torch.Generator().manual_seed(1000 * m + 100 * n_c + 10 * C + kw)
        pc, pf = torch.rand(n_c, 4, generator=gen), torch.rand(m, 4, generator=gen)
        nbr = torch.randint(0, n_c, (m, kw), generator=gen, dtype=torch.int32)
        deg = 1 + torch.randint(0, kw, (m,), generator=gen, dtype=torch.int32)
        Pc, S, g = torch.randn(n_c, C, generator=gen), torch.randn(m, C, generator=gen), torch.randn(m, C, generator=gen)
        if long_runs:
            deg[:] = 1
        else:
            if m > 2:
                deg[0], deg[1] = 0, 1
            deg[m - 1] = kw + 2
            S[3 % m], S[m // 2] = -100.0, -50.0
            Pc[n_c - 1, C // 2] = NAN
            S[m - 1, 1] = NAN
            q = 2 % m
            if int(deg[q]) > 0:
                pf[q, :3] = pc[int(nbr[q, 0]), :3]
        nbr[torch.arange(kw)[None, :] >= deg[:, None]] = -1
        _kcases[key] = {k: v.cuda() for k, v in dict(pc=pc, pf=pf, nbr=nbr, deg=deg, Pc=Pc, S=S, g=g).items()}
    return _kcases[key]


def _want_forward(L, c, kw):
    """where(h < 0, 0, h), h = p2w_interp_concat(Pc) + S: the merged entry point and one torch fp32 add."""
    _, ptr, stream = _abi()
    (m, C) = c["S"].shape
    t = torch.empty((m, C), device="cuda")
    assert L.p2w_interp_concat(ptr(c["Pc"]), C, ptr(c["pc"]), ptr(c["pf"]), ptr(c["nbr"]), ptr(c["deg"]), kw, None, 0, m, ptr(t), C, stream()) == 0
    h = t + c["S"]
    return torch.where(h < 0, torch.zeros_like(h), h)


def _fp_forward(L, c, kw, pitched=True):
    _, ptr, stream = _abi()
    (m, C), n_c = c["S"].shape, c["Pc"].shape[0]
    ldp, lds, ldh = (C + 8, C + 4, C + 12) if pitched else (C, C, C)
    Pc, S = _pitched(c["Pc"], ldp), _pitched(c["S"], lds)
    Hh = torch.full((m + 1, ldh), NAN, device="cuda")
    assert L.p2w_interp_add_relu(ptr(Pc), ldp, ptr(S), lds, ptr(c["pc"]), ptr(c["pf"]), ptr(c["nbr"]), ptr(c["deg"]), kw, m, n_c, C, ptr(Hh), ldh,
                                 stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(Hh[m]).all()) and bool(torch.isnan(Hh[:, C:]).all())
    assert bool(torch.isnan(Pc[:, C:]).all()) and bool(torch.isnan(S[:, C:]).all())
    return Hh[:m, :C].contiguous()


def _fp_backward(L, c, kw, Hd, pitched=True):
    _, ptr, stream = _abi()
    (m, C), n_c = c["S"].shape, c["Pc"].shape[0]
    ldg, ldh, ldds, lddp = (C + 4, C + 12, C + 8, C + 4) if pitched else (C, C, C, C)
    g, Hp = _pitched(c["g"], ldg), _pitched(Hd, ldh)
    dS, dPc = torch.full((m + 1, ldds), NAN, device="cuda"), torch.full((n_c + 1, lddp), NAN, device="cuda")
    need = int(L.p2w_interp_add_relu_bwd_ws_size(m, kw, n_c))
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_interp_add_relu_bwd(ptr(g), ldg, ptr(Hp), ldh, ptr(c["pc"]), ptr(c["pf"]), ptr(c["nbr"]), ptr(c["deg"]), kw, m, n_c, C, ptr(dS), ldds,
                                     ptr(dPc), lddp, ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    for t, rows in ((dS, m), (dPc, n_c)):
        assert bool(torch.isnan(t[rows]).all()) and bool(torch.isnan(t[:, C:]).all())
    return dS[:m, :C].contiguous(), dPc[:n_c, :C].contiguous()


def _want_backward(L, c, kw, Hd):
    _, ptr, stream = _abi()
    (m, C), n_c = c["S"].shape, c["Pc"].shape[0]
    dS = torch.where(Hd > 0, c["g"], torch.zeros_like(c["g"]))
    dPc = torch.full((n_c, C), NAN, device="cuda")
    need = int(L.p2w_interp_bwd_ws_bytes(m, kw, n_c))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_interp_bwd(ptr(dS), C, C, ptr(c["pc"]), ptr(c["pf"]), ptr(c["nbr"]), ptr(c["deg"]), kw, m, n_c, ptr(dPc), C, ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    return dS, dPc


SIZES = [(m, n_c) for m in (1, 63, 257) for n_c in (1, 5, 130)]


@pytest.mark.parametrize("C", [4, 68, 132, 520])
@pytest.mark.parametrize("kw", [1, 2, 3, 5])
def test_interp_add_relu_forward_equals_interp_concat_plus_add(L, C, kw):
    """p2w_interp_add_relu on pitched tensors (NaN padding, one guard row behind H) against where(h < 0, 0, h) with
    h = p2w_interp_concat(Pc) + S, for m in {1, 63, 257} x n_c in {1, 5, 130}: kw = 5 leaves the four register-held neighbours, C = 520
    takes the two-chunk loop and its tail, m = 257 needs 65 blocks with three idle waves in the last.  Rows with deg 0, deg 1 and a deg
    above kw, a coincident point, whole rows below zero, a NaN in Pc and one in S (_kcase).  Padding and guard rows stay NaN; dense
    rows give the same values."""
    for m, n_c in SIZES:
        c = _kcase(m, n_c, C, kw)
        want = _want_forward(L, c, kw)
        got = _fp_forward(L, c, kw)
        assert _same(got, want), (m, n_c)
        assert _same(_fp_forward(L, c, kw, pitched=False), want), (m, n_c)
        assert bool((torch.nan_to_num(got[3 % m], nan=0.0) == 0).all()) and bool(torch.isnan(got[m - 1, 1]))
        if m > 2:
            assert _same(got[0], torch.where(c["S"][0] < 0, torch.zeros_like(c["S"][0]), c["S"][0]))      # deg 0: t = 0


@pytest.mark.parametrize("C", [4, 68, 132, 520])
@pytest.mark.parametrize("kw", [1, 2, 3, 5])
def test_interp_add_relu_backward_equals_mask_plus_interp_bwd(L, C, kw):
    """p2w_interp_add_relu_bwd on the forward's own H: dS = where(H > 0, g, 0) and dPc = p2w_interp_bwd of that dS, for the shapes of
    the forward test; coarse rows nobody references (n_c = 130 against m = 1 and 63 leaves some) get zeros, the rows behind the last
    and the padding stay NaN, and a second call with dense rows gives the same bits."""
    for m, n_c in SIZES:
        c = _kcase(m, n_c, C, kw)
        Hd = _fp_forward(L, c, kw, pitched=False)
        want_dS, want_dPc = _want_backward(L, c, kw, Hd)
        dS, dPc = _fp_backward(L, c, kw, Hd)
        assert _same(dS, want_dS) and _same(dPc, want_dPc), (m, n_c)
        used = torch.zeros(n_c, dtype=torch.bool, device="cuda")
        valid = c["nbr"][c["nbr"] >= 0].long()
        used[valid] = True
        if n_c == 130 and m <= 63:
            assert int((~used).sum()) > 0
        assert bool((dPc[~used] == 0).all())
        dS2, dPc2 = _fp_backward(L, c, kw, Hd, pitched=False)
        assert torch.equal(_bits(dS), _bits(dS2)) and torch.equal(_bits(dPc), _bits(dPc2)), (m, n_c)


@pytest.mark.parametrize("n_c,unreferenced", [(2, None), (3, 1)])
def test_interp_add_relu_backward_long_runs(L, n_c, unreferenced):
    """The fp4 regime: m = 700 fine rows of one neighbour over 2 (3) coarse rows with kw = 2, a mean run of 700 slots - the run sums are
    split over blocks and combined.  Equal to p2w_interp_bwd of the masked gradient; with n_c = 3 coarse row 1 is referenced by nobody
    and gets zeros.  Two calls give the same bits."""
    m, C, kw = 700, 132, 2
    c = dict(_kcase(m, n_c, C, kw, long_runs=True))
    if unreferenced is not None:
        nbr = c["nbr"].clone()
        nbr[nbr == unreferenced] = 0
        c["nbr"] = nbr
    Hd = _fp_forward(L, c, kw)
    assert _same(Hd, _want_forward(L, c, kw)) and float(Hd.max()) > 0
    want_dS, want_dPc = _want_backward(L, c, kw, Hd)
    dS, dPc = _fp_backward(L, c, kw, Hd)
    assert _same(dS, want_dS) and _same(dPc, want_dPc)
    assert float(dPc[0].abs().max()) > 0
    if unreferenced is not None:
        assert bool((dPc[unreferenced] == 0).all())
    dS2, dPc2 = _fp_backward(L, c, kw, Hd)
    assert torch.equal(_bits(dS), _bits(dS2)) and torch.equal(_bits(dPc), _bits(dPc2))


# ------------------------------------------------------------------------------------------------ family 2 through the ABI
ALL_NEG, GAMMA_ZERO, GAMMA_NEG, NAN_COL = 0, 1, 2, 3


def _bcase(M, C, nan=True):
    """z, g [M, C], gamma, beta, running statistics.  With C >= 4: column 0 of z is all negative (relu(z) is constant 0: zero
    variance), gamma = 0 in column 1, gamma < 0 in column 2 and, with `nan`, one NaN in column 3 of z."""
    gen = torch.Generator().manual_seed(100 * M + C)
    z, g = torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen)
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    rm, rv = 0.1 * torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    if C >= 4:
        z[:, ALL_NEG] = -z[:, ALL_NEG].abs() - 0.01
        gamma[GAMMA_ZERO], gamma[GAMMA_NEG] = 0.0, -0.8
        if nan:
            z[M // 2, NAN_COL] = NAN
    return dict(z=z, g=g, gamma=gamma, beta=beta, rm=rm, rv=rv)


def _relu_bn_run(L, c, ld, chain):
    """Forward and backward through the ABI with every [M, C] tensor pitched to ld: p2w_relu_bn / _bwd on z, or (chain) p2w_bn_chain /
    _bwd with one plain stage on a materialised relu(z), its dz masked by z > 0 afterwards.  One guard row or element of NaN behind
    every output."""
    BnStage, ptr, stream = _abi()
    (M, C) = c["z"].shape
    zin = torch.relu(c["z"].cuda()) if chain else c["z"].cuda()
    z, g = _pitched(zin, ld), _pitched(c["g"], ld)
    gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
    rm, rv = (torch.cat([c[k], torch.full((1,), NAN)]).cuda() for k in ("rm", "rv"))
    out, dz = (torch.full((M + 1, ld), NAN, device="cuda") for _ in range(2))
    mean, invstd, dgamma, dbeta = (torch.full((C + 1,), NAN, device="cuda") for _ in range(4))
    need = int(L.p2w_bn_chain_ws_size(M, C, 1)) if chain else int(L.p2w_relu_bn_ws_size(M, C))
    assert need > 0 and need % 256 == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if chain:
        arr = (BnStage * 1)()
        arr[0] = BnStage(None, None, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), BR.MOMENTUM, BR.BN_EPS, 0)
        assert L.p2w_bn_chain(ptr(z), ld, None, 0, arr, 1, M, C, ptr(out), ld, ptr(mean), ptr(invstd), ptr(ws), need, stream()) == 0
        assert L.p2w_bn_chain_bwd(ptr(g), ld, ptr(z), ld, None, 0, arr, 1, ptr(mean), ptr(invstd), M, C, ptr(dz), ld, None, 0, ptr(dgamma),
                                  ptr(dbeta), None, None, ptr(ws), need, stream()) == 0
    else:
        assert L.p2w_relu_bn(ptr(z), ld, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), BR.MOMENTUM, BR.BN_EPS, M, C, ptr(out), ld, ptr(mean),
                             ptr(invstd), ptr(ws), need, stream()) == 0
        assert L.p2w_relu_bn_bwd(ptr(g), ld, ptr(z), ld, ptr(gamma), ptr(mean), ptr(invstd), M, C, ptr(dz), ld, ptr(dgamma), ptr(dbeta),
                                 ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    for t in (out, dz):
        assert bool(torch.isnan(t[M]).all()) and bool(torch.isnan(t[:, C:]).all())
    for t in (mean, invstd, dgamma, dbeta, rm, rv):
        assert bool(torch.isnan(t[C]))
    r = dict(out=out[:M, :C], dz=dz[:M, :C], mean=mean[:C], invstd=invstd[:C], dgamma=dgamma[:C], dbeta=dbeta[:C], running_mean=rm[:C],
             running_var=rv[:C])
    if chain:
        r["dz"] = torch.where(c["z"].cuda() > 0, r["dz"], torch.zeros_like(r["dz"]))
    return {k: v.contiguous().cpu() for k, v in r.items()}


@pytest.mark.parametrize("C", [1, 4, 67, 132])
@pytest.mark.parametrize("M", [2, 31, 33, 257])
def test_relu_bn_equals_the_chain_on_relu_z(L, M, C):
    """p2w_relu_bn / p2w_relu_bn_bwd against p2w_bn_chain / p2w_bn_chain_bwd (L = 1, no depthwise, relu = 0) on a materialised relu(z):
    out, mean, invstd, the running statistics, dgamma, dbeta, and dz = the chain's masked by z > 0.  M = 31 / 33 / 257 are one partial,
    two and nine work items; widths that are multiples of 4 run with 16-byte lanes (pitch C + 8) and with 4-byte lanes (pitch C + 3),
    the others with 4-byte lanes.  An all-negative column, gamma = 0, gamma < 0 and a NaN column (C >= 4)."""
    c = _bcase(M, C)
    first = None
    for ld in ([C + 8, C + 3] if C % 4 == 0 else [C + 3]):
        got, want = _relu_bn_run(L, c, ld, chain=False), _relu_bn_run(L, c, ld, chain=True)
        for k in want:
            assert _same(got[k], want[k]), (k, ld)
        if first is None:
            first = got
        for k in got:                                                            # the two access widths: the same bits in every number
            ok = ~torch.isnan(first[k])                                          # (a NaN's sign and payload are not pinned)
            assert _same(got[k], first[k]) and torch.equal(_bits(got[k])[ok], _bits(first[k])[ok]), (k, ld)
    if C >= 4:
        assert bool((first["dz"][:, ALL_NEG] == 0).all()) and float(first["mean"][ALL_NEG]) == 0.0
        assert bool((first["dz"][:, GAMMA_ZERO] == 0).all())
        assert bool(torch.isnan(first["out"][:, NAN_COL]).all()) and bool(torch.isfinite(first["out"][:, [0, 1, 2]]).all())
    assert bool((first["dz"][c["z"] <= 0] == 0).all())


def test_relu_bn_against_fp64_chain():
    """One case (M = 257, C = 132, finite) against tests/bn_chain_ref.py's float64 one-stage chain on relu(z), within that file's own
    derived caps: mean, invstd, running statistics, out; dgamma, dbeta and dz, reference and cap masked by z > 0."""
    from pointstowood_amd._lib import lib
    c = _bcase(257, 132, nan=False)
    got = _relu_bn_run(lib(), c, 132 + 8, chain=False)
    u = torch.relu(c["z"])
    st = [dict(a=None, b=None, gamma=c["gamma"], beta=c["beta"], running_mean=c["rm"], running_var=c["rv"], relu=False)]
    mean, invstd = got["mean"][None], got["invstd"][None]
    ref, caps = BR.forward_reference(u, st, None, mean, invstd)
    ratios = {k: BR.ratio(got[k].reshape(ref[k].shape), ref[k], caps[k]) for k in ("mean", "invstd", "running_mean", "running_var", "out")}
    bref, bcaps = BR.backward_reference(c["g"], u, st, None, mean, invstd)
    mask = c["z"] > 0
    ratios["dz"] = BR.ratio(got["dz"], torch.where(mask, bref["dz"], torch.zeros_like(bref["dz"])), bcaps["dz"])
    for k in ("dgamma", "dbeta"):
        ratios[k] = BR.ratio(got[k].reshape(bref[k].shape), bref[k], bcaps[k])
    print("FP_RELU_BN_RATIO " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0
    assert float(got["dz"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ ABI guards
def test_interp_add_relu_guards_launch_nothing(L):
    """P2W_ENULL, P2W_EALIGN, P2W_EINVAL (C % 4, a pitch below C or off a multiple of 4, kw = 0 and 101, m < 0) and P2W_EWORKSPACE of both
    entry points come back before anything is launched: the NaN-filled outputs stay NaN.  m = 0 is P2W_OK.  Then the good calls write."""
    _, ptr, stream = _abi()
    m, n_c, C, kw = 9, 4, 8, 2
    c = _kcase(m, n_c, C, kw, long_runs=True)
    Hh, dS = (torch.full((m, C), NAN, device="cuda") for _ in range(2))
    dPc = torch.full((n_c, C), NAN, device="cuda")
    need = int(L.p2w_interp_add_relu_bwd_ws_size(m, kw, n_c))
    assert need > 0 and need % 256 == 0
    assert L.p2w_interp_add_relu_bwd_ws_size(m, 0, n_c) == 0 and L.p2w_interp_add_relu_bwd_ws_size(-1, kw, n_c) == 0
    assert L.p2w_interp_add_relu_bwd_ws_size(m, 101, n_c) == 0 and L.p2w_interp_add_relu_bwd_ws_size(m, kw, -1) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    s = stream()

    def fwd(Pc=ptr(c["Pc"]), ldp=C, S=ptr(c["S"]), lds=C, rc=ptr(c["pc"]), rf=ptr(c["pf"]), nbr=ptr(c["nbr"]), deg=ptr(c["deg"]), kw_=kw, m_=m,
            n_=n_c, C_=C, H_=ptr(Hh), ldh=C):
        return L.p2w_interp_add_relu(Pc, ldp, S, lds, rc, rf, nbr, deg, kw_, m_, n_, C_, H_, ldh, s)

    def bwd(g=ptr(c["g"]), ldg=C, H_=ptr(c["S"]), ldh=C, rc=ptr(c["pc"]), rf=ptr(c["pf"]), nbr=ptr(c["nbr"]), deg=ptr(c["deg"]), kw_=kw, m_=m,
            n_=n_c, C_=C, dS_=ptr(dS), ldds=C, dPc_=ptr(dPc), lddp=C, ws_=ptr(ws), wsb=need):
        return L.p2w_interp_add_relu_bwd(g, ldg, H_, ldh, rc, rf, nbr, deg, kw_, m_, n_, C_, dS_, ldds, dPc_, lddp, ws_, wsb, s)

    for name in ("Pc", "S", "rc", "rf", "nbr", "deg", "H_"):
        assert fwd(**{name: None}) == ENULL, name
    for name in ("g", "H_", "rc", "rf", "nbr", "deg", "dS_", "dPc_", "ws_"):
        assert bwd(**{name: None}) == ENULL, name
    for name in ("Pc", "S", "rc", "rf", "H_"):
        assert fwd(**{name: ptr(c["S"]) + 4}) == EALIGN, name
    for name in ("g", "H_", "dS_", "dPc_", "ws_"):
        assert bwd(**{name: ptr(ws) + 8}) == EALIGN, name
    assert fwd(C_=6) == EINVAL and fwd(C_=0) == EINVAL and fwd(ldp=C - 4) == EINVAL and fwd(lds=C + 2) == EINVAL and fwd(ldh=4) == EINVAL
    assert fwd(kw_=0) == EINVAL and fwd(kw_=101) == EINVAL and fwd(m_=-1) == EINVAL and fwd(n_=-1) == EINVAL
    assert bwd(C_=6) == EINVAL and bwd(ldg=C - 4) == EINVAL and bwd(ldh=C + 1) == EINVAL and bwd(ldds=4) == EINVAL and bwd(lddp=4) == EINVAL
    assert bwd(kw_=0) == EINVAL and bwd(m_=-1) == EINVAL
    assert bwd(wsb=need - 1) == EWORKSPACE and bwd(wsb=0) == EWORKSPACE
    assert fwd(m_=0) == 0
    torch.cuda.synchronize()
    for t in (Hh, dS, dPc):
        assert bool(torch.isnan(t).all())
    assert fwd() == 0
    assert bwd(H_=ptr(Hh)) == 0
    torch.cuda.synchronize()
    for t in (Hh, dS, dPc):
        assert bool(torch.isfinite(t).all())
    assert bool((Hh >= 0).all())


def test_relu_bn_guards_launch_nothing(L):
    """P2W_ENULL, P2W_EALIGN (the workspace), P2W_EINVAL (M = 1, C = 0, a pitch below C, eps < 0, momentum > 1) and P2W_EWORKSPACE of both
    entry points: the NaN-filled outputs stay NaN and the running statistics stay put.  Then the good calls write them."""
    _, ptr, stream = _abi()
    M, C = 14, 8
    z, g = (torch.randn(M, C + 4, device="cuda") for _ in range(2))
    gamma, beta = (torch.rand(C, device="cuda") + 0.5 for _ in range(2))
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    out, dz = (torch.full((M, C + 4), NAN, device="cuda") for _ in range(2))
    mean, invstd, dgamma, dbeta = (torch.full((C,), NAN, device="cuda") for _ in range(4))
    need = int(L.p2w_relu_bn_ws_size(M, C))
    assert need > 0 and need % 256 == 0 and need == int(L.p2w_bn_chain_ws_size(M, C, 1))
    assert L.p2w_relu_bn_ws_size(1, C) == 0 and L.p2w_relu_bn_ws_size(M, 0) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    s = stream()

    def fwd(z_=ptr(z), ldz=C + 4, gamma_=ptr(gamma), beta_=ptr(beta), rm_=ptr(rm), rv_=ptr(rv), mom=0.1, eps=1e-5, M_=M, C_=C, out_=ptr(out),
            ldo=C + 4, mean_=ptr(mean), invstd_=ptr(invstd), ws_=ptr(ws), wsb=need):
        return L.p2w_relu_bn(z_, ldz, gamma_, beta_, rm_, rv_, mom, eps, M_, C_, out_, ldo, mean_, invstd_, ws_, wsb, s)

    def bwd(g_=ptr(g), ldg=C + 4, z_=ptr(z), ldz=C + 4, gamma_=ptr(gamma), mean_=ptr(mean), invstd_=ptr(invstd), M_=M, C_=C, dz_=ptr(dz),
            lddz=C + 4, dgamma_=ptr(dgamma), dbeta_=ptr(dbeta), ws_=ptr(ws), wsb=need):
        return L.p2w_relu_bn_bwd(g_, ldg, z_, ldz, gamma_, mean_, invstd_, M_, C_, dz_, lddz, dgamma_, dbeta_, ws_, wsb, s)

    for name in ("z_", "gamma_", "beta_", "rm_", "rv_", "out_", "mean_", "invstd_", "ws_"):
        assert fwd(**{name: None}) == ENULL, name
    for name in ("g_", "z_", "gamma_", "mean_", "invstd_", "dz_", "dgamma_", "dbeta_", "ws_"):
        assert bwd(**{name: None}) == ENULL, name
    assert fwd(ws_=ptr(ws) + 4) == EALIGN and bwd(ws_=ptr(ws) + 8) == EALIGN
    assert fwd(M_=1) == EINVAL and fwd(C_=0) == EINVAL and fwd(ldz=C - 1) == EINVAL and fwd(ldo=C - 1) == EINVAL
    assert fwd(eps=-1.0) == EINVAL and fwd(mom=1.5) == EINVAL
    assert bwd(M_=1) == EINVAL and bwd(C_=0) == EINVAL and bwd(ldg=C - 1) == EINVAL and bwd(ldz=4) == EINVAL and bwd(lddz=C - 1) == EINVAL
    assert fwd(wsb=need - 1) == EWORKSPACE and fwd(wsb=0) == EWORKSPACE and bwd(wsb=need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    for t in (out, dz, mean, invstd, dgamma, dbeta):
        assert bool(torch.isnan(t).all())
    assert bool((rm == 0).all()) and bool((rv == 1).all())
    assert fwd() == 0
    assert bwd() == 0
    torch.cuda.synchronize()
    for t in (out[:, :C], dz[:, :C], mean, invstd, dgamma, dbeta):
        assert bool(torch.isfinite(t).all())
    assert bool(torch.isnan(out[:, C:]).all()) and bool(torch.isnan(dz[:, C:]).all())
    assert bool((rm != 0).any()) and bool((rv != 1).any()) and bool((dz[:, :C][z[:, :C] <= 0] == 0).all())


# ------------------------------------------------------------------------------------------------ the operators under autograd
def _op_case(C, seed=4):
    gen = torch.Generator().manual_seed(seed)
    coarse, fine = [70, 2, 58], [150, 30, 120]
    c = dict(batch=torch.repeat_interleave(torch.arange(3), torch.tensor(coarse)), batch_skip=torch.repeat_interleave(torch.arange(3), torch.tensor(fine)),
             pos=torch.rand(sum(coarse), 3, generator=gen), pos_skip=torch.rand(sum(fine), 3, generator=gen),
             Pc=torch.randn(sum(coarse), C, generator=gen), S=torch.randn(sum(fine), C, generator=gen), g=torch.randn(sum(fine), C, generator=gen))
    return {k: v.cuda() for k, v in c.items()}


@pytest.mark.parametrize("C", [132, 30])
def test_interp_add_relu_operator_equals_the_composition(H, C):
    """ops.interp_add_relu against torch.relu(ops.knn_interpolate(Pc, ...) + S) under ordinary autograd on three ragged batches (the
    middle one has two coarse points under k = 3): the output, the gradient to Pc and the gradient to S are equal.  C = 30 goes through
    the padding to a multiple of 4."""
    c = _op_case(C)
    r = {}
    for fused in (True, False):
        Pc, S = c["Pc"].clone().requires_grad_(), c["S"].clone().requires_grad_()
        if fused:
            out = H.interp_add_relu(Pc, S, c["pos"], c["pos_skip"], c["batch"], c["batch_skip"], k=3)
        else:
            out = torch.relu(H.knn_interpolate(Pc, c["pos"], c["pos_skip"], c["batch"], c["batch_skip"], k=3) + S)
        (out * c["g"]).sum().backward()
        r[fused] = (out.detach(), Pc.grad, S.grad)
    assert r[True][0].shape == c["S"].shape and r[True][0].dtype == torch.float32
    for a, b in zip(r[True], r[False]):
        assert _same(a, b) and float(a.abs().max()) > 0


def test_interp_add_relu_operator_modes(H):
    """autocast with float16 inputs: an fp32 output, gradients in the inputs' dtypes.  no_grad: the tracked output's bits, no graph."""
    c = _op_case(68)
    Pc, S = c["Pc"].half().requires_grad_(), c["S"].half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = H.interp_add_relu(Pc, S, c["pos"], c["pos_skip"], c["batch"], c["batch_skip"], k=3)
    assert out.dtype == torch.float32
    (out * c["g"]).sum().backward()
    assert Pc.grad.dtype == torch.float16 and S.grad.dtype == torch.float16 and Pc.grad.shape == Pc.shape and S.grad.shape == S.shape
    tracked = H.interp_add_relu(c["Pc"].clone().requires_grad_(), c["S"], c["pos"], c["pos_skip"], c["batch"], c["batch_skip"], k=3)
    assert tracked.grad_fn is not None
    with torch.no_grad():
        plain = H.interp_add_relu(c["Pc"].clone().requires_grad_(), c["S"], c["pos"], c["pos_skip"], c["batch"], c["batch_skip"], k=3)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(_bits(plain), _bits(tracked.detach()))
    with pytest.raises(RuntimeError):
        H.interp_add_relu(c["Pc"], c["S"][:, :8], c["pos"], c["pos_skip"], c["batch"], c["batch_skip"], k=3)


def _bn(c, **kw):
    C = c["z"].shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=BR.BN_EPS, momentum=BR.MOMENTUM, **kw)
    with torch.no_grad():
        if bn.affine:
            bn.weight.copy_(c["gamma"]), bn.bias.copy_(c["beta"])
        if bn.track_running_stats:
            bn.running_mean.copy_(c["rm"]), bn.running_var.copy_(c["rv"])
    return bn.cuda().train()


@pytest.mark.parametrize("M,C", [(257, 132), (33, 67)])
def test_relu_bn_operator_equals_bn_chain_on_relu(H, M, C):
    """ops.relu_bn(z, bn) against ops.bn_chain(torch.relu(z), [(bn, False)]) on cloned modules: the output, dz, dgamma, dbeta, the running
    statistics and num_batches_tracked are equal."""
    c = _bcase(M, C, nan=False)
    r = {}
    for fused in (True, False):
        bn = _bn(c)
        z = c["z"].cuda().requires_grad_()
        out = H.relu_bn(z, bn) if fused else H.bn_chain(torch.relu(z), [(bn, False)])
        (out * c["g"].cuda()).sum().backward()
        r[fused] = dict(out=out.detach(), dz=z.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, rm=bn.running_mean, rv=bn.running_var,
                        n=bn.num_batches_tracked)
    for k in r[True]:
        assert _same(r[True][k].float(), r[False][k].float()), k
    assert int(r[True]["n"]) == 1 and float(r[True]["dz"].abs().max()) > 0


def test_relu_bn_operator_modes_and_errors(H):
    """no_grad: the same bits, no graph, the statistics move.  autocast(float16): fp32 out, dz in z's dtype.  Eval mode: bn(relu(z)) bit
    for bit, the statistics stay put.  affine=False, track_running_stats=False, momentum=None: NotImplementedError; one row: PyTorch's
    ValueError; a wrong width: RuntimeError; not a BatchNorm1d: TypeError."""
    c = _bcase(33, 68, nan=False)
    z = c["z"].cuda()
    a, b = _bn(c), _bn(c)
    tracked = H.relu_bn(z.clone().requires_grad_(), a)
    with torch.no_grad():
        plain = H.relu_bn(z.clone().requires_grad_(), b)
    assert tracked.grad_fn is not None and plain.grad_fn is None and torch.equal(_bits(plain), _bits(tracked.detach()))
    assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
    assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 1 and not torch.equal(a.running_mean.cpu(), c["rm"])
    h, zh = _bn(c), z.half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = H.relu_bn(zh, h)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert zh.grad.dtype == torch.float16 and h.weight.grad.dtype == torch.float32
    e = _bn(c).eval()
    got, want = H.relu_bn(z, e), e(torch.relu(z))
    assert torch.equal(_bits(got.detach()), _bits(want.detach())) and torch.equal(e.running_mean.cpu(), c["rm"]) and int(e.num_batches_tracked) == 0
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        with pytest.raises(NotImplementedError):
            H.relu_bn(z, _bn(c, **kw))
    none = _bn(c)
    none.momentum = None
    with pytest.raises(NotImplementedError):
        H.relu_bn(z, none)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        H.relu_bn(z[:1], _bn(c))
    with pytest.raises(RuntimeError):
        H.relu_bn(z[:, :8], _bn(c))
    with pytest.raises(TypeError):
        H.relu_bn(z, torch.nn.Identity())


# ------------------------------------------------------------------------------------------------ the module
def test_module_has_the_reference_state_dict(H):
    """ops.FPModule(2, [96, 80, 64]): keys, order and shapes against the literal list written from model.py:142-153,198-202 (MLP: Lin +
    ReLU, then Lin + ReLU + BN); a plain MLP-shaped state dict loads."""
    want = [("NN.0.0.weight", [80, 96]), ("NN.0.0.bias", [80]), ("NN.1.0.weight", [64, 80]), ("NN.1.0.bias", [64]), ("NN.1.2.weight", [64]),
            ("NN.1.2.bias", [64]), ("NN.1.2.running_mean", [64]), ("NN.1.2.running_var", [64]), ("NN.1.2.num_batches_tracked", [])]
    mod = H.FPModule(2, [96, 80, 64])
    assert [(k, list(v.shape)) for k, v in mod.state_dict().items()] == want and mod.k == 2 and mod.fused is True
    from torch.nn import BatchNorm1d as BN, Linear as Lin, ReLU, Sequential as Seq
    mlp = Seq(Seq(Lin(96, 80), ReLU()), Seq(Lin(80, 64), ReLU(), BN(64)))
    mod.load_state_dict({"NN." + k: v for k, v in mlp.state_dict().items()})
    assert all(torch.equal(v, mlp.state_dict()[k[3:]]) for k, v in mod.state_dict().items())
    assert len(H.FPModule(3, [8, 8, 8, 8]).state_dict()) == 2 + 7 + 7


def _module(H, c, fused, train=True):
    mod = H.FPModule(c["k"], c["NN"])
    mod.load_state_dict(c["sd"])
    mod = mod.cuda().train(train)
    mod.fused = fused
    return mod


def _gpu_step(H, c, fused, lr=None):
    mod = _module(H, c, fused)
    x, xs = c["x"].cuda().requires_grad_(), c["x_skip"].cuda().requires_grad_()
    out, pos_out, batch_out = mod(x, c["pos"].cuda(), c["batch"].cuda(), xs, c["pos_skip"].cuda(), c["batch_skip"].cuda())
    assert pos_out.shape == c["pos_skip"].shape and torch.equal(batch_out.cpu(), c["batch_skip"])
    (out * c["g"].cuda()).sum().backward()
    r = dict(out=out.detach(), x=x.grad, x_skip=xs.grad, **{k: p.grad for k, p in mod.named_parameters()})
    r.update({k: v.clone() for k, v in mod.state_dict().items() if "running" in k})
    tracked = [int(v) for k, v in mod.state_dict().items() if k.endswith("num_batches_tracked")]
    if lr is not None:
        torch.optim.AdamW(mod.parameters(), lr=lr).step()
        r.update({"step." + k: p.detach().clone() for k, p in mod.named_parameters()})
    return {k: v.cpu() for k, v in r.items()}, tracked


@pytest.mark.parametrize("name", list(R.MODULE_CASES))
def test_module_eval_and_unfused_are_the_plain_composition(H, name):
    """Eval mode, fused = False in training mode and x_skip = None run knn_interpolate, cat, self.NN statement by statement: the same
    bits as those statements written out here on a clone."""
    c = R.module_case(name)
    args = [c[k].cuda() for k in ("x", "pos", "batch", "x_skip", "pos_skip", "batch_skip")]
    for fused, train in ((True, False), (False, False), (False, True)):
        mod, twin = _module(H, c, fused, train), _module(H, c, fused, train)
        got = mod(*args)[0]
        want = twin.NN(torch.cat([H.knn_interpolate(args[0], args[1], args[4], args[2], args[5], k=c["k"]), args[3]], 1))
        assert torch.equal(_bits(got.detach()), _bits(want.detach())), (fused, train)
        assert all(torch.equal(a, b) for a, b in zip(mod.state_dict().values(), twin.state_dict().values()))
    wide = H.FPModule(c["k"], [c["Fc"]] + c["NN"][1:]).cuda().train()
    twin = copy.deepcopy(wide)
    got = wide(args[0], args[1], args[2], None, args[4], args[5])[0]
    want = twin.NN(H.knn_interpolate(args[0], args[1], args[4], args[2], args[5], k=c["k"]))
    assert torch.equal(_bits(got.detach()), _bits(want.detach()))


@pytest.mark.parametrize("name", list(R.MODULE_CASES))
def test_module_trains_like_the_fp64_composition(H, name):
    """One training step and one AdamW step of ops.FPModule, fused and fused = False on cloned modules, both against the float64
    composition of tests/fp_ref.py (oracle knn_interpolate, training-mode F.batch_norm): the output, the gradients to x and x_skip,
    every parameter gradient, the running statistics and every parameter after the optimiser step.  Per tensor the fused route's
    relative L2 error is at most 8 x the plain route's own (the bar of tests/test_gpu_bn_chain.py: fp32 reordering noise measured
    against float64), and the plain route's error is positive.  'ragged': B = 3, 300 coarse and 600 fine points, a batch with two
    coarse points under k = 3; 'fp4': one coarse point per batch at the origin.  test_fp_ref_cpu.py asserts that no pre-activation of
    these cases is close enough to 0 for a ReLU mask to differ.  A second fused step from the same state gives the same bits."""
    c = R.module_case(name)
    ref = R.train_step(c, lr=1e-3)
    fused, tf = _gpu_step(H, c, True, lr=1e-3)
    plain, tp = _gpu_step(H, c, False, lr=1e-3)
    assert tf == tp == [1]
    keys = [k for k in ref if k != "pre"]
    assert set(keys) == set(fused) == set(plain)
    worst = 0.0
    for k in keys:
        ef, ep = _rel_l2(fused[k], ref[k]), _rel_l2(plain[k], ref[k])
        print(f"FP_MODULE {name} {k}: fused {ef:.3e} plain {ep:.3e} ratio {ef / ep if ep > 0 else float('inf'):.3f}")
        assert ep > 0, k
        worst = max(worst, ef / ep)
    print(f"FP_MODULE_WORST {name} {worst:.3f}")
    for k in keys:
        assert _rel_l2(fused[k], ref[k]) <= 8 * _rel_l2(plain[k], ref[k]), k
    again, _ = _gpu_step(H, c, True)
    for k in again:
        assert torch.equal(_bits(again[k]), _bits(fused[k])), k
