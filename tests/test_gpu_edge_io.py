"""Layer 1 of the edge MLP with a float16 / bfloat16 H1 and a recomputed ReLU mask (csrc/p2w_edge.hip: p2w_edge_l1_io /
p2w_edge_l1_bwd_io; ops.edge_layer1(out_dtype=); ops.PointNetConv under autocast with ops.half_io).  The contract is exact, so nothing
here has a tolerance: a 16-bit H1 is the fp32 entry point's H1 rounded once by torch.Tensor.half() / .bfloat16(), the backward gives the
bits of p2w_edge_l1_bwd on the widened gradient and the fp32 H1 - also where the stored H1 is zero and the fp32 one is not
(tests/edge_io_ref.py) -, and half_io on equals half_io off bit for bit up to one whole AdamW step of train.Net."""
import numpy as np
import pytest
import torch

from tests import conv_train_ref as C
from tests import edge_io_ref as R

pytestmark = pytest.mark.gpu

EINVAL, ENULL, EALIGN, EWORKSPACE, EUNSUPPORTED = -1, -2, -3, -4, -5
F32, F16, BF16 = 0, 1, 2
DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
# one lane per row; the 4-byte path; 16 lanes per row; the 4-byte path with two column passes; the 16-byte path with two column passes
WIDTHS = [4, 6, 64, 67, 260]
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
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


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


def _buf(rows, ld, dtype, fill=NAN, off=0):
    """[rows, ld] of `fill` in `dtype` that starts `off` elements into its allocation."""
    flat = torch.full((rows * ld + off,), fill, dtype=dtype, device="cuda")
    return flat[off:].view(rows, ld)


def _pitched(t, ld, dtype=torch.float32, off=0):
    buf = _buf(t.shape[0], ld, dtype, NAN, off)
    buf[:, :t.shape[1]] = t.to(dtype).cuda()
    return buf


def _pitch(C1):
    """A row pitch larger than C1 that keeps the access width of C1."""
    return C1 + 8 if C1 % 4 == 0 else C1 + 3


# ------------------------------------------------------------------------------------------------ the cases and their fp32 results
BAD_EDGES = (7, 1234, 3000)              # edges whose source is outside [0, n_src): in a short target, in the 1500-edge one, past it


def _edge_case():
    """conv_train_ref.edge_case() (degrees 0, 1, 32, 33, 100 and 1500; about six 1 024-edge chunks) with three sources outside
    [0, n_src) planted: n_src, -1 and a large one."""
    c = dict(C.edge_case())
    src = c["src"].clone()
    src[BAD_EDGES[0]], src[BAD_EDGES[1]], src[BAD_EDGES[2]] = C.N_SRC, -1, 1 << 30
    c.update(src=src, n_src=C.N_SRC, M=C.M_DST)
    return c


def _long_case():
    """E = 4097 edges over 2 sources (17 targets of 241 edges): runs of about 2048 edges, which run_sum cuts into 8 pieces."""
    g = torch.Generator().manual_seed(31)
    E, n, M = 4097, 2, 17
    return dict(src=torch.randint(0, 2, (E,), generator=g).to(torch.int32), ptr=torch.arange(0, E + 1, 241, dtype=torch.int32),
                pos_src=torch.rand(n, 4, generator=g), pos_dst=torch.rand(M, 4, generator=g), E=E, n_src=n, M=M)


_fp32 = {}


def _reference(L, name, C1):
    """The case `name` at width C1 on the GPU, its P and Wg, and geo / H1 of the fp32 entry point p2w_edge_l1: computed once."""
    key = (name, C1)
    if key not in _fp32:
        ptr, stream = _abi()
        c = {"edge": _edge_case, "long": _long_case}[name]() if name != "planted" else R.planted_case(C1)
        g = torch.Generator().manual_seed(100 + C1)
        P = c["P"] if "P" in c else torch.randn(c["n_src"], C1, generator=g)
        Wg = c["Wg"] if "Wg" in c else torch.randn(4, C1, generator=g)
        d = {k: c[k].cuda() for k in ("pos_src", "pos_dst", "ptr", "src")}
        d.update(P=P.cuda(), Wg=Wg.cuda(), E=c["E"], n_src=c["n_src"], M=c["M"], cols=c.get("cols"))
        geo, H1 = torch.full((c["E"] + 1, 4), NAN, device="cuda"), torch.full((c["E"] + 1, C1), NAN, device="cuda")
        assert L.p2w_edge_l1(ptr(d["P"]), C1, ptr(d["pos_src"]), ptr(d["pos_dst"]), ptr(d["ptr"]), ptr(d["src"]), ptr(d["Wg"]), d["n_src"],
                             d["M"], d["E"], C1, ptr(geo), ptr(H1), C1, stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(geo[-1]).all()) and bool(torch.isnan(H1[-1]).all())
        d.update(geo=geo[:-1].contiguous(), H1=H1[:-1].contiguous())
        _fp32[key] = d
    return _fp32[key]


# ------------------------------------------------------------------------------------------------ forward through the C ABI
@pytest.mark.parametrize("C1", WIDTHS)
@pytest.mark.parametrize("th", [F32, F16, BF16])
def test_forward_io_equals_the_fp32_entry_point_rounded_once(L, th, C1):
    """p2w_edge_l1_io on the edge case with three sources outside [0, n_src): geo bit for bit the fp32 entry point's; H1 with th = F32
    bit for bit the fp32 entry point's, with th = F16 / BF16 bit for bit .half() / .bfloat16() of it (converted on the CPU).  Dense
    rows, rows pitched beyond C1, and - 16-bit, C1 a multiple of 4 - a base that is 8-byte aligned only: the columns between C1 and
    the pitch and the row behind the last edge stay untouched.  The bad sources' rows are 0 in geo and H1."""
    ptr, stream = _abi()
    d = _reference(L, "edge", C1)
    E, dt = d["E"], DT[th]
    want = d["H1"].cpu().to(dt)
    assert bool((d["H1"][list(BAD_EDGES)] == 0).all()) and bool((d["geo"][list(BAD_EDGES)] == 0).all())
    assert bool((d["H1"] > 0).any()) and bool((d["H1"] == 0).any())
    layouts = [(C1, 0), (_pitch(C1), 0)] + ([(_pitch(C1), 4)] if th != F32 and C1 % 4 == 0 else [])
    for ld, off in layouts:
        ldp = ld
        Pp = _pitched(d["P"], ldp)
        geo, H1 = torch.full((E + 1, 4), NAN, device="cuda"), _buf(E + 1, ld, dt, 3.0, off)
        assert L.p2w_edge_l1_io(ptr(Pp), ldp, ptr(d["pos_src"]), ptr(d["pos_dst"]), ptr(d["ptr"]), ptr(d["src"]), ptr(d["Wg"]), d["n_src"],
                                d["M"], E, C1, ptr(geo), ptr(H1), th, ld, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_ibits(geo[:E]), _ibits(d["geo"])) and bool(torch.isnan(geo[E]).all())
        assert torch.equal(_ibits(H1[:E, :C1]).cpu(), _ibits(want)), (ld, off)
        assert bool((H1[:E, C1:] == 3.0).all()) and bool((H1[E] == 3.0).all())


# ------------------------------------------------------------------------------------------------ backward through the C ABI
def _bwd_fp32(L, d, C1, g32):
    """p2w_edge_l1_bwd on an fp32 gradient and the fp32 H1 of the reference."""
    ptr, stream = _abi()
    E, n = d["E"], d["n_src"]
    need = int(L.p2w_edge_l1_bwd_ws_bytes(E, n, C1))
    gP, gR, gWg = torch.full((n, C1), NAN, device="cuda"), torch.full((n,), NAN, device="cuda"), torch.full((4, C1), NAN, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert L.p2w_edge_l1_bwd(ptr(g32), C1, ptr(d["H1"]), C1, ptr(d["geo"]), ptr(d["src"]), ptr(d["Wg"]), n, E, C1, ptr(gP), C1, ptr(gR),
                             ptr(gWg), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    return gP, gR, gWg


def _bwd_io(L, d, C1, tg, g, ld=None, off=0):
    """p2w_edge_l1_bwd_io on the gradient in its dtype, the workspace filled with 0xFF, the outputs with NaN; pitched with ld."""
    ptr, stream = _abi()
    E, n, ld = d["E"], d["n_src"], ld or C1
    need = int(L.p2w_edge_l1_bwd_ws_bytes(E, n, C1))
    gp, Pp = _pitched(g, ld, DT[tg], off), _pitched(d["P"], ld)
    gP, gR, gWg = torch.full((n + 1, ld), NAN, device="cuda"), torch.full((n + 1,), NAN, device="cuda"), torch.full((5, C1), NAN, device="cuda")
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    assert L.p2w_edge_l1_bwd_io(ptr(gp), tg, ld, ptr(Pp), ld, ptr(d["geo"]), ptr(d["src"]), ptr(d["Wg"]), n, E, C1, ptr(gP), ld, ptr(gR),
                                ptr(gWg), ptr(ws), need, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(gP[n]).all()) and bool(torch.isnan(gR[n])) and bool(torch.isnan(gWg[4]).all()) and bool(torch.isnan(gP[:, C1:]).all())
    return gP[:n, :C1].contiguous(), gR[:n].contiguous(), gWg[:4].contiguous()


def _gradient(E, C1, tg, seed):
    """A gradient representable in tg's dtype, and its exact widening."""
    g = torch.randn(E, C1, generator=torch.Generator().manual_seed(seed)).to(DT[tg])
    return g.cuda(), g.float().cuda()


def _assert_equal(got, want, what):
    for name, a, b in zip(("gP", "gR", "gWg"), got, want):
        assert _same(a, b), (what, name)


@pytest.mark.parametrize("C1", WIDTHS)
@pytest.mark.parametrize("tg", [F32, F16, BF16])
def test_backward_io_equals_the_fp32_entry_point(L, tg, C1):
    """p2w_edge_l1_bwd_io on the edge case (E spans several 1 024-edge chunks, the hub's run is about 3000 edges, three sources lie
    outside [0, n_src) and their gradient rows are +inf): gP, gR and gWg bit for bit p2w_edge_l1_bwd on the widened gradient and the
    fp32 H1.  The workspace arrives filled with 0xFF; a second call, and one with pitches beyond C1 (16-bit, C1 a multiple of 4: on a
    base that is 8-byte aligned only), give the same bits; everything stays finite."""
    d = _reference(L, "edge", C1)
    g, g32 = _gradient(d["E"], C1, tg, 200 + C1)
    g[list(BAD_EDGES)], g32[list(BAD_EDGES)] = float("inf"), float("inf")
    want = _bwd_fp32(L, d, C1, g32)
    got = _bwd_io(L, d, C1, tg, g)
    _assert_equal(got, want, "dense")
    assert all(bool(torch.isfinite(t).all()) for t in got) and float(got[0][C.HUB].abs().max()) > 0 and float(got[2].abs().max()) > 0
    _assert_equal(_bwd_io(L, d, C1, tg, g), got, "second call")
    _assert_equal(_bwd_io(L, d, C1, tg, g, _pitch(C1), 4 if tg != F32 and C1 % 4 == 0 else 0), got, "pitched")


@pytest.mark.parametrize("C1", [32, 33])
@pytest.mark.parametrize("tg", [F16, BF16])
def test_backward_io_on_split_runs(L, tg, C1):
    """E = 4097 edges over 2 sources: run_sum cuts each run into 8 pieces and adds the partial rows, at both panel widths."""
    d = _reference(L, "long", C1)
    g, g32 = _gradient(d["E"], C1, tg, 300 + C1)
    got = _bwd_io(L, d, C1, tg, g)
    _assert_equal(got, _bwd_fp32(L, d, C1, g32), "long runs")
    _assert_equal(_bwd_io(L, d, C1, tg, g), got, "second call")
    assert int((got[0] != 0).sum()) > C1          # (a column whose pre-activation is negative on all of a source's edges gives 0)


@pytest.mark.parametrize("tg", [F32, F16, BF16])
def test_backward_io_without_edges(L, tg):
    """E = 0: every element of gP, gR and gWg is written, with zeros, as by the fp32 entry point; gH, P, geo and src may be NULL."""
    ptr, stream = _abi()
    n, C1 = 5, 8
    need = int(L.p2w_edge_l1_bwd_ws_bytes(0, n, C1))
    Wg = torch.randn(4, C1, device="cuda")
    outs = []
    for io in (True, False):
        gP, gR, gWg = torch.full((n, C1), NAN, device="cuda"), torch.full((n,), NAN, device="cuda"), torch.full((4, C1), NAN, device="cuda")
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        if io:
            st = L.p2w_edge_l1_bwd_io(None, tg, C1, None, C1, None, None, ptr(Wg), n, 0, C1, ptr(gP), C1, ptr(gR), ptr(gWg), ptr(ws), need, stream())
        else:
            st = L.p2w_edge_l1_bwd(None, C1, None, C1, None, None, ptr(Wg), n, 0, C1, ptr(gP), C1, ptr(gR), ptr(gWg), ptr(ws), need, stream())
        assert st == 0
        torch.cuda.synchronize()
        outs.append((gP, gR, gWg))
    _assert_equal(outs[0], outs[1], "E = 0")
    assert all(bool((t == 0).all()) for t in outs[0])


# ------------------------------------------------------------------------------------------------ planted values
@pytest.mark.parametrize("C1", [8, 6])
@pytest.mark.parametrize("t", [F16, BF16])
def test_planted_values_keep_their_gradient(L, t, C1):
    """tests/edge_io_ref.py's planted case: columns 1 and 2 of Wg are zero, so h = P[j, c] exactly there, and P carries the table
    (2^-25, 2^-26, 1e-30, 1e-40, the neighbours of the float16 ties, 1e-44, bfloat16's carry to inf, ...) plus -0.0, a negative tiny
    value, a NaN and +inf.  The stored H1 is torch's conversion of the fp32 H1 - the table's own patterns in the planted columns.
    Every source has exactly one edge, so gP[s, c] must BE that edge's gradient wherever the fp32 h is > 0 - the elements whose
    stored value is zero included, which a mask read from the 16-bit H1 would drop - and 0 elsewhere; gP, gR, gWg equal
    p2w_edge_l1_bwd on the fp32 H1 bit for bit."""
    ptr, stream = _abi()
    d = _reference(L, "planted", C1)
    E, n, dt = d["E"], d["n_src"], DT[t]
    H1 = _buf(E, C1, dt)
    geo = torch.full((E, 4), NAN, device="cuda")
    assert L.p2w_edge_l1_io(ptr(d["P"]), C1, ptr(d["pos_src"]), ptr(d["pos_dst"]), ptr(d["ptr"]), ptr(d["src"]), ptr(d["Wg"]), n, d["M"], E,
                            C1, ptr(geo), ptr(H1), t, C1, stream()) == 0
    torch.cuda.synchronize()
    h32 = d["H1"].cpu()
    assert _same(H1, h32.to(dt)) and torch.equal(_ibits(geo), _ibits(d["geo"]))
    j = d["src"].cpu().long()
    table = torch.from_numpy((R.TABLE_F16 if t == F16 else R.TABLE_BF16).astype(np.int16))
    planted = torch.from_numpy(R.PLANTED32.copy())
    for col, shift in zip(d["cols"], (0, 5)):
        src_of_entry = (torch.arange(len(R.TABLE)) - shift) % R.N_PLANTED          # P[s, col] = PLANTED32[(s + shift) % 16]
        edge_of_source = torch.empty(n, dtype=torch.long)
        edge_of_source[j] = torch.arange(E)
        assert torch.equal(_ibits(H1.cpu())[edge_of_source[src_of_entry], col], table)
        assert torch.equal(h32[:, col], torch.relu(planted.roll(-shift)[j]).nan_to_num(nan=0.0, posinf=float("inf")))     # h = relu(P[j, c]) exactly
    lost = (h32 > 0) & (H1.cpu().float() == 0)
    assert int(lost.sum()) >= (8 if t == F16 else 2) and not bool(lost[:, [0, 3]].any())
    g, g32 = _gradient(E, C1, t, 400 + C1)
    g[g == 0], g32[g32 == 0] = 1.0, 1.0
    got = _bwd_io(L, d, C1, t, g)
    _assert_equal(got, _bwd_fp32(L, d, C1, g32), "planted")
    want_gP = torch.zeros(n, C1)
    want_gP[j] = torch.where(h32 > 0, g32.cpu(), torch.zeros(()))
    assert torch.equal(_ibits(got[0].cpu()), _ibits(want_gP))
    lost_by_source = torch.zeros(n, C1, dtype=torch.bool)
    lost_by_source[j] = lost
    assert bool((got[0].cpu()[lost_by_source] != 0).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(L):
    """Unknown codes: P2W_EUNSUPPORTED ahead of every other check.  On fp32, float16 and bfloat16 tensors: null pointers (-2), pitches
    and pointers the 4-column lanes cannot take (-3), bad sizes and pitches below C1 (-1), a workspace that is too small (-4) - all
    before anything is launched, so the NaN-filled outputs stay NaN.  Then the good calls write them."""
    ptr, stream = _abi()
    n, M, C1, E = 12, 5, 8, 14
    csr = torch.tensor([0, 3, 3, 10, 11, 14], dtype=torch.int32, device="cuda")
    src = (torch.arange(E, dtype=torch.int32) % n).cuda()
    P, Wg = torch.randn(n + 1, C1, device="cuda"), torch.randn(5, C1, device="cuda")
    rs, rd = torch.rand(n + 1, 4, device="cuda"), torch.rand(M + 1, 4, device="cuda")
    need = int(L.p2w_edge_l1_bwd_ws_bytes(E, n, C1))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    gs = torch.rand(E + 1, 4, device="cuda")
    s = stream()
    for t in (F32, F16, BF16):
        geo = torch.full((E + 1, 4), NAN, device="cuda")
        H1 = _buf(E + 1, C1 + 4, DT[t])
        gH = torch.randn(E + 1, C1, device="cuda").to(DT[t])
        gP = torch.full((n + 1, C1 + 4), NAN, device="cuda")
        gR, gWg = torch.full((n + 1,), NAN, device="cuda"), torch.full((5, C1), NAN, device="cuda")

        def fwd(t_=t, P_=ptr(P), ldp=C1, rs_=ptr(rs), rd_=ptr(rd), csr_=ptr(csr), src_=ptr(src), Wg_=ptr(Wg), n_=n, M_=M, E_=E, C1_=C1,
                geo_=ptr(geo), H1_=ptr(H1), ldh=C1 + 4):
            return L.p2w_edge_l1_io(P_, ldp, rs_, rd_, csr_, src_, Wg_, n_, M_, E_, C1_, geo_, H1_, t_, ldh, s)

        def bwd(t_=t, gH_=ptr(gH), ldg=C1, P_=ptr(P), ldp=C1, geo_=ptr(gs), src_=ptr(src), Wg_=ptr(Wg), n_=n, E_=E, C1_=C1, gP_=ptr(gP),
                ldgp=C1 + 4, gR_=ptr(gR), gWg_=ptr(gWg), ws_=ptr(ws), wsb=need):
            return L.p2w_edge_l1_bwd_io(gH_, t_, ldg, P_, ldp, geo_, src_, Wg_, n_, E_, C1_, gP_, ldgp, gR_, gWg_, ws_, wsb, s)

        for code in (3, -1):
            assert fwd(t_=code) == EUNSUPPORTED and bwd(t_=code) == EUNSUPPORTED
            assert fwd(t_=code, H1_=None) == EUNSUPPORTED and fwd(t_=code, C1_=0) == EUNSUPPORTED and fwd(t_=code, ldh=C1 + 1) == EUNSUPPORTED
            assert bwd(t_=code, gH_=None) == EUNSUPPORTED and bwd(t_=code, ldg=1) == EUNSUPPORTED and bwd(t_=code, wsb=0) == EUNSUPPORTED
        for name in ("P_", "rs_", "rd_", "csr_", "src_", "Wg_", "geo_", "H1_"):
            assert fwd(**{name: None}) == ENULL, name
        for name in ("gH_", "P_", "geo_", "src_", "Wg_", "gP_", "gR_", "gWg_", "ws_"):
            assert bwd(**{name: None}) == ENULL, name
        el = H1.element_size()
        assert fwd(ldp=C1 + 2) == EALIGN and fwd(ldh=C1 + 1) == EALIGN and fwd(P_=ptr(P) + 4) == EALIGN and fwd(Wg_=ptr(Wg) + 4) == EALIGN
        assert fwd(H1_=ptr(H1) + 2 * el) == EALIGN and fwd(rs_=ptr(rs) + 4) == EALIGN and fwd(rd_=ptr(rd) + 8) == EALIGN
        assert fwd(geo_=ptr(geo) + 4) == EALIGN
        assert fwd(ldp=C1 - 4) == EINVAL and fwd(ldh=4) == EINVAL and fwd(C1_=0) == EINVAL and fwd(n_=-1) == EINVAL and fwd(M_=-1) == EINVAL
        assert fwd(E_=-1) == EINVAL and fwd(M_=0) == EINVAL and fwd(n_=0) == EINVAL
        assert fwd(M_=0, E_=0) == 0 and fwd(E_=0) == 0                       # nothing to do: nothing launched
        assert bwd(ldg=C1 + 2) == EALIGN and bwd(ldp=C1 + 1) == EALIGN and bwd(ldgp=C1 + 3) == EALIGN and bwd(gH_=ptr(gH) + 2 * el) == EALIGN
        assert bwd(P_=ptr(P) + 8) == EALIGN and bwd(Wg_=ptr(Wg) + 4) == EALIGN and bwd(gP_=ptr(gP) + 4) == EALIGN
        assert bwd(gWg_=ptr(gWg) + 4) == EALIGN and bwd(geo_=ptr(gs) + 4) == EALIGN and bwd(ws_=ptr(ws) + 4) == EALIGN
        assert bwd(ldg=4) == EINVAL and bwd(ldp=C1 - 4) == EINVAL and bwd(ldgp=4) == EINVAL and bwd(C1_=0) == EINVAL
        assert bwd(n_=-1) == EINVAL and bwd(E_=-1) == EINVAL and bwd(n_=0) == EINVAL
        assert bwd(wsb=need - 1) == EWORKSPACE and bwd(wsb=0) == EWORKSPACE
        torch.cuda.synchronize()
        for x in (geo, H1, gP, gR, gWg):
            assert bool(torch.isnan(x).all())
        assert fwd() == 0 and bwd() == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(geo[:E]).all()) and bool(torch.isnan(geo[E]).all())
        assert bool(torch.isfinite(H1[:E, :C1]).all()) and bool(torch.isnan(H1[:, C1:]).all()) and bool(torch.isnan(H1[E]).all())
        assert bool(torch.isfinite(gP[:n, :C1]).all()) and bool(torch.isnan(gP[:, C1:]).all()) and bool(torch.isnan(gP[n]).all())
        assert bool(torch.isfinite(gR[:n]).all()) and bool(torch.isnan(gR[n])) and bool(torch.isfinite(gWg[:4]).all()) and bool(torch.isnan(gWg[4]).all())


# ------------------------------------------------------------------------------------------------ the operator
class _Saved:
    """saved_tensors_hooks that record what the graph keeps for its backward."""

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

    def fp32_of(self, *shapes):
        return sum(1 for dt, shape, _ in self.kept if dt == torch.float32 and shape in shapes)


def _operator_inputs(dtype, C1=16):
    c, g = C.edge_case(), torch.Generator().manual_seed(500)
    ei = torch.stack([c["src"].long(), c["i"]], 0).cuda()
    P = torch.randn(C.N_SRC, C1, generator=g).to(dtype).cuda().requires_grad_()
    Wg = torch.randn(4, C1, generator=g).cuda().requires_grad_()
    ps = c["pos_src"].cuda().clone().requires_grad_()
    return P, Wg, ps, c["pos_dst"].cuda(), ei, torch.randn(c["E"], C1, generator=g).to(dtype).cuda()


def _operator_route(H, dtype, new, cotangent=None):
    P, Wg, ps, pd, ei, g = _operator_inputs(dtype)
    with torch.autocast("cuda", dtype=dtype), _Saved() as saved:
        if new:
            out = H.edge_layer1(P, Wg, ps, pd, ei, out_dtype=dtype)
            fn = out.grad_fn
        else:
            first = H.edge_layer1(P, Wg, ps, pd, ei)
            fn, out = first.grad_fn, first.to(dtype)
            assert first.dtype == torch.float32
    out.backward(g if cotangent is None else g.to(cotangent))
    return dict(out=out.detach(), P=P.grad, Wg=Wg.grad, pos_src=ps.grad), saved, type(fn).__name__


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_operator_out_dtype_against_the_default_call(H, L, dtype):
    """ops.edge_layer1(..., out_dtype=dt) under autocast(dt) against the default call followed by .to(dt): the output and the
    gradients to P (dt), Wg and pos_src (fp32) bit for bit.  The new route saves no [E, C1] tensor, the default one fp32 tensor of
    that shape.  The default call is what it was: fp32 out under autocast, the bits of p2w_edge_l1, _EdgeLayer1's node.  An fp32
    cotangent at the 16-bit output is accepted and gives the same gradients; without a gradient to track the same bits come back
    and nothing is saved; another out_dtype is refused."""
    new, kept_new, fn_new = _operator_route(H, dtype, True)
    old, kept_old, fn_old = _operator_route(H, dtype, False)
    assert set(new) == set(old)
    for k in new:
        assert _same(new[k], old[k]), k
    E, C1 = new["out"].shape
    assert new["out"].dtype == dtype and new["P"].dtype == dtype and new["Wg"].dtype == torch.float32 and new["pos_src"].dtype == torch.float32
    assert float(new["P"].float().abs().max()) > 0 and bool((new["pos_src"][:, :3] == 0).all()) and float(new["pos_src"][:, 3].abs().max()) > 0
    assert not [k for k in kept_new.kept if k[1] == (E, C1)], kept_new.kept
    assert kept_old.fp32_of((E, C1)) == 1 and kept_new.fp32_of((E, C1)) == 0
    assert (fn_new, fn_old) == ("_EdgeLayer1HalfBackward", "_EdgeLayer1Backward")
    wide, _, _ = _operator_route(H, dtype, True, cotangent=torch.float32)
    for k in new:
        assert _same(wide[k], new[k]), k
    # the default call's bits: the fp32 entry point on the widened P
    ptr, stream = _abi()
    P, Wg, ps, pd, ei, _ = _operator_inputs(dtype)
    with torch.autocast("cuda", dtype=dtype):
        first = H.edge_layer1(P, Wg, ps, pd, ei)
        with torch.no_grad(), _Saved() as nothing:
            plain = H.edge_layer1(P, Wg, ps, pd, ei, out_dtype=dtype)
    c = C.edge_case()
    geo, H1 = torch.empty(E, 4, device="cuda"), torch.empty(E, C1, device="cuda")
    P32 = P.detach().float()
    assert L.p2w_edge_l1(ptr(P32), C1, ptr(ps.detach()), ptr(pd), ptr(c["ptr"].cuda()), ptr(c["src"].cuda()), ptr(Wg.detach()), C.N_SRC,
                         C.M_DST, E, C1, ptr(geo), ptr(H1), C1, stream()) == 0
    assert first.dtype == torch.float32 and torch.equal(_ibits(first), _ibits(H1))
    assert plain.grad_fn is None and not nothing.kept and _same(plain, new["out"])
    with pytest.raises(RuntimeError, match="out_dtype"):
        H.edge_layer1(P, Wg, ps, pd, ei, out_dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the layer
def _mlp_for():
    from tests.test_gpu_ops_backward import _mlp
    return _mlp([12, 16, 32], seed=8)


def _layer_route(H, on, dtype, fused, c, seen):
    old, H.half_io = H.half_io, on
    try:
        conv = H.PointNetConv(local_nn=_mlp_for(), global_nn=None, add_self_loops=False).cuda().train()
        conv.fused_bn_max = fused
        x, ps = c["x"].cuda().requires_grad_(), c["pos_src"].cuda().requires_grad_()
        n0 = len(seen)
        with torch.autocast("cuda", dtype=dtype), _Saved() as saved:
            out = conv(x, (ps, c["pos_dst"].cuda()), c["ei"].cuda())
        (out.float() * c["g"].cuda()).sum().backward()
    finally:
        H.half_io = old
    bn = conv.local_nn[1][2]
    r = dict(out=out.detach(), x=x.grad, pos_src=ps.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
             **{k: p.grad.clone() for k, p in conv.named_parameters()})
    return r, saved, seen[n0:]


def _spy_on_edge_layer1(H, monkeypatch):
    """Records (requested out_dtype, the result's dtype and shape) of every call PointNetConv makes through ops.edge_layer1."""
    seen, inner = [], H.edge_layer1

    def spy(*a, **k):
        out = inner(*a, **k)
        seen.append((k.get("out_dtype"), out.dtype, tuple(out.shape)))
        return out
    monkeypatch.setattr(H, "edge_layer1", spy)
    return seen


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_layer_half_io_on_against_off(H, dtype, fused, monkeypatch):
    """ops.PointNetConv(local_nn=MLP([12, 16, 32])) in training mode under autocast, fused_bn_max False and True: half_io on against
    off - the output, every parameter gradient, the gradients to x and pos_src and the running statistics bit for bit.  On asks
    edge_layer1 for the autocast dtype and keeps no fp32 [E, C1] tensor; off asks for nothing, gets fp32 and keeps one."""
    from tests.test_gpu_conv_train import _layer_case
    c = _layer_case(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    seen = _spy_on_edge_layer1(H, monkeypatch)
    on, kept_on, calls_on = _layer_route(H, True, dtype, fused, c, seen)
    off, kept_off, calls_off = _layer_route(H, False, dtype, fused, c, seen)
    big = (c["ei"].shape[1], 16)
    assert calls_on == [(dtype, dtype, big)] and calls_off == [(None, torch.float32, big)]
    assert set(on) == set(off) and len(on) >= 11
    for k in on:
        assert _same(on[k], off[k]), k
        assert bool(torch.isfinite(on[k]).all()), k
    assert float(on["x"].abs().max()) > 0 and float(on["pos_src"][:, 3].abs().max()) > 0
    assert kept_on.fp32_of(big) == 0 and kept_off.fp32_of(big) == 1, (kept_on.kept, kept_off.kept)
    with torch.no_grad():       # without autocast nothing changes: edge_layer1 is asked for nothing
        conv = H.PointNetConv(local_nn=_mlp_for(), add_self_loops=False).cuda().train()
        conv(c["x"].cuda(), (c["pos_src"].cuda(), c["pos_dst"].cuda()), c["ei"].cuda())
    assert seen[-1] == (None, torch.float32, big)


# ------------------------------------------------------------------------------------------------ the whole network
def _net_step(H, dtype, on, seen):
    """tests/test_gpu_train_net.py's training step (a freshly initialised train.Net(1, 8), two voxels of 600 and 200 points) as
    trainer.SemanticTraining takes it: float16 with GradScaler(512), bfloat16 with the scaler disabled; one AdamW step."""
    from pointstowood_amd.loss import Poly1FocalLoss
    from pointstowood_amd.trainer import finish_step
    from tests import net_train_ref as NR
    from tests import test_gpu_train_net as TN
    old, H.half_io = H.half_io, on
    try:
        torch.manual_seed(TN.SEED)
        d = TN._data(NR.inputs(TN.SEED))
        net = TN._net(None)
        criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
        optimizer = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
        scaler = torch.amp.GradScaler("cuda", init_scale=512, enabled=dtype == torch.float16)
        before = {k: v.detach().clone() for k, v in net.state_dict().items()}
        optimizer.zero_grad()
        n0 = len(seen)
        with torch.autocast("cuda", dtype=dtype), _Saved() as saved:
            outputs = net(d)
            loss, _ = criterion(outputs, d.y)
        scaler.scale(loss).backward()
        skipped = finish_step(net, optimizer, scaler, "fp16" if dtype == torch.float16 else "bf16")
    finally:
        H.half_io = old
    r = dict(logits=outputs.detach(), loss=loss.detach(), **{"grad." + k: p.grad.clone() for k, p in net.named_parameters()},
             **{"state." + k: v.detach().clone() for k, v in net.state_dict().items()})
    moved = sum(1 for k, p in net.named_parameters() if not torch.equal(p.detach(), before[k]))
    return r, saved, seen[n0:], skipped, moved


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_net_training_step_half_io_on_against_off(H, dtype, monkeypatch):
    """One whole AdamW step of train.Net at C = 8 under autocast, ops.half_io on against off: the logits, the loss, every gradient,
    every parameter and every buffer after the step bit for bit.  The three PointNetConv levels ask edge_layer1 for the autocast
    dtype when on and for nothing when off; of the fp32 tensors of the three [E, C1] shapes the graph keeps 0 on and 3 off."""
    seen = _spy_on_edge_layer1(H, monkeypatch)
    on, kept_on, calls_on, skipped_on, moved = _net_step(H, dtype, True, seen)
    off, kept_off, calls_off, skipped_off, _ = _net_step(H, dtype, False, seen)
    assert [c[:2] for c in calls_on] == [(dtype, dtype)] * 3 and [c[:2] for c in calls_off] == [(None, torch.float32)] * 3
    shapes = [c[2] for c in calls_on]
    print("EDGE_IO kept fp32 [E, C1]:", kept_on.fp32_of(*shapes), "on,", kept_off.fp32_of(*shapes), "off; shapes", shapes)
    assert shapes == [c[2] for c in calls_off] and len(set(shapes)) == 3
    assert set(on) == set(off) and len([k for k in on if k.startswith("grad.")]) == 158
    for k in on:
        assert _same(on[k], off[k]), k
    assert bool(torch.isfinite(on["logits"]).all()) and bool(torch.isfinite(on["loss"]))
    assert all(bool(torch.isfinite(v).all()) for k, v in on.items() if k.startswith("grad."))
    assert skipped_on == skipped_off == 0 and moved > 100
    assert kept_on.fp32_of(*shapes) == 0 and kept_off.fp32_of(*shapes) == 3
