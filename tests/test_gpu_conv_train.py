"""The training route of ops.PointNetConv: p2w_edge_l1 / p2w_edge_l1_bwd (csrc/p2w_edge.hip) through the C ABI against the
float64 references and caps of tests/conv_train_ref.py, ops.edge_layer1, and the layer in training mode against the same layer
over oracle/ops.py in float64.

``python -m tests.test_gpu_conv_train`` (no GPU needed) rewrites tests/golden/conv_train/noise.json: per compared tensor, the
relative L2 error of the oracle layer (reference-style message() + local_nn over oracle/ops.py, training-mode BatchNorm) in fp32
against itself in fp64, both on the CPU."""
import copy
import json
import os

import pytest
import torch

from oracle import ops as O
from tests import conv_train_ref as R
from tests.test_gpu_ops_backward import _OracleMessagePassing, _block_data, _mlp, _ref_style_conv, _rel_l2

pytestmark = pytest.mark.gpu

NOISE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_train", "noise.json")
WIDTHS = [6, 16, 64, 384]          # 4-byte lanes; 16-byte lanes with 4, 16 and 64 + 32 lanes per row (two 256-column panels)
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


def _pitch(C1):
    """A row pitch larger than C1 that keeps the access width of C1."""
    return C1 + 8 if C1 % 4 == 0 else C1 + 3


def _pitched(t, ld, fill=float("nan")):
    """t's rows in a buffer of pitch ld whose other columns hold `fill`."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf


_gpu_fwd = {}


def _forward_on_gpu(L, C1):
    """(geo, H1) of p2w_edge_l1 with dense rows, computed once per width: the backward test takes its mask from them."""
    if C1 not in _gpu_fwd:
        ptr, stream = _abi()
        c, f = R.edge_case(), R.forward_case(C1)
        d = {k: c[k].cuda() for k in ("pos_src", "pos_dst", "ptr", "src")}
        P, Wg = f["P"].cuda(), f["Wg"].cuda()
        geo = torch.full((c["E"] + 1, 4), float("nan"), device="cuda")
        H1 = torch.full((c["E"] + 1, C1), float("nan"), device="cuda")
        assert L.p2w_edge_l1(ptr(P), C1, ptr(d["pos_src"]), ptr(d["pos_dst"]), ptr(d["ptr"]), ptr(d["src"]), ptr(Wg), R.N_SRC, R.M_DST,
                             c["E"], C1, ptr(geo), ptr(H1), C1, stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(geo[-1]).all()) and bool(torch.isnan(H1[-1]).all())          # nothing behind the last edge
        _gpu_fwd[C1] = (geo[:-1].cpu(), H1[:-1].cpu(), d, P, Wg)
    return _gpu_fwd[C1]


@pytest.mark.parametrize("C1", WIDTHS)
def test_kernel_forward_against_fp64(L, C1):
    """p2w_edge_l1 through the ABI on conv_train_ref.edge_case() (degrees 0, 1, 32, 33, 100 and 1500, a target on top of all its
    neighbours, unreferenced sources): every element of geo within 4 EPS |geo| (exactly 0 on the coincident target, the reflectance
    a copy) and every element of H1 within 8 EPS (|P| + sum |geo_d Wg_d|) of the float64 reference - the operation counts behind the
    two constants are derived in conv_train_ref's docstring.  Then the same call with row pitches larger than C1: the same bits,
    and the columns between C1 and the pitch untouched."""
    ptr, stream = _abi()
    c, f = R.edge_case(), R.forward_case(C1)
    geo, H1, d, P, Wg = _forward_on_gpu(L, C1)
    rg, rh = R.ratio(geo, f["geo"], f["cap_geo"]), R.ratio(H1, f["H1"], f["cap_H1"])
    print(f"EDGE_RATIO forward C1={C1} geo {rg:.3f} H1 {rh:.3f}")
    assert rg <= 1.0 and rh <= 1.0
    assert bool((geo[c["i"] == R.COINCIDENT, :3] == 0).all())
    assert bool((H1 == 0).any()) and bool((H1 > 0).any())
    ld = _pitch(C1)
    Pp, H1p = _pitched(f["P"], ld), torch.full((c["E"], ld), 3.0, device="cuda")
    geo2 = torch.full((c["E"], 4), float("nan"), device="cuda")
    assert L.p2w_edge_l1(ptr(Pp), ld, ptr(d["pos_src"]), ptr(d["pos_dst"]), ptr(d["ptr"]), ptr(d["src"]), ptr(Wg), R.N_SRC, R.M_DST, c["E"],
                         C1, ptr(geo2), ptr(H1p), ld, stream()) == 0
    assert torch.equal(H1p[:, :C1].cpu().view(torch.int32), H1.view(torch.int32)) and bool((H1p[:, C1:] == 3.0).all())
    assert torch.equal(geo2.cpu().view(torch.int32), geo.view(torch.int32))


@pytest.mark.parametrize("C1", WIDTHS)
def test_kernel_backward_against_fp64_sums(L, C1):
    """p2w_edge_l1_bwd through the ABI on the GPU forward's own H1 and geo (so a pre-activation near 0 cannot flip the mask):
    gP[s, c] within len_s EPS sum |gZ| of the float64 sum over the source's run (the hub's run is about 3000 edges), gR[s] within
    (len_s + C1 + 1) EPS sum |gZ Wg3|, gWg within (E + 1) EPS sum |geo gZ| (conv_train_ref's docstring); rows and entries of sources
    without edges exactly 0; a second call into fresh buffers, and one with pitches larger than C1, give the same bits."""
    ptr, stream = _abi()
    c = R.edge_case()
    geo, H1, d, P, Wg = _forward_on_gpu(L, C1)
    E, n = c["E"], R.N_SRC
    gH = torch.randn(E, C1, generator=torch.Generator().manual_seed(200 + C1))
    ref, caps = R.backward_reference(gH, H1, geo, c["src"], Wg.cpu(), n)
    need = int(L.p2w_edge_l1_bwd_ws_bytes(E, n, C1))
    assert need > 0

    def run(ld):
        g, h = _pitched(gH, ld), _pitched(H1, ld)
        dgeo = geo.cuda()
        gP, gR = torch.full((n + 1, ld), float("nan"), device="cuda"), torch.full((n + 1,), float("nan"), device="cuda")
        gWg, ws = torch.full((5, C1), float("nan"), device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")
        assert L.p2w_edge_l1_bwd(ptr(g), ld, ptr(h), ld, ptr(dgeo), ptr(d["src"]), ptr(Wg), n, E, C1, ptr(gP), ld, ptr(gR), ptr(gWg),
                                 ptr(ws), need, stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(gP[n]).all()) and bool(torch.isnan(gR[n])) and bool(torch.isnan(gWg[4]).all())
        assert bool(torch.isnan(gP[:n, C1:]).all())
        return gP[:n, :C1].cpu(), gR[:n].cpu(), gWg[:4].cpu()

    got = run(C1)
    ratios = [R.ratio(g_, r_, c_) for g_, r_, c_ in zip(got, ref, caps)]
    print(f"EDGE_RATIO backward C1={C1} gP {ratios[0]:.3f} gR {ratios[1]:.3f} gWg {ratios[2]:.3f}")
    assert max(ratios) <= 1.0
    unref = torch.bincount(c["src"].long(), minlength=n) == 0
    assert int(unref.sum()) >= 13 and bool((got[0][unref] == 0).all()) and bool((got[1][unref] == 0).all())
    assert float(got[0][R.HUB].abs().max()) > 0 and float(got[1].abs().max()) > 0
    for other in (run(C1), run(_pitch(C1))):
        for a, b in zip(got, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the layer
def _layer_case(knn):
    d = _block_data(knn)
    g = torch.randn(d["idx"].numel(), 32, generator=torch.Generator().manual_seed(43))
    return dict(x=d["x"], pos_src=d["pos4"], pos_dst=d["pos4"][d["idx"]].clone(), ei=d["ei"], g=g)


def _layer_results(conv, c, dev):
    """One training-mode forward and backward of sum(out * g): output, running statistics and gradients by name."""
    to = lambda t: t.to(dev) if not t.is_floating_point() else t.to(dev, next(conv.parameters()).dtype)       # noqa: E731
    x, ps = to(c["x"]).detach().clone().requires_grad_(), to(c["pos_src"]).detach().clone().requires_grad_()
    conv.train()
    conv.zero_grad()
    out = conv(x, (ps, to(c["pos_dst"])), to(c["ei"]))
    (out * to(c["g"])).sum().backward()
    bn = conv.local_nn[1][2]
    res = dict(out=out.detach(), x=x.grad, pos_src_refl=ps.grad[:, 3], running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
               **{k: p.grad.clone() for k, p in conv.named_parameters()})
    return {k: v.cpu() for k, v in res.items()}


def _oracle_layer(c, dtype):
    conv = _ref_style_conv(_OracleMessagePassing, O.scatter_max, _mlp([12, 16, 32], seed=8)).to(dtype)
    return _layer_results(conv, c, "cpu")


def oracle_noise():
    c = _layer_case(O.knn)
    a, b = _oracle_layer(c, torch.float32), _oracle_layer(c, torch.float64)
    return {k: _rel_l2(a[k], b[k]) for k in b}


def test_layer_trains_like_the_oracle_layer(H):
    """Training-mode ops.PointNetConv(local_nn=MLP([8 + 4, 16, 32])) on the edge case of _block_data (1400 points, 350 targets,
    knn k = 16 from the product's own search, handed to both sides) against the reference-style layer over oracle/ops.py in float64
    with training-mode BatchNorm: output, gradient to x and to pos_src[:, 3], every parameter gradient and BatchNorm's running
    statistics, relative L2 <= 8 x the oracle layer's own fp32-against-fp64 noise per tensor (tests/golden/conv_train/noise.json;
    the project's margin for another fixed summation order and a winner switching at a near-tie).  The running statistics move.
    Then one AdamW step: every parameter stays finite and moves."""
    noise = json.load(open(NOISE_JSON))["rel_l2"]
    c = _layer_case(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    ref = _oracle_layer(c, torch.float64)
    nn = _mlp([12, 16, 32], seed=8)
    before_stats = (nn[1][2].running_mean.clone(), nn[1][2].running_var.clone())
    conv = H.PointNetConv(local_nn=nn, global_nn=None, add_self_loops=False).cuda()
    assert list(conv.state_dict()) == ["local_nn." + k for k in nn.state_dict()]
    got = _layer_results(conv, c, "cuda")
    assert set(got) == set(ref) == set(noise)
    errs = {k: _rel_l2(got[k], ref[k]) for k in ref}
    for k in ref:
        print(f"layer {k}: rel L2 {errs[k]:.3e}, noise {noise[k]:.3e}, ratio {errs[k] / noise[k]:.2f}")
    for k in ref:
        assert errs[k] <= 8 * noise[k], (k, errs[k], noise[k])
    assert not torch.equal(got["running_mean"], before_stats[0]) and not torch.equal(got["running_var"], before_stats[1])
    assert got["x"].dtype == torch.float32 and got["x"].shape == c["x"].shape
    before = {k: p.detach().clone() for k, p in conv.named_parameters()}
    opt = torch.optim.AdamW(conv.parameters(), lr=1e-3)
    opt.zero_grad()
    out = conv(c["x"].cuda(), (c["pos_src"].cuda(), c["pos_dst"].cuda()), c["ei"].cuda())
    (out * c["g"].cuda()).sum().backward()
    opt.step()
    for k, p in conv.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert not torch.equal(p.detach(), before[k]), k


def test_training_mode_structural_checks(H):
    c = _layer_case(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    x, pos, ei = c["x"].cuda(), (c["pos_src"].cuda(), c["pos_dst"].cuda()), c["ei"].cuda()
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8)).cuda().train()(x, pos, ei)
    conv = H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), add_self_loops=False).cuda().train()
    with pytest.raises(NotImplementedError, match="x = None"):
        conv(None, pos, ei)
    with pytest.raises(RuntimeError, match=r"pos must be \[n, 4\]"):
        conv(x, (pos[0][:, :3], pos[1][:, :3]), ei)
    with pytest.raises(NotImplementedError, match="MLP"):
        H.PointNetConv(local_nn=_mlp([12, 16, 16, 32], seed=8), add_self_loops=False).cuda().train()(x, pos, ei)
    with pytest.raises(RuntimeError, match="grouped by target"):
        conv(x, pos, ei.flip(1))
    conv.eval()
    conv.local_nn[1][2].train()                  # the fused path still refuses a BatchNorm in training mode
    with pytest.raises(RuntimeError, match="inference-only"):
        conv(x, pos, ei)


# ------------------------------------------------------------------------------------------------ unchanged paths
def test_eval_mode_is_untouched_by_a_round_trip(H):
    """Eval-mode ops.PointNetConv: the same bits before and after a .train() / .eval() round trip, and the same bits as a second
    instance that was never switched; the result carries no graph."""
    c = _layer_case(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    x, pos, ei = c["x"].cuda(), (c["pos_src"].cuda(), c["pos_dst"].cuda()), c["ei"].cuda()
    a = H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), add_self_loops=False).cuda().eval()
    b = H.PointNetConv(local_nn=_mlp([12, 16, 32], seed=8), add_self_loops=False).cuda().eval()
    first = a(x, pos, ei)
    assert not first.requires_grad
    a.train()
    a.eval()
    again, never = a(x, pos, ei), b(x, pos, ei)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    assert torch.equal(first.view(torch.int32), never.view(torch.int32))


def test_edge_layer1_no_grad_and_autocast(H):
    """edge_layer1 under no_grad returns the bits it returns with gradients tracked and builds no graph; under autocast(float16)
    the output is fp32 and the gradients carry their inputs' dtypes (fp16 P, fp32 Wg and pos_src)."""
    c, f = R.edge_case(), R.forward_case(16)
    ei = torch.stack([c["src"].long(), c["i"]], 0).cuda()
    ps, pd = c["pos_src"].cuda(), c["pos_dst"].cuda()
    P, Wg = f["P"].cuda().requires_grad_(), f["Wg"].cuda().requires_grad_()
    tracked = H.edge_layer1(P, Wg, ps, pd, ei)
    assert tracked.grad_fn is not None
    with torch.no_grad():
        plain = H.edge_layer1(P, Wg, ps, pd, ei)
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain.view(torch.int32), tracked.detach().view(torch.int32))
    assert H.edge_layer1(P.detach(), Wg.detach(), ps, pd, ei).grad_fn is None
    assert R.ratio(plain.cpu(), f["H1"], f["cap_H1"]) <= 1.0
    Ph, psg = f["P"].cuda().half().requires_grad_(), ps.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = H.edge_layer1(Ph, Wg, psg, pd, ei)
    assert out.dtype == torch.float32
    out.sum().backward()
    assert Ph.grad.dtype == torch.float16 and Wg.grad.dtype == torch.float32 and psg.grad.dtype == torch.float32
    assert bool((psg.grad[:, :3] == 0).all()) and float(psg.grad[:, 3].abs().max()) > 0
    with pytest.raises(RuntimeError, match="grouped by target"):
        H.edge_layer1(P, Wg, ps, pd, ei.flip(1))


# ------------------------------------------------------------------------------------------------ ABI guards
def test_abi_guards_return_their_codes_and_launch_nothing(L):
    """NULL pointers (-2), a pitch that is no multiple of 4 floats or a pointer off 16 bytes with C1 a multiple of 4 (-3), negative
    sizes, pitches below C1 and edges without targets or sources to hold them (-1), a workspace that is too small (-4): checked
    before anything is launched, so the NaN-filled outputs stay NaN.  Then the good call writes them."""
    ptr, stream = _abi()
    n, M, C1 = 12, 5, 8
    csr = torch.tensor([0, 3, 3, 10, 11, 14], dtype=torch.int32, device="cuda")
    E = 14
    src = (torch.arange(E, dtype=torch.int32) % n).cuda()
    P, Wg = torch.randn(n + 1, C1, device="cuda"), torch.randn(5, C1, device="cuda")
    rs, rd = torch.rand(n + 1, 4, device="cuda"), torch.rand(M + 1, 4, device="cuda")
    geo = torch.full((E + 1, 4), float("nan"), device="cuda")
    H1 = torch.full((E + 1, C1 + 4), float("nan"), device="cuda")
    s = stream()

    def fwd(P_=ptr(P), ldp=C1, rs_=ptr(rs), rd_=ptr(rd), csr_=ptr(csr), src_=ptr(src), Wg_=ptr(Wg), n_=n, M_=M, E_=E, C1_=C1, geo_=ptr(geo),
            H1_=ptr(H1), ldh=C1):
        return L.p2w_edge_l1(P_, ldp, rs_, rd_, csr_, src_, Wg_, n_, M_, E_, C1_, geo_, H1_, ldh, s)

    for name in ("P_", "rs_", "rd_", "csr_", "src_", "Wg_", "geo_", "H1_"):
        assert fwd(**{name: None}) == ENULL, name
    assert fwd(ldp=C1 + 2) == EALIGN and fwd(ldh=C1 + 1) == EALIGN
    assert fwd(P_=ptr(P) + 4, ldp=C1) == EALIGN and fwd(H1_=ptr(H1) + 4) == EALIGN and fwd(Wg_=ptr(Wg) + 4) == EALIGN
    assert fwd(rs_=ptr(rs) + 4) == EALIGN and fwd(rd_=ptr(rd) + 8) == EALIGN and fwd(geo_=ptr(geo) + 4) == EALIGN
    assert fwd(ldp=C1 - 4) == EINVAL and fwd(ldh=4) == EINVAL and fwd(C1_=0) == EINVAL
    assert fwd(n_=-1) == EINVAL and fwd(M_=-1) == EINVAL and fwd(E_=-1) == EINVAL
    assert fwd(M_=0) == EINVAL and fwd(n_=0) == EINVAL                   # E edges that ptr / the sources cannot hold
    assert fwd(M_=0, E_=0) == 0 and fwd(E_=0) == 0                       # nothing to do: nothing launched
    gH = torch.randn(E + 1, C1, device="cuda")
    gP = torch.full((n + 1, C1 + 4), float("nan"), device="cuda")
    gR, gWg = torch.full((n + 1,), float("nan"), device="cuda"), torch.full((5, C1), float("nan"), device="cuda")
    Hs, gs = torch.randn(E + 1, C1, device="cuda"), torch.rand(E + 1, 4, device="cuda")
    need = int(L.p2w_edge_l1_bwd_ws_bytes(E, n, C1))
    assert need > 0 and need % 256 == 0
    assert L.p2w_edge_l1_bwd_ws_bytes(-1, n, C1) == 0 and L.p2w_edge_l1_bwd_ws_bytes(E, -1, C1) == 0 and L.p2w_edge_l1_bwd_ws_bytes(E, n, 0) == 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")

    def bwd(gH_=ptr(gH), ldg=C1, H1_=ptr(Hs), ldh=C1, geo_=ptr(gs), src_=ptr(src), Wg_=ptr(Wg), n_=n, E_=E, C1_=C1, gP_=ptr(gP), ldgp=C1,
            gR_=ptr(gR), gWg_=ptr(gWg), ws_=ptr(ws), wsb=need):
        return L.p2w_edge_l1_bwd(gH_, ldg, H1_, ldh, geo_, src_, Wg_, n_, E_, C1_, gP_, ldgp, gR_, gWg_, ws_, wsb, s)

    for name in ("gH_", "H1_", "geo_", "src_", "Wg_", "gP_", "gR_", "gWg_", "ws_"):
        assert bwd(**{name: None}) == ENULL, name
    assert bwd(ldg=C1 + 2) == EALIGN and bwd(ldh=C1 + 1) == EALIGN and bwd(ldgp=C1 + 3) == EALIGN
    assert bwd(gH_=ptr(gH) + 4) == EALIGN and bwd(H1_=ptr(Hs) + 4) == EALIGN and bwd(gP_=ptr(gP) + 4) == EALIGN
    assert bwd(gWg_=ptr(gWg) + 4) == EALIGN and bwd(geo_=ptr(gs) + 4) == EALIGN and bwd(ws_=ptr(ws) + 4) == EALIGN
    assert bwd(ldg=4) == EINVAL and bwd(ldh=C1 - 4) == EINVAL and bwd(ldgp=4) == EINVAL and bwd(C1_=0) == EINVAL
    assert bwd(n_=-1) == EINVAL and bwd(E_=-1) == EINVAL and bwd(n_=0) == EINVAL
    assert bwd(wsb=need - 1) == EWORKSPACE and bwd(wsb=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(geo).all()) and bool(torch.isnan(H1).all())
    assert bool(torch.isnan(gP).all()) and bool(torch.isnan(gR).all()) and bool(torch.isnan(gWg).all())
    assert fwd() == 0 and bwd(ldgp=C1 + 4) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(geo[:E]).all()) and bool(torch.isfinite(H1.view(-1)[:E * C1]).all()) and bool(torch.isnan(geo[E]).all())
    assert bool(torch.isfinite(gP[:n, :C1]).all()) and bool(torch.isnan(gP[:, C1:]).all()) and bool(torch.isnan(gP[n]).all())
    assert bool(torch.isfinite(gR[:n]).all()) and bool(torch.isnan(gR[n])) and bool(torch.isfinite(gWg[:4]).all()) and bool(torch.isnan(gWg[4]).all())


if __name__ == "__main__":
    os.makedirs(os.path.dirname(NOISE_JSON), exist_ok=True)
    with open(NOISE_JSON, "w") as f:
        json.dump({"what": "relative L2 error per compared tensor of the oracle PointNetConv layer (training-mode BatchNorm), fp32 against "
                           "fp64, CPU", "rel_l2": oracle_noise()}, f, indent=1)
        f.write("\n")
    print(open(NOISE_JSON).read())
