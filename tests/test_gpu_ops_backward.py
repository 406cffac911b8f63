"""Backward passes of the operator route (ops.global_max_pool / scatter_max / MessagePassing.propagate / knn_interpolate,
csrc/p2w_grad.hip) against oracle/ops.py on the CPU in float64 under ordinary autograd.

``python -m tests.test_gpu_ops_backward`` (no GPU needed) rewrites tests/golden/ops_backward/noise.json: the rounding noise of
the oracle block of ``test_training_step_of_a_reference_shaped_block`` in fp32 against itself in fp64."""
import copy
import json
import os

import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu

NOISE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_backward", "noise.json")
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def H():
    from pointstowood_amd import ops
    return ops


@pytest.fixture(scope="module")
def L():
    from pointstowood_amd._lib import lib
    return lib()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ptr_of(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(sizes).cumsum(0)]).to(torch.int32)


# ------------------------------------------------------------------------------------------------ segment max
FEW = [0, 1, 63, 64, 65, 1000, 0, 3]                       # p2w_segment_max + the arg pass (few segments, rows split over blocks)
MANY = [(i * 7) % 41 for i in range(700)]                  # the one-pass kernel (one block per segment), empty segments included
SEGMENTS = {"few": FEW, "many": MANY}
_segcache = {}


def _segment_case(layout, F):
    """(x with distinct values, batch, B, upstream gradient, fp64 gradient of the oracle, reference arg): computed once per case."""
    key = (layout, F)
    if key not in _segcache:
        sizes = SEGMENTS[layout]
        n, B = sum(sizes), len(sizes)
        x = (torch.randperm(n * F, generator=_gen(11 + F)).float() - float(n * F // 2)).reshape(n, F)
        batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
        g = torch.randn(B, F, generator=_gen(12 + F))
        x64 = x.double().requires_grad_()
        O.segment_max_rows(x64, batch, B).backward(g.double())
        arg = torch.full((B, F), -1, dtype=torch.int32)
        s = 0
        for b, k in enumerate(sizes):
            if k:
                arg[b] = (x[s:s + k].argmax(0) + s).int()
            s += k
        _segcache[key] = (x, batch, B, g, x64.grad, arg)
    return _segcache[key]


SEG_CASES = [("few", F) for F in (1, 7, 64, 130)] + [("many", F) for F in (7, 64)]


@pytest.mark.parametrize("layout,F", SEG_CASES)
def test_segment_max_values_and_arg(H, L, layout, F):
    """With requires_grad the output is today's output bit for bit (p2w_segment_max through the ABI), and arg is the argmax per
    segment and column (-1 and 0 for an empty segment)."""
    from pointstowood_amd._lib import ptr, stream
    x, batch, B, _, _, arg_ref = _segment_case(layout, F)
    dx, ptr_d = x.cuda(), _ptr_of(SEGMENTS[layout]).cuda()
    today = torch.empty((B, F), dtype=torch.float32, device="cuda")
    assert L.p2w_segment_max(ptr(dx), F, F, ptr(ptr_d), B, ptr(today), stream()) == 0
    got = H.global_max_pool(dx.clone().requires_grad_(), batch.cuda(), size=B)
    assert got.grad_fn is not None
    assert torch.equal(got.detach().view(torch.int32), today.view(torch.int32))
    out = torch.full((B, F), float("nan"), device="cuda")
    arg = torch.full((B, F), -7, dtype=torch.int32, device="cuda")
    assert L.p2w_segment_max_arg(ptr(dx), F, F, ptr(ptr_d), B, ptr(out), ptr(arg), stream()) == 0
    assert torch.equal(out.view(torch.int32), today.view(torch.int32))
    assert torch.equal(arg.cpu(), arg_ref)
    assert torch.equal(today.cpu(), O.segment_max_rows(x, batch, B))


@pytest.mark.parametrize("layout,F", SEG_CASES)
def test_segment_max_gradient_is_a_copy(H, L, layout, F):
    """grad_x == the fp64 autograd gradient of oracle.ops.segment_max_rows exactly (no ties: a copy of grad_out at the winners,
    0 elsewhere), through the operator and through the ABI into a NaN-filled buffer with three rows past ptr[B]."""
    from pointstowood_amd._lib import ptr, stream
    x, batch, B, g, ref, arg_ref = _segment_case(layout, F)
    dx = x.cuda().requires_grad_()
    H.global_max_pool(dx, batch.cuda(), size=B).backward(g.cuda())
    assert dx.grad.shape == x.shape and dx.grad.dtype == torch.float32
    assert torch.equal(dx.grad.cpu().double(), ref)
    n = x.shape[0]
    winners = torch.zeros(n, F, dtype=torch.bool)
    cols = torch.arange(F)[None, :].expand(B, F)
    winners[arg_ref[arg_ref >= 0].long(), cols[arg_ref >= 0]] = True
    assert bool((dx.grad.cpu()[~winners] == 0).all())
    # scatter_max: the same through the edge signature, with a 3-d src
    if F % 2 == 0:
        sx = x.reshape(n, 2, F // 2).cuda().requires_grad_()
        res, none = H.scatter_max(sx, batch.cuda(), dim=0, dim_size=B)
        assert none is None and res.shape == (B, 2, F // 2)
        res.backward(g.reshape(B, 2, F // 2).cuda())
        assert torch.equal(sx.grad.cpu().double().reshape(n, F), ref)
    # the ABI alone: every element of grad_x[0..n + 3) is written
    buf = torch.full((n + 3, F), float("nan"), device="cuda")
    dg, darg, dptr = g.cuda(), arg_ref.cuda(), _ptr_of(SEGMENTS[layout]).cuda()
    assert L.p2w_segment_max_bwd(ptr(dg), F, ptr(darg), ptr(dptr), B, F, ptr(buf), F, n + 3, stream()) == 0
    assert torch.equal(buf[:n].cpu().double(), ref)
    assert bool((buf[n:] == 0).all())


@pytest.mark.parametrize("nseg,F", [(1, 12), (1, 7), (300, 12), (300, 7)])
def test_segment_max_ties_go_to_the_lowest_row(H, nseg, F):
    """Rows 5, 40 and 69 of a 70-row segment hold the maximum of every column: all of the gradient lands in row 5 and the column
    sums of grad_x equal grad_out (one segment: the split path; 300 segments: the one-pass kernel)."""
    x = torch.randn(nseg, 70, F, generator=_gen(3))
    x[:, [5, 40, 69]] = 100.0
    g = torch.randn(nseg, F, generator=_gen(4))
    dx = x.reshape(nseg * 70, F).cuda().requires_grad_()
    batch = torch.repeat_interleave(torch.arange(nseg), 70).cuda()
    H.global_max_pool(dx, batch, size=nseg).backward(g.cuda())
    gx = dx.grad.cpu().reshape(nseg, 70, F)
    assert torch.equal(gx[:, 5], g)
    assert torch.equal(gx.sum(1), g)
    gx[:, 5] = 0
    assert bool((gx == 0).all())


# ------------------------------------------------------------------------------------------------ the edge form
def _mlp(dims, seed, bn_stats=True):
    """MLP(dims) as the reference builds it (model.py:198-202): Lin + ReLU per layer, BatchNorm after the last."""
    from torch.nn import BatchNorm1d as BN, Linear as Lin, ReLU, Sequential as Seq
    torch.manual_seed(seed)
    layers = [Seq(Lin(a, b), ReLU()) for a, b in zip(dims[:-2], dims[1:-1])]
    layers.append(Seq(Lin(dims[-2], dims[-1]), ReLU(), BN(dims[-1])))
    nn = Seq(*layers)
    if bn_stats:
        bn = nn[-1][2]
        with torch.no_grad():
            bn.weight.copy_(torch.randn(dims[-1])); bn.bias.copy_(torch.randn(dims[-1]) * 0.3)
            bn.running_mean.copy_(torch.randn(dims[-1]) * 0.2); bn.running_var.copy_(torch.rand(dims[-1]) + 0.5)
    return nn


class _OracleMessagePassing(torch.nn.Module):
    """propagate of the reference's conv over oracle.ops: gather, message, segment_max_rows."""

    def __init__(self, aggr="max"):
        super().__init__()

    def propagate(self, edge_index, x, pos):
        j, i = edge_index[0], edge_index[1]
        return O.segment_max_rows(self.message(x[0][j], pos[1][i], pos[0][j], i), i, pos[1].shape[0])


def _ref_style_conv(base, scatter_max, local_nn):
    """A PointNetConv written like the reference's (pointnet.py:19-132) over the given MessagePassing base."""

    class RefStyleConv(base):
        def __init__(self, local_nn):
            super().__init__(aggr="max")
            self.local_nn = local_nn

        def forward(self, x, pos, edge_index):
            return self.propagate(edge_index, x=(x, None), pos=pos)

        def message(self, x_j, pos_i, pos_j, edge_index_i):
            msg = torch.zeros((pos_j.size(0), pos_j.size(1)), device=pos_j.device, dtype=pos_j.dtype)
            relative_pos = pos_j[:, :3] - pos_i[:, :3]
            max_distances, _ = scatter_max(torch.norm(relative_pos, dim=1, keepdim=True), edge_index_i, dim=0)
            msg[:, :3] = relative_pos / (max_distances[edge_index_i] + 1e-8)
            msg[:, 3] = pos_j[:, 3]
            return self.local_nn(torch.cat([x_j, msg], dim=1))

    return RefStyleConv(local_nn)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


_edgecache = {}


def _edge_case():
    """500 targets with degrees 0..32 (targets 0, 7, 8, 250 and 499 and whatever the draw gives have none), 800 sources,
    local_nn = MLP([8 + 4, 16, 128]) in eval mode; the fp64 gradients of sum(out * g) over oracle.ops."""
    if not _edgecache:
        gen = _gen(21)
        deg = torch.randint(0, 33, (500,), generator=gen)
        deg[[0, 7, 8, 250, 499]] = 0
        deg[3] = 32
        i = torch.repeat_interleave(torch.arange(500), deg)
        j = torch.randint(0, 800, (i.numel(),), generator=gen)
        ei = torch.stack([j, i], 0)
        x = torch.randn(800, 8, generator=gen)
        pos_src, pos_dst = torch.rand(800, 4, generator=gen), torch.rand(500, 4, generator=gen)
        g = torch.randn(500, 128, generator=gen)
        nn = _mlp([12, 16, 128], seed=5).eval()
        conv = _ref_style_conv(_OracleMessagePassing, O.scatter_max, copy.deepcopy(nn)).double().eval()
        x64 = x.double().requires_grad_()
        out = conv(x64, (pos_src.double(), pos_dst.double()), ei)
        (out * g.double()).sum().backward()
        grads = {"x": x64.grad, **{k: p.grad for k, p in conv.named_parameters()}}
        _edgecache.update(ei=ei, x=x, pos_src=pos_src, pos_dst=pos_dst, g=g, nn=nn, out=out.detach(), grads=grads, deg=deg)
    return _edgecache


def _edge_backward(H, c):
    conv = _ref_style_conv(H.MessagePassing, H.scatter_max, copy.deepcopy(c["nn"])).cuda().eval()
    x = c["x"].cuda().requires_grad_()
    out = conv(x, (c["pos_src"].cuda(), c["pos_dst"].cuda()), c["ei"].cuda())
    (out * c["g"].cuda()).sum().backward()
    return out.detach(), {"x": x.grad, **{k: p.grad for k, p in conv.named_parameters()}}


def test_edge_form_through_message_passing_propagate(H):
    """scatter_max under MessagePassing.propagate (a reference-style subclass): gradients with respect to x and to the local_nn
    parameters against the same composition over oracle.ops in fp64.

    Bound: relative L2 error 1e-4 per tensor.  Everything but the aggregation is fp32 PyTorch on both sides of the max (two
    Linear layers of 12 and 16 inputs, a per-column sum over about 8000 edges for the parameter gradients), the aggregation's
    gradient itself is a copy: sqrt(8000) 2^-23 = 1e-5 of accumulated rounding, times a handful of layers, rounded up to the
    next decade.  Exact ties of the max are ReLU zeros, whose gradient is 0 under either tie rule."""
    c = _edge_case()
    out, grads = _edge_backward(H, c)
    assert (out.cpu().double() - c["out"]).abs().max() <= 2e-5 * float(c["out"].abs().max())
    assert bool((out[c["deg"] == 0] == 0).all())
    assert set(grads) == set(c["grads"])
    for k, ref in c["grads"].items():
        err = _rel_l2(grads[k].cpu(), ref)
        print(f"edge form {k}: rel L2 {err:.3e}")
        assert err <= 1e-4, (k, err)


# ------------------------------------------------------------------------------------------------ interpolation
INTERP_SHAPES = [(300, 2000, 2, 64), (300, 2000, 3, 7), (50, 700, 1, 24), (1, 5000, 2, 130), (400, 100, 2, 16), "batch"]
_interpcache = {}


def _interp_case(shape):
    """Inputs, the fp64 gradient of oracle.ops.knn_interpolate and the element-wise bound (L_j + 8) 2^-23 sum |a| |g| over row j's
    run, both from the oracle's own neighbour table (the product's table equals it bit for bit: test_gpu_ops.py)."""
    if shape not in _interpcache:
        gen = _gen(31)
        if shape == "batch":     # two voxels; the coarse points are fine points, so some fine points coincide with a coarse one
            k, F = 2, 20
            pos_f = torch.rand(900, 3, generator=gen)
            bf = torch.repeat_interleave(torch.arange(2), torch.tensor([700, 200]))
            idx = torch.cat([torch.arange(0, 700, 9), torch.arange(700, 900, 7)])
            pos_c, bc = pos_f[idx].clone(), bf[idx]
        else:
            nc, m, k, F = shape
            pos_c, pos_f, bc, bf = torch.rand(nc, 3, generator=gen), torch.rand(m, 3, generator=gen), None, None
        nc, m = pos_c.shape[0], pos_f.shape[0]
        x = torch.randn(nc, F, generator=gen)
        g = torch.randn(m, F, generator=gen)
        x64 = x.double().requires_grad_()
        O.knn_interpolate(x64, pos_c.double(), pos_f.double(), bc, bf, k=k).backward(g.double())
        q, j = O.knn(pos_c, pos_f, k, bc, bf)
        d2 = ((pos_c.double()[j] - pos_f.double()[q]) ** 2).sum(1)
        w = 1.0 / d2.clamp(min=1e-16)
        a = w / torch.zeros(m, dtype=torch.float64).index_add_(0, q, w)[q]
        run = torch.bincount(j, minlength=nc)
        bound = torch.zeros(nc, F, dtype=torch.float64).index_add_(0, j, a[:, None] * g.double().abs()[q])
        bound = (run[:, None] + 8).double() * EPS * bound
        _interpcache[shape] = dict(x=x, g=g, pos_c=pos_c, pos_f=pos_f, bc=bc, bf=bf, k=k, ref=x64.grad, bound=bound, run=run,
                                   coincide=int((d2 == 0).sum()))
    return _interpcache[shape]


def _interp_backward(H, c):
    cu = lambda t: None if t is None else t.cuda()
    x = c["x"].cuda().requires_grad_()
    out = H.knn_interpolate(x, cu(c["pos_c"]), cu(c["pos_f"]), cu(c["bc"]), cu(c["bf"]), k=c["k"])
    out.backward(c["g"].cuda())
    return x.grad


@pytest.mark.parametrize("shape", INTERP_SHAPES, ids=str)
def test_interpolation_gradient_within_the_derived_bound(H, shape):
    """|grad_x - fp64| <= (L_j + 8) 2^-23 sum |a| |g| per element: L_j fp32 additions of the run's products (one rounding each,
    plus the product's), 8 for the fp32 weights; rows nobody references are exactly 0."""
    c = _interp_case(shape)
    if shape == "batch":
        assert c["coincide"] > 100      # the d2 clamp is exercised
    gx = _interp_backward(H, c)
    assert gx.shape == c["x"].shape and gx.dtype == torch.float32
    err = (gx.cpu().double() - c["ref"]).abs()
    print(f"interp {shape}: max err / bound {float((err / c['bound'].clamp(min=1e-300)).max()):.3f}, longest run {int(c['run'].max())}")
    assert bool((err <= c["bound"]).all())
    assert bool((gx.cpu()[c["run"] == 0] == 0).all())
    if shape == (400, 100, 2, 16):
        assert int((c["run"] == 0).sum()) > 200


# ------------------------------------------------------------------------------------------------ determinism
def test_backward_is_bit_reproducible(H):
    """The (1, 5000, 2, 130) interpolation (one run of 5000 slots, split over blocks) and the edge form, twice, and once more
    with an unrelated allocation in between (another workspace address): all bit-equal."""
    ci, ce = _interp_case((1, 5000, 2, 130)), _edge_case()
    runs = []
    keep = []
    for rep in range(3):
        if rep == 2:
            keep.append(torch.empty(3 * 1024 * 1024 + 17, dtype=torch.uint8, device="cuda"))
        gi = _interp_backward(H, ci)
        _, ge = _edge_backward(H, ce)
        runs.append([gi.clone()] + [ge[k].clone() for k in sorted(ge)])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ no change without grad
def test_forward_bits_do_not_depend_on_grad_mode(H, L):
    """Per operator: the output under no_grad == the parent's code path (p2w_segment_max / p2w_interp_concat through the ABI) ==
    the output with requires_grad."""
    from pointstowood_amd._lib import ptr, stream
    bits = lambda t: t.detach().contiguous().view(torch.int32)
    # global_max_pool / scatter_max
    x, batch, B, _, _, _ = _segment_case("few", 64)
    dx, db, dptr = x.cuda(), batch.cuda(), _ptr_of(FEW).cuda()
    parent = torch.empty((B, 64), dtype=torch.float32, device="cuda")
    assert L.p2w_segment_max(ptr(dx), 64, 64, ptr(dptr), B, ptr(parent), stream()) == 0
    with torch.no_grad():
        a = H.global_max_pool(dx.clone().requires_grad_(), db, size=B)
        sa = H.scatter_max(dx, db, dim=0, dim_size=B)[0]
    assert a.grad_fn is None and not a.requires_grad
    b = H.global_max_pool(dx.clone().requires_grad_(), db, size=B)
    sb = H.scatter_max(dx.clone().requires_grad_(), db, dim=0, dim_size=B)[0]
    for t in (a, sa, b, sb):
        assert torch.equal(bits(t), bits(parent))
    # knn_interpolate (F = 7: the padded path)
    c = _interp_case((300, 2000, 3, 7))
    dxc, pc, pf = c["x"].cuda(), c["pos_c"].cuda(), c["pos_f"].cuda()
    nbr, deg = H._search("knn", pc, pf, None, None, None, 3)
    xc = torch.nn.functional.pad(dxc, (0, 1)).contiguous()
    rc, rf = H._xyzr(pc), H._xyzr(pf)
    parent = torch.empty((2000, 8), dtype=torch.float32, device="cuda")
    assert L.p2w_interp_concat(ptr(xc), 8, ptr(rc), ptr(rf), ptr(nbr), ptr(deg), 3, None, 0, 2000, ptr(parent), 8, stream()) == 0
    with torch.no_grad():
        a = H.knn_interpolate(dxc.clone().requires_grad_(), pc, pf, k=3)
    b = H.knn_interpolate(dxc.clone().requires_grad_(), pc, pf, k=3)
    assert a.grad_fn is None and b.grad_fn is not None
    assert torch.equal(bits(a), bits(parent[:, :7])) and torch.equal(bits(b), bits(parent[:, :7]))


def test_backward_under_autocast_returns_the_inputs_dtype(H):
    """Under torch.autocast('cuda', float16) with fp16 input the operators compute in fp32, the backward runs and the gradient
    comes back in fp16 with the input's shape; a non-contiguous input gets a gradient of its own shape too."""
    x, batch, B, g, ref, _ = _segment_case("few", 64)
    c = _interp_case((50, 700, 1, 24))
    hx = x.cuda().half().requires_grad_()
    hc = c["x"].cuda().half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        o1 = H.global_max_pool(hx, batch.cuda(), size=B)
        o2 = H.knn_interpolate(hc, c["pos_c"].cuda(), c["pos_f"].cuda(), k=1)
        assert o1.dtype == torch.float32 and o2.dtype == torch.float32
        (o1 * g.cuda()).sum().backward()
        (o2 * c["g"].cuda()).sum().backward()
    assert hx.grad.dtype == torch.float16 and hx.grad.shape == hx.shape
    assert hc.grad.dtype == torch.float16 and hc.grad.shape == hc.shape
    assert bool(torch.isfinite(hx.grad).all()) and bool(((hx.grad != 0).sum(0) == sum(k > 0 for k in FEW)).all())   # one winner per segment
    assert bool(torch.isfinite(hc.grad).all()) and float(hc.grad.abs().sum()) > 0
    wide = torch.randn(x.shape[0], 2 * 64, generator=_gen(5)).cuda().requires_grad_()
    H.global_max_pool(wide[:, ::2], batch.cuda(), size=B).sum().backward()
    assert wide.grad.shape == wide.shape and bool((wide.grad[:, 1::2] == 0).all())
    assert torch.equal(wide.grad[:, ::2].sum(0), (torch.tensor(FEW) > 0).sum().float().cuda().expand(64))


# ------------------------------------------------------------------------------------------------ one training step
class _Block(torch.nn.Module):
    """A reference-shaped block: conv (MLP([F + 4, 16, 32]) with BatchNorm, max over knn edges) -> small MLP -> global_max_pool ->
    knn_interpolate(k = 2) back to the input points -> linear head.  ``ops`` supplies the three operators."""

    def __init__(self, ops, F=8):
        super().__init__()
        torch.manual_seed(17)
        self.conv = _ref_style_conv(ops["base"], ops["scatter_max"], _mlp([F + 4, 16, 32], seed=17, bn_stats=False))
        self.glob = torch.nn.Sequential(torch.nn.Linear(32, 24), torch.nn.ReLU())
        self.head = torch.nn.Linear(32 + 24, 1)
        self.ops = ops

    def forward(self, d):
        h = self.conv(d["x"], (d["pos4"], d["pos4"][d["idx"]]), d["ei"])
        bc = d["batch"][d["idx"]]
        pooled = self.ops["global_max_pool"](self.glob(h), bc)
        coarse = torch.cat([h, pooled[bc]], 1)
        fine = self.ops["knn_interpolate"](coarse, d["pos4"][d["idx"], :3], d["pos4"][:, :3], bc, d["batch"], k=2)
        return torch.nn.functional.binary_cross_entropy_with_logits(self.head(fine)[:, 0], d["label"])


ORACLE_OPS = dict(base=_OracleMessagePassing, scatter_max=O.scatter_max, global_max_pool=O.global_max_pool,
                  knn_interpolate=O.knn_interpolate)


def _block_data(knn):
    """Two voxels of 1200 and 200 points, a seeded sample of a quarter of each (ascending, as random_sample's result is used),
    knn(k = 16) edges from the given search."""
    gen = _gen(41)
    sizes = [1200, 200]
    n = sum(sizes)
    batch = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes))
    pos4 = torch.rand(n, 4, generator=gen)
    x = torch.randn(n, 8, generator=gen)
    label = (torch.rand(n, generator=gen) < 0.4).float()
    idx = torch.cat([torch.randperm(1200, generator=gen)[:300].sort().values, 1200 + torch.randperm(200, generator=gen)[:50].sort().values])
    row, col = knn(pos4[:, :3], pos4[idx, :3], 16, batch, batch[idx])
    return dict(x=x, pos4=pos4, batch=batch, idx=idx, label=label, ei=torch.stack([col, row], 0))


def _block_grads(block, d):
    block.train()
    block.zero_grad()
    block(d).backward()
    return {k: p.grad.detach().clone() for k, p in block.named_parameters()}


def _oracle_block_grads(d, dtype):
    to = lambda t: t.to(dtype) if t.is_floating_point() else t
    return _block_grads(_Block(ORACLE_OPS).to(dtype), {k: to(v) for k, v in d.items()})


def oracle_noise():
    """Per parameter tensor: relative L2 error of the oracle block's gradients in fp32 against fp64, both on the CPU."""
    d = _block_data(O.knn)
    g32, g64 = _oracle_block_grads(d, torch.float32), _oracle_block_grads(d, torch.float64)
    return {k: _rel_l2(g32[k], g64[k]) for k in g64}


def test_training_step_of_a_reference_shaped_block(H):
    """Every parameter's gradient of the block over the product's operators (training-mode BatchNorm, fp32 on the GPU) against
    the same block over oracle.ops in fp64 on the CPU, same edges (the product's knn, handed to both) and same sample: relative
    L2 error per tensor <= 8 x the oracle's own fp32-against-fp64 noise (tests/golden/ops_backward/noise.json; the factor covers
    another, fixed summation order and one winner switching at a near-tie).  Then one AdamW step: all parameters stay finite
    and all of them move."""
    noise = json.load(open(NOISE_JSON))["rel_l2"]
    d = _block_data(lambda *a: H.knn(*[t.cuda() if torch.is_tensor(t) else t for t in a]).cpu())
    ref = _oracle_block_grads(d, torch.float64)
    block = _Block(dict(base=H.MessagePassing, scatter_max=H.scatter_max, global_max_pool=H.global_max_pool,
                        knn_interpolate=H.knn_interpolate)).cuda()
    dd = {k: v.cuda() for k, v in d.items()}
    got = _block_grads(block, dd)
    assert set(got) == set(ref) == set(noise)
    errs = {k: _rel_l2(got[k].cpu(), ref[k]) for k in ref}
    for k in ref:
        print(f"block {k}: rel L2 {errs[k]:.3e}, noise {noise[k]:.3e}, ratio {errs[k] / noise[k]:.2f}")
    for k in ref:
        assert errs[k] <= 8 * noise[k], (k, errs[k], noise[k])
    before = {k: p.detach().clone() for k, p in block.named_parameters()}
    opt = torch.optim.AdamW(block.parameters(), lr=1e-3)
    opt.zero_grad()
    block(dd).backward()
    opt.step()
    for k, p in block.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert not torch.equal(p.detach(), before[k]), k


# ------------------------------------------------------------------------------------------------ ABI guards
def test_abi_guards_return_their_codes_and_launch_nothing(L):
    """NULL pointers (-2), misaligned pointers (-3), row pitches that are no multiple of 4 floats and kw outside 1..100 (-1), a
    workspace that is too small (-4): checked before anything is launched, so the NaN-filled outputs stay NaN."""
    from pointstowood_amd._lib import ptr, stream
    EINVAL, ENULL, EALIGN, EWORKSPACE = -1, -2, -3, -4
    n, B, F = 40, 2, 8
    x = torch.randn(n, F, device="cuda")
    csr = torch.tensor([0, 25, 40], dtype=torch.int32, device="cuda")
    out = torch.full((B, F), float("nan"), device="cuda")
    arg = torch.full((B, F), -7, dtype=torch.int32, device="cuda")
    gx = torch.full((n, F), float("nan"), device="cuda")
    s = stream()
    assert L.p2w_segment_max_arg(None, F, F, ptr(csr), B, ptr(out), ptr(arg), s) == ENULL
    assert L.p2w_segment_max_arg(ptr(x), F, F, None, B, ptr(out), ptr(arg), s) == ENULL
    assert L.p2w_segment_max_arg(ptr(x), F, F, ptr(csr), B, None, ptr(arg), s) == ENULL
    assert L.p2w_segment_max_arg(ptr(x), F, F, ptr(csr), B, ptr(out), None, s) == ENULL
    assert L.p2w_segment_max_arg(ptr(x), F - 1, F, ptr(csr), B, ptr(out), ptr(arg), s) == EINVAL
    assert L.p2w_segment_max_arg(ptr(x), F, 0, ptr(csr), B, ptr(out), ptr(arg), s) == EINVAL
    assert L.p2w_segment_max_arg(ptr(x), F, F, ptr(csr), 0, ptr(out), ptr(arg), s) == EINVAL
    g = torch.randn(B, F, device="cuda")
    assert L.p2w_segment_max_bwd(None, F, ptr(arg), ptr(csr), B, F, ptr(gx), F, n, s) == ENULL
    assert L.p2w_segment_max_bwd(ptr(g), F, None, ptr(csr), B, F, ptr(gx), F, n, s) == ENULL
    assert L.p2w_segment_max_bwd(ptr(g), F, ptr(arg), None, B, F, ptr(gx), F, n, s) == ENULL
    assert L.p2w_segment_max_bwd(ptr(g), F, ptr(arg), ptr(csr), B, F, None, F, n, s) == ENULL
    assert L.p2w_segment_max_bwd(ptr(g), F - 1, ptr(arg), ptr(csr), B, F, ptr(gx), F, n, s) == EINVAL
    assert L.p2w_segment_max_bwd(ptr(g), F, ptr(arg), ptr(csr), B, F, ptr(gx), F - 1, n, s) == EINVAL
    assert L.p2w_segment_max_bwd(ptr(g), F, ptr(arg), ptr(csr), B, F, ptr(gx), F, -1, s) == EINVAL
    # interpolation
    m, nc, kw = 30, 10, 2
    rc, rf = torch.rand(nc, 4, device="cuda"), torch.rand(m, 4, device="cuda")
    nbr = torch.zeros((m, kw), dtype=torch.int32, device="cuda")
    deg = torch.ones(m, dtype=torch.int32, device="cuda")
    go = torch.randn(m + 1, F, device="cuda")
    gc = torch.full((nc + 1, F), float("nan"), device="cuda")
    need = int(L.p2w_interp_bwd_ws_bytes(m, kw, nc))
    assert need > 0 and L.p2w_interp_bwd_ws_bytes(m, 0, nc) == 0 and L.p2w_interp_bwd_ws_bytes(m, 101, nc) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda go_=ptr(go), ldg=F, F_=F, rc_=ptr(rc), rf_=ptr(rf), nbr_=ptr(nbr), deg_=ptr(deg), kw_=kw, gc_=ptr(gc), ldx=F, \
        ws_=ptr(ws), wsb=need: L.p2w_interp_bwd(go_, ldg, F_, rc_, rf_, nbr_, deg_, kw_, m, nc, gc_, ldx, ws_, wsb, s)
    for name in ("go_", "rc_", "rf_", "nbr_", "deg_", "gc_", "ws_"):
        assert call(**{name: None}) == ENULL, name
    assert call(go_=ptr(go) + 4) == EALIGN and call(gc_=ptr(gc) + 4) == EALIGN and call(rc_=ptr(rc) + 4) == EALIGN
    assert call(rf_=ptr(rf) + 8) == EALIGN and call(ws_=ptr(ws) + 4) == EALIGN
    assert call(ldg=F + 2) == EINVAL and call(ldx=F + 1) == EINVAL and call(F_=6) == EINVAL and call(ldg=4) == EINVAL
    assert call(kw_=0) == EINVAL and call(kw_=101) == EINVAL
    assert call(wsb=need - 1) == EWORKSPACE and call(wsb=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((arg == -7).all()) and bool(torch.isnan(gx).all()) and bool(torch.isnan(gc).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gc[:nc]).all()) and bool((gc[1:nc] == 0).all()) and bool(torch.isnan(gc[nc]).all())


if __name__ == "__main__":
    os.makedirs(os.path.dirname(NOISE_JSON), exist_ok=True)
    with open(NOISE_JSON, "w") as f:
        json.dump({"what": "relative L2 error per parameter tensor of the oracle block's gradients, fp32 against fp64, CPU",
                   "rel_l2": oracle_noise()}, f, indent=1)
        f.write("\n")
    print(open(NOISE_JSON).read())
