"""The eight third-party operators of the reference forward, HIP-backed, with the call
signatures used at the reference's call sites (so its ``src/model.py`` could run over this
module instead of torch-geometric / torch-cluster / torch-scatter):

    voxel_grid(pos, size, batch)                       model.py:104
    consecutive_cluster(src) -> (inv, perm)            model.py:105
    radius(x, y, r, batch_x, batch_y, max_num_neighbors)   model.py:118
    knn(x, y, k, batch_x, batch_y)                     model.py:120
    scatter_max(src, index, dim=0)                     pointnet.py:122
    global_max_pool(x, batch)                          model.py:136
    knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k)  model.py:149
    MessagePassing.propagate(edge_index, x=, pos=)  (aggr=max)   pointnet.py:108 -> ``MessagePassing`` below
    PointNetConv(local_nn, ...)(x, (pos, pos[idx]), edge_index)   pointnet.py:19-132, called at model.py:123 (fused kernel)

Every function requires CUDA (MI355X) tensors and libp2w_gfx950.so; there is no fallback.
Index results are int64 like the reference's; the kernels work in int32 internally.
``Net.forward`` does not go through these wrappers (it keeps padded neighbour tables and
fuses the message/aggregate step); they exist for operator-level drop-in use and tests.

Gradients: ``global_max_pool``, ``scatter_max`` (and with it ``MessagePassing.propagate``) and ``knn_interpolate`` are
differentiable with respect to their features (HIP backward kernels, ``csrc/p2w_grad.hip``, the same bits on every run);
positions, batch vectors and indices get none.  A tied maximum sends its whole gradient to the lowest row.  ``PointNetConv``
trains through ``edge_layer1`` (``csrc/p2w_edge.hip``: the hoisted layer 1 of the edge MLP with a deterministic backward) and
``scatter_max``, or, with ``fused_bn_max``, through ``relu_bn_max`` (``csrc/p2w_bnmax.hip``: ReLU, training-mode BatchNorm1d and the
segment max in one forward and one backward kernel, differentiable with respect to its input and BatchNorm's weight and bias); its
fused eval-mode kernel and ``Net.forward`` stay inference-only.  ``InvertedResidualBlock`` (``model.py:46-85``) trains through
``bn_chain`` (``csrc/p2w_bnchain.hip``): everything between two of its 1x1 convolutions - depthwise convolution, training-mode
BatchNorm1d, ReLU, up to three times, and the residual add - computed from the GEMM's output alone in both directions.  ``FPModule``
(``model.py:142-153``) trains through ``interp_add_relu`` (``csrc/p2w_fp.hip``: layer 0 hoisted behind the interpolation, the add and the
ReLU in the interpolation's pass) and ``relu_bn`` (``csrc/p2w_bnchain.hip``: ReLU and training-mode BatchNorm1d from the GEMM's output).

dtypes under autocast: ``bn_chain``, ``relu_bn``, ``relu_bn_max``, ``bn_relu_rowdot`` and ``scatter_max`` / ``global_max_pool`` take a float16 or
bfloat16 tensor as it is, save that tensor and write a gradient of its dtype from the kernel (``half_io``, default True; False casts to fp32
first - the same bits); ``bn_chain`` and ``relu_bn`` return that dtype on request (``out_dtype``), for a result that goes into ``F.linear``
and nowhere else.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, lib, ptr, stream, ws_bytes


def _csr(batch, nb):
    b = batch.to(torch.int64).contiguous()
    return torch.searchsorted(b, torch.arange(nb + 1, device=b.device, dtype=torch.int64)).to(torch.int32)


def _num_batches(*batches):
    m = 0
    for b in batches:
        if b is not None and b.numel():
            m = max(m, int(b.max()) + 1)   # host sync, as in torch-cluster's Python wrappers
    return max(m, 1)


def _xyzr(pos):
    _lib.require_cuda(pos)
    n = pos.shape[0]
    out = torch.zeros((n, 4), dtype=torch.float32, device=pos.device)
    out[:, :3] = pos[:, :3].to(torch.float32)
    return out


def _ws(name, *args, device):
    """The workspace of entry point ``name`` for these sizes (``_lib.ws_bytes``: a refused size is a RuntimeError)."""
    return torch.empty(ws_bytes(name, *args), dtype=torch.uint8, device=device)


def voxel_grid(pos, size, batch=None):
    _lib.require_cuda(pos)
    n = pos.shape[0]
    if batch is None:
        batch = torch.zeros(n, dtype=torch.long, device=pos.device)
    nb = _num_batches(batch)
    x = _xyzr(pos)
    cell = torch.empty(n, dtype=torch.int64, device=pos.device)
    ws, csr = _ws("voxel_sample", max(n, 1), device=pos.device), _csr(batch, nb)
    check(lib().p2w_voxel_grid(ptr(x), ptr(csr), nb, n, float(size), ptr(cell), ptr(ws), ws.numel(), stream()),
          "voxel_grid")
    return cell


def consecutive_cluster(src):
    _lib.require_cuda(src)
    n = src.numel()
    src = src.to(torch.int64).contiguous()
    inv = torch.empty(n, dtype=torch.int32, device=src.device)
    perm = torch.empty(n, dtype=torch.int32, device=src.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=src.device)
    ws = _ws("voxel_sample", max(n, 1), device=src.device)
    check(lib().p2w_consecutive_cluster(ptr(src), n, ptr(inv), ptr(perm), ptr(cnt), ptr(ws), ws.numel(), stream()),
          "consecutive_cluster")
    return inv.to(torch.int64), perm[: int(cnt)].to(torch.int64)


def _search(kind, x, y, arg, batch_x, batch_y, k):
    _lib.require_cuda(x, y)
    dev = x.device
    if batch_x is None:
        batch_x = torch.zeros(x.shape[0], dtype=torch.long, device=dev)
    if batch_y is None:
        batch_y = torch.zeros(y.shape[0], dtype=torch.long, device=dev)
    nb = _num_batches(batch_x, batch_y)
    m = y.shape[0]
    nbr = torch.empty((m, k), dtype=torch.int32, device=dev)
    deg = torch.empty(m, dtype=torch.int32, device=dev)
    xx, yy = _xyzr(x), _xyzr(y)
    px, py = _csr(batch_x, nb), _csr(batch_y, nb)
    if kind == "knn":
        bb = torch.empty((lib().p2w_tile_bbox_count(nb, x.shape[0]), 6), dtype=torch.float32, device=dev)
        check(lib().p2w_tile_bbox(ptr(xx), ptr(px), nb, x.shape[0], ptr(bb), stream()), "tile_bbox")
        check(lib().p2w_knn(ptr(xx), ptr(px), ptr(yy), None, ptr(py), nb, m, k, ptr(nbr), ptr(deg), ptr(bb), 0, stream()),
              "knn")
    else:
        check(lib().p2w_ball_query(ptr(xx), ptr(px), ptr(yy), None, ptr(py), nb, m, float(arg), k, ptr(nbr), ptr(deg),
                                   None, 0, stream()), "radius")
    return nbr, deg


def _edges(nbr, deg):
    """padded [m,k] table -> [2,E] (query, candidate), query-major: boolean-mask compaction."""
    m, k = nbr.shape
    mask = torch.arange(k, device=nbr.device)[None, :] < deg[:, None]
    q = torch.arange(m, device=nbr.device)[:, None].expand(m, k)[mask]
    return torch.stack([q, nbr[mask].to(torch.int64)], 0)


def radius(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32, num_workers=1):
    if not 1 <= max_num_neighbors <= 100:   # torch-cluster's limit (65 .. 100 run on the one-thread-per-query path)
        raise RuntimeError("max_num_neighbors must be in 1..100")
    return _edges(*_search("radius", x, y, r, batch_x, batch_y, int(max_num_neighbors)))


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False, num_workers=1):
    if cosine:
        raise RuntimeError("cosine distance is not supported")
    if not 1 <= k <= 100:
        raise RuntimeError("`k` needs to smaller than or equal to 100")   # torch-cluster's TORCH_CHECK (65 .. 100: one thread per query)
    return _edges(*_search("knn", x, y, None, batch_x, batch_y, int(k)))


def _wants_grad(x):
    return torch.is_grad_enabled() and x.requires_grad


# float16 in and out of the training operators.  Under autocast the GEMMs around bn_chain, relu_bn, relu_bn_max, bn_relu_rowdot and
# scatter_max / global_max_pool give and take float16.  True: with a gradient to track, a float16 z / x goes to the kernels as it is
# (the ``*_io`` entry points of include/p2w.h widen it as they load it), it is the tensor saved for the backward, and dz / grad_x is written in
# float16 by the kernel.  False: the route as it was - the big tensor is cast to fp32 first, that copy is saved, and the fp32
# gradient is rounded in one more pass - launch for launch.  The two give the same bits everywhere: only the element type at the
# loads and stores differs, and a float16 store is the one rounding the cast would have made.
# bfloat16 (autocast with dtype=torch.bfloat16) takes the same two routes with its own element type: a bfloat16 store is the one
# round-to-nearest-even conversion of torch.Tensor.bfloat16().  (The chain entry points take the dtype code P2W_BF16; the head and the
# segment max have entry points of their own for bfloat16, p2w_*_bf16 - include/p2w.h.)
half_io = True

_HALF_TYPES = (torch.float16, torch.bfloat16)
_CODES = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def _keeps_half(x):
    return half_io and x.dtype in _HALF_TYPES and x.is_cuda


def _code(t):
    return _CODES.get(t.dtype, _lib.F32)


def _grad_for(grad_out, z):
    """The output's gradient as the kernel reads it: float16 / bfloat16 as it arrives where z has that dtype, fp32 otherwise."""
    if z.dtype in _HALF_TYPES and grad_out.dtype == z.dtype:
        return grad_out.contiguous()
    return _f32c(grad_out)


def _no_autocast():
    return torch.autocast("cuda", enabled=False)


def _entry(name, t):
    """(entry point, its dtype arguments) of the head and the segment max for the big tensor ``t``: ``p2w_<name>_bf16`` has bfloat16 in its
    name, ``p2w_<name>_io`` takes the code of fp32 or float16 (and refuses P2W_BF16)."""
    if t.dtype == torch.bfloat16:
        return getattr(lib(), f"p2w_{name}_bf16"), ()
    return getattr(lib(), f"p2w_{name}_io"), (_code(t),)


def _half_twin(base, doc):
    """The ``half_io`` route of ``base`` as a class of its own, ``<base>Half`` (so ``grad_fn`` says which route ran): the same argument
    list, ``base._forward(..., keeps_half=True)`` and ``base._backward`` with autocast off and without the fp32 route's cast of the inputs
    - the big float16 / bfloat16 tensor goes to the kernels as it is, is the tensor saved, and gets its gradient in its dtype."""
    def forward(ctx, *args):
        with _no_autocast():
            return base._forward(ctx, *args, keeps_half=True)

    def backward(ctx, *grads):
        with _no_autocast():
            return base._backward(ctx, *grads)

    return type(base.__name__ + "Half", (base,), {"forward": staticmethod(forward), "backward": staticmethod(backward), "__doc__": doc})


# The prelude of the operators that own a training-mode BatchNorm1d (relu_bn_max, bn_chain, relu_bn, bn_relu_rowdot).  Each one refuses in
# this order - _check_bn, its shapes, its out_dtype - takes its eval-mode shortcut, and only then _training_tick: a refused call and an
# eval-mode call move no counter and no statistic.
def _check_bn(bn, who, not_a_bn=None):
    if not isinstance(bn, torch.nn.BatchNorm1d):
        raise TypeError(not_a_bn or f"{who}: bn must be a torch.nn.BatchNorm1d")
    if not bn.affine or not bn.track_running_stats or bn.momentum is None:
        raise NotImplementedError(f"{who} supports BatchNorm1d(affine=True, track_running_stats=True, momentum=<float>) as the reference builds it")


def _training_tick(z, bns):
    """PyTorch's refusal of a batch of fewer than two rows, then ``num_batches_tracked`` of every ``bn`` as its forward would count."""
    if z.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {z.size()}")
    for bn in bns:
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)


def _running(bns):
    """[(running_mean, running_var)] as the kernels update them in place: fp32 and contiguous - the modules' own storage wherever it is."""
    return [tuple(t.detach().to(torch.float32).contiguous() for t in (bn.running_mean, bn.running_var)) for bn in bns]


def _write_back(bns, running):
    """After the launch: a pair that ``_running`` had to copy goes back into its module."""
    with torch.no_grad():
        for bn, pair in zip(bns, running):
            for mine, theirs in zip(pair, (bn.running_mean, bn.running_var)):
                if mine.data_ptr() != theirs.data_ptr():
                    theirs.copy_(mine)


def _pad4(x):
    """fp32, contiguous, rows padded to a multiple of 4 floats (the interpolation kernels' 16-byte accesses)."""
    F0 = x.shape[1]
    F = (F0 + 3) // 4 * 4
    xc = x.to(torch.float32)
    if F != F0:
        xc = torch.nn.functional.pad(xc, (0, F - F0))
    return xc.contiguous(), F


class _SegmentMax(torch.autograd.Function):
    """Segment max that keeps its winners (``p2w_segment_max_arg``) for the gather of the backward
    (``p2w_segment_max_bwd``).  The arg table is saved for backward only."""

    @staticmethod
    def _forward(ctx, x, csr, nb, keeps_half=False):
        xc = x.contiguous() if keeps_half else x.to(torch.float32).contiguous()
        n, F = xc.shape
        out = torch.empty((nb, F), dtype=torch.float32, device=x.device)
        arg = torch.empty((nb, F), dtype=torch.int32, device=x.device)
        fn, code = _entry("segment_max_arg", xc)
        check(fn(ptr(xc), *code, F, F, ptr(csr), nb, ptr(out), ptr(arg), stream()), "segment_max_arg")
        ctx.save_for_backward(arg, csr)
        ctx.shape, ctx.dtype, ctx.kernel_dtype = (n, F), x.dtype, xc.dtype
        return out

    @staticmethod
    def _backward(ctx, grad_out):
        arg, csr = ctx.saved_tensors
        n, F = ctx.shape
        g = grad_out.to(torch.float32).contiguous()
        grad_x = torch.empty((n, F), dtype=ctx.kernel_dtype, device=g.device)
        fn, code = _entry("segment_max_bwd", grad_x)
        check(fn(ptr(g), F, ptr(arg), ptr(csr), arg.shape[0], F, ptr(grad_x), *code, F, n, stream()), "segment_max_bwd")
        return grad_x.to(ctx.dtype), None, None

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, csr, nb):
        return _SegmentMax._forward(ctx, x, csr, nb)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        return _SegmentMax._backward(ctx, grad_out)


_SegmentMaxHalf = _half_twin(_SegmentMax, """``_SegmentMax`` on a float16 or bfloat16 ``x`` as it is (``half_io``): no fp32 copy of ``x``,
    ``grad_x`` written in its dtype by the kernel.""")


def global_max_pool(x, batch, size=None):
    """Differentiable with respect to ``x`` (``batch`` gets no gradient).  Tie rule: the whole gradient of a column goes to
    the lowest row that holds the segment's maximum.  (PyTorch's ``scatter_reduce(amax)`` splits it evenly among the tied
    rows; the two rules give the same parameter gradients wherever the tied values are equal outputs of the same layer -
    the ReLU zeros after ``local_nn``.)  Without a gradient to track the launches and the bits are those of
    ``p2w_segment_max`` alone."""
    _lib.require_cuda(x, batch)
    nb = _num_batches(batch) if size is None else int(size)
    csr = _csr(batch, nb)
    if _wants_grad(x):
        return (_SegmentMaxHalf if _keeps_half(x) else _SegmentMax).apply(x, csr, nb)
    x = x.to(torch.float32).contiguous()
    out = torch.empty((nb, x.shape[1]), dtype=torch.float32, device=x.device)
    check(lib().p2w_segment_max(ptr(x), x.shape[1], x.shape[1], ptr(csr), nb, ptr(out), stream()), "global_max_pool")
    return out


def scatter_max(src, index, dim=0, out=None, dim_size=None):
    """Sorted-index segment max (the reference's index is the query-major edge target, pointnet.py:122).  Differentiable
    with respect to ``src`` with ``global_max_pool``'s tie rule (lowest row wins); the second result stays ``None``."""
    assert dim == 0
    res = global_max_pool(src.reshape(src.shape[0], -1), index, size=dim_size)
    return res.reshape((res.shape[0],) + tuple(src.shape[1:])), None


def _interp_forward(x, rc, rf, nbr, deg, k):
    m, F0 = rf.shape[0], x.shape[1]
    xc, F = _pad4(x)
    out = torch.empty((m, F), dtype=torch.float32, device=x.device)
    check(lib().p2w_interp_concat(ptr(xc), F, ptr(rc), ptr(rf), ptr(nbr), ptr(deg), int(k), None, 0, m,
                                  ptr(out), F, stream()), "knn_interpolate")
    return out if F == F0 else out[:, :F0].contiguous()


class _KnnInterpolate(torch.autograd.Function):
    """``p2w_interp_concat`` forward, ``p2w_interp_bwd`` backward: gradient with respect to the coarse features only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, rc, rf, nbr, deg, k):
        ctx.save_for_backward(rc, rf, nbr, deg)
        ctx.k, ctx.shape, ctx.dtype = int(k), tuple(x.shape), x.dtype
        return _interp_forward(x, rc, rf, nbr, deg, k)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        rc, rf, nbr, deg = ctx.saved_tensors
        (n, F0), m = ctx.shape, rf.shape[0]
        g, F = _pad4(grad_out)
        grad_x = torch.empty((n, F), dtype=torch.float32, device=g.device)
        ws = _ws("interp_bwd", m, ctx.k, n, device=g.device)
        check(lib().p2w_interp_bwd(ptr(g), F, F, ptr(rc), ptr(rf), ptr(nbr), ptr(deg), ctx.k, m, n, ptr(grad_x), F,
                                   ptr(ws), ws.numel(), stream()), "knn_interpolate backward")
        if F != F0:
            grad_x = grad_x[:, :F0].contiguous()
        return grad_x.to(ctx.dtype), None, None, None, None, None


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, num_workers=1):
    """PyG's signature and default (k = 3); any 1 <= k <= 100 and any feature width (rows are padded to a multiple of 4
    floats for the kernel's 16-byte accesses).  Differentiable with respect to ``x``; positions and batch vectors get no
    gradient."""
    _lib.require_cuda(x, pos_x, pos_y)
    if not 1 <= k <= 100:
        raise RuntimeError("knn_interpolate: k must be in 1..100")
    nbr, deg = _search("knn", pos_x, pos_y, None, batch_x, batch_y, int(k))
    rc, rf = _xyzr(pos_x), _xyzr(pos_y)   # keep both alive until the launch is enqueued
    if _wants_grad(x):
        return _KnnInterpolate.apply(x, rc, rf, nbr, deg, int(k))
    return _interp_forward(x, rc, rf, nbr, deg, k)


def _edge_l1_forward(P, Wg, rs, rd, csr, src, out_dtype=None):
    """(geo [E, 4], H1 [E, C1]) of ``p2w_edge_l1_io``: fp32, contiguous inputs; H1 in ``out_dtype`` (None: fp32)."""
    (n_src, C1), M, E = P.shape, rd.shape[0], src.numel()
    geo = torch.empty((E, 4), dtype=torch.float32, device=P.device)
    H1 = torch.empty((E, C1), dtype=out_dtype or torch.float32, device=P.device)
    check(lib().p2w_edge_l1_io(ptr(P), C1, ptr(rs), ptr(rd), ptr(csr), ptr(src), ptr(Wg), n_src, M, E, C1, ptr(geo), ptr(H1), _code(H1), C1,
                               stream()), "edge_layer1")
    return geo, H1


def _f32c(t):
    return _lib.aligned16(t.detach().to(torch.float32).contiguous())


def _edge_l1_backward(ctx, g, recompute):
    """(grad P, grad Wg, grad pos_src) for both routes of ``edge_layer1``.  What ``ctx`` saved first is the fp32 H1, whose sign is the ReLU
    mask (``p2w_edge_l1_bwd`` on an fp32 ``g``), or - ``recompute`` - the fp32 P that the mask is computed from once more
    (``p2w_edge_l1_bwd_io`` on ``g`` in the dtype it came in)."""
    mask, geo, src, Wg = ctx.saved_tensors
    n_src, E, C1, dev = ctx.n_src, src.numel(), Wg.shape[1], g.device
    gP = torch.empty((n_src, C1), dtype=torch.float32, device=dev)
    gR = torch.empty(n_src, dtype=torch.float32, device=dev)
    gWg = torch.empty((4, C1), dtype=torch.float32, device=dev)
    ws = _ws("edge_l1_bwd", E, n_src, C1, device=dev)
    tail = (ptr(mask), C1, ptr(geo), ptr(src), ptr(Wg), n_src, E, C1, ptr(gP), C1, ptr(gR), ptr(gWg), ptr(ws), ws.numel(), stream())
    if recompute:
        check(lib().p2w_edge_l1_bwd_io(ptr(g), _code(g), C1, *tail), "edge_layer1 backward")
    else:
        check(lib().p2w_edge_l1_bwd(ptr(g), C1, *tail), "edge_layer1 backward")
    gpos = None
    if ctx.needs_input_grad[2]:
        gpos = torch.zeros((n_src, 4), dtype=torch.float32, device=dev)
        gpos[:, 3] = gR
        gpos = gpos.to(ctx.dtypes[2])
    return gP.to(ctx.dtypes[0]), gWg.to(ctx.dtypes[1]), gpos


class _EdgeLayer1(torch.autograd.Function):
    """``p2w_edge_l1`` forward, ``p2w_edge_l1_bwd`` backward: gradients with respect to P, Wg and column 3 of ``pos_src``.
    H1 (the ReLU mask) and geo are saved for backward only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, P, Wg, pos_src, rd, csr, src):
        Pc, Wc = _f32c(P), _f32c(Wg)
        geo, H1 = _edge_l1_forward(Pc, Wc, _f32c(pos_src), rd, csr, src)
        ctx.save_for_backward(H1, geo, src, Wc)
        ctx.n_src, ctx.dtypes = P.shape[0], (P.dtype, Wg.dtype, pos_src.dtype)
        ctx.mark_non_differentiable(geo)
        return H1, geo

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_H1, _grad_geo):
        return (*_edge_l1_backward(ctx, _f32c(grad_H1), recompute=False), None, None, None)


class _EdgeLayer1Half(torch.autograd.Function):
    """``_EdgeLayer1`` with H1 in float16 or bfloat16 (``p2w_edge_l1_io`` / ``p2w_edge_l1_bwd_io``): no [E, C1] tensor is saved - the
    backward recomputes the ReLU mask from the widened fp32 P, geo, src and Wg with the forward's own statements, so it is the fp32
    H1's mask whatever the 16-bit store rounded to zero - and the gradient is read in the dtype it arrives in."""

    @staticmethod
    def forward(ctx, P, Wg, pos_src, rd, csr, src, out_dtype):
        with _no_autocast():
            Pc, Wc = _f32c(P), _f32c(Wg)
            geo, H1 = _edge_l1_forward(Pc, Wc, _f32c(pos_src), rd, csr, src, out_dtype)
            ctx.save_for_backward(Pc, geo, src, Wc)
            ctx.n_src, ctx.dtypes = P.shape[0], (P.dtype, Wg.dtype, pos_src.dtype)
            ctx.mark_non_differentiable(geo)
            return H1, geo

    @staticmethod
    def backward(ctx, grad_H1, _grad_geo):
        with _no_autocast():
            g = _lib.aligned16(grad_H1.detach().contiguous()) if grad_H1.dtype in _HALF_TYPES else _f32c(grad_H1)
            return (*_edge_l1_backward(ctx, g, recompute=True), None, None, None, None)


def edge_layer1(P, Wg, pos_src, pos_dst, edge_index, out_dtype=None):
    """Layer 1 of the reference's edge MLP (``pointnet.py:116-132`` followed by ``local_nn[0]``, ``model.py:198-202``), hoisted:
    ``H1[e] = relu(P[j] + geo[e] @ Wg)`` for edge e = (j -> i) with ``P = x_src @ W1[:, :F_in].T + b1`` ``[n_src, C1]`` computed by
    the caller once per source point, ``Wg`` ``[4, C1]`` = the transposed last four columns of ``W1`` and ``geo[e] = ((pos_j - pos_i)
    / (maxd_i + 1e-8), refl_j)``.  ``pos_*`` = [n, 4] (xyz, reflectance); ``edge_index`` = (source j, target i), grouped by target,
    any number of edges per target.  One HIP kernel; the [E, F_in + 4] message tensor is never formed.

    Differentiable with respect to ``P``, ``Wg`` and ``pos_src[:, 3]`` (the other columns of ``pos_src`` get zeros, ``pos_dst``
    none: positions get no gradient anywhere in this module).  The backward uses no floating-point atomics: the same bits on
    every run.  Computes in fp32 under autocast.  Without a gradient to track nothing is saved.

    ``out_dtype`` None (the default, whatever autocast says): H1 in fp32, and the fp32 H1 is saved for the backward as its ReLU
    mask.  ``torch.float16`` / ``torch.bfloat16``: the kernel stores H1 in that dtype - the fp32 result rounded once, the bits of the
    default call followed by ``.to(out_dtype)`` - no [E, C1] tensor is saved (the backward recomputes the mask from the fp32 P, geo
    and Wg, bit for bit the fp32 H1's), and the output's gradient is read in the dtype it arrives in: the same gradients as the
    default call followed by ``.to(out_dtype)``, bit for bit."""
    _lib.require_cuda(P, Wg, pos_src, pos_dst, edge_index)
    if P.dim() != 2 or tuple(Wg.shape) != (4, P.shape[1]) or pos_src.shape != (P.shape[0], 4) or pos_dst.dim() != 2 or pos_dst.shape[1] != 4:
        raise RuntimeError("edge_layer1: P [n_src, C1], Wg [4, C1], pos_src [n_src, 4], pos_dst [M, 4]")
    if out_dtype is not None and out_dtype not in _HALF_TYPES:
        raise RuntimeError("edge_layer1: out_dtype is None (fp32), torch.float16 or torch.bfloat16")
    j, i = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    n_src, M = P.shape[0], pos_dst.shape[0]
    if j.numel() and (bool((i[1:] < i[:-1]).any()) or int(i[0]) < 0 or int(i[-1]) >= M or int(j.min()) < 0 or int(j.max()) >= n_src):
        raise RuntimeError("edge_layer1: edges must be grouped by target (ascending edge_index[1]) and index existing points")
    csr = torch.searchsorted(i.contiguous(), torch.arange(M + 1, device=i.device, dtype=torch.int64)).to(torch.int32)
    src, rd = j.to(torch.int32).contiguous(), _f32c(pos_dst)
    if torch.is_grad_enabled() and (P.requires_grad or Wg.requires_grad or pos_src.requires_grad):
        if out_dtype is not None:
            return _EdgeLayer1Half.apply(P, Wg, pos_src, rd, csr, src, out_dtype)[0]
        return _EdgeLayer1.apply(P, Wg, pos_src, rd, csr, src)[0]
    return _edge_l1_forward(_f32c(P), _f32c(Wg), _f32c(pos_src), rd, csr, src, out_dtype)[1]


def _relu_bn_max_forward(zc, gamma, beta, csr, M, bn):
    """(out, ext, arg, mean, invstd) of ``p2w_relu_bn_max_io`` on a contiguous fp32, float16 or bfloat16 z (the vectors fp32); bn's running
    statistics move in place."""
    (E, C2), dev = zc.shape, zc.device
    out, ext = (torch.empty((M, C2), dtype=torch.float32, device=dev) for _ in range(2))
    arg = torch.empty((M, C2), dtype=torch.int32, device=dev)
    mean, invstd = (torch.empty(C2, dtype=torch.float32, device=dev) for _ in range(2))
    running = _running([bn])
    rm, rv = running[0]
    ws = _ws("relu_bn_max", E, M, C2, device=dev)
    check(lib().p2w_relu_bn_max_io(ptr(zc), _code(zc), C2, ptr(csr), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), float(bn.momentum), float(bn.eps),
                                   E, M, C2, ptr(out), ptr(ext), ptr(arg), ptr(mean), ptr(invstd), ptr(ws), ws.numel(), stream()), "relu_bn_max")
    _write_back([bn], running)
    return out, ext, arg, mean, invstd


class _ReluBnMax(torch.autograd.Function):
    """``p2w_relu_bn_max`` forward, ``p2w_relu_bn_max_bwd`` backward: gradients with respect to z, gamma and beta.  Saved for backward:
    z, arg, ext, mean, invstd, the CSR and gamma - no [E, C2] tensor besides z itself."""

    @staticmethod
    def _forward(ctx, z, gamma, beta, csr, M, bn, keeps_half=False):
        zc, gc = z.detach().contiguous() if keeps_half else _f32c(z), _f32c(gamma)
        out, ext, arg, mean, invstd = _relu_bn_max_forward(zc, gc, _f32c(beta), csr, M, bn)
        ctx.save_for_backward(zc, arg, ext, mean, invstd, csr, gc)
        ctx.dtypes = (z.dtype, gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def _backward(ctx, grad_out):
        z, arg, ext, mean, invstd, csr, gamma = ctx.saved_tensors
        (E, C2), M, dev = z.shape, arg.shape[0], z.device
        g = _f32c(grad_out)
        dz = torch.empty((E, C2), dtype=z.dtype, device=dev)
        dgamma, dbeta = (torch.empty(C2, dtype=torch.float32, device=dev) for _ in range(2))
        ws = _ws("relu_bn_max", E, M, C2, device=dev)
        check(lib().p2w_relu_bn_max_bwd_io(ptr(g), ptr(z), _code(z), C2, ptr(csr), ptr(arg), ptr(ext), ptr(mean), ptr(invstd), ptr(gamma), E, M,
                                           C2, ptr(dz), C2, ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream()), "relu_bn_max backward")
        return dz.to(ctx.dtypes[0]), dgamma.to(ctx.dtypes[1]), dbeta.to(ctx.dtypes[2]), None, None, None

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, z, gamma, beta, csr, M, bn):
        return _ReluBnMax._forward(ctx, z, gamma, beta, csr, M, bn)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        return _ReluBnMax._backward(ctx, grad_out)


_ReluBnMaxHalf = _half_twin(_ReluBnMax, """``_ReluBnMax`` on a float16 or bfloat16 ``z`` as it is (``half_io``): ``z`` itself is saved - no fp32
    copy of it - the output stays fp32 and ``dz`` is written in ``z``'s dtype by the kernel.""")


def _relu_bn_max_sorted(z, index, bn, M):
    """``relu_bn_max`` on an index that is known to be ascending and inside [0, M)."""
    if not bn.training:
        return scatter_max(bn(torch.relu(z)), index, dim=0, dim_size=M)[0]
    _training_tick(z, [bn])
    csr = torch.searchsorted(index.to(torch.int64).contiguous(), torch.arange(M + 1, device=index.device, dtype=torch.int64)).to(torch.int32)
    if torch.is_grad_enabled() and (z.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad):
        return (_ReluBnMaxHalf if _keeps_half(z) else _ReluBnMax).apply(z, bn.weight, bn.bias, csr, M, bn)
    zc = z.detach().contiguous() if _keeps_half(z) else _f32c(z)
    return _relu_bn_max_forward(zc, _f32c(bn.weight), _f32c(bn.bias), csr, M, bn)[0]


def relu_bn_max(z, index, bn, dim_size=None):
    """``scatter_max(bn(relu(z)), index, dim=0, dim_size=dim_size)[0]`` for a ``torch.nn.BatchNorm1d`` ``bn`` in training mode without
    the three [E, C] tensors in between (the tail of the reference's edge MLP and its aggregation, ``model.py:198-202`` and
    ``pointnet.py:122``): per column BatchNorm is an affine map, non-decreasing for ``gamma >= 0`` and non-increasing for ``gamma < 0``,
    so the maximum of ``bn(relu(z))`` over a target's rows is bn of the rows' maximum of ``relu(z)`` (their minimum where ``gamma < 0``).
    ``z`` [E, C] is the pre-activation, ``index`` [E] the ascending target of every row (as for ``scatter_max``), ``dim_size`` the
    number of targets (default ``index.max() + 1``); targets without rows get 0.

    Two HIP kernels (``csrc/p2w_bnmax.hip``): the forward reads ``z`` once (fp64 column sums of ``relu(z)`` and its square, one
    extremum and its lowest row per target and column) and updates ``bn.running_mean``, ``bn.running_var`` (unbiased variance) and
    ``bn.num_batches_tracked`` as PyTorch does; the backward reads ``z`` once more and writes the gradient with respect to ``z`` once,
    BatchNorm's gradient through the batch statistics included.  Gradients go to ``z``, ``bn.weight`` and ``bn.bias`` in their dtypes;
    a tied extremum sends its gradient to the lowest row (``scatter_max``'s rule).  Where ``gamma == 0`` the output does not depend on
    the winner; the gradient with respect to gamma is taken on the ``gamma >= 0`` side (through the maximum).  No floating-point
    atomics: the same bits on every run, the batch statistics included.  Saved for backward: ``z`` and [M, C] / [C] tensors only.
    Computes in fp32 under autocast and returns fp32.  A float16 or bfloat16 ``z`` is read as it is, is itself the tensor saved for the
    backward and gets its gradient written in its dtype by the kernel (module switch ``half_io``, default True); with ``half_io`` False
    it is cast to fp32 first: one extra pass each way and an fp32 copy saved, the same bits.  Under ``no_grad`` the forward runs, the
    running statistics move, and nothing is saved.

    With ``bn.training`` false this is the composition itself, ``scatter_max(bn(relu(z)))`` on the running statistics: the kernels'
    backward carries the batch-statistics terms, so eval mode would need a second backward, not a flag.  ``affine=False``,
    ``track_running_stats=False`` and ``momentum=None`` raise ``NotImplementedError`` (the reference builds none of them); fewer than
    two rows in training mode raise PyTorch's ``ValueError``."""
    _lib.require_cuda(z, index)
    _check_bn(bn, "relu_bn_max")
    if z.dim() != 2 or z.shape[1] != bn.num_features or index.dim() != 1 or index.numel() != z.shape[0]:
        raise RuntimeError("relu_bn_max: z [E, C] with C = bn.num_features, index [E]")
    i = index.to(torch.int64)
    M = (int(i.max()) + 1 if i.numel() else 1) if dim_size is None else int(dim_size)
    if i.numel() and (bool((i[1:] < i[:-1]).any()) or int(i[0]) < 0 or int(i[-1]) >= M):
        raise RuntimeError("relu_bn_max: index must be ascending and inside [0, dim_size)")
    return _relu_bn_max_sorted(z, i, bn, M)


# --------------------------------------------------------------------------- the 8th operator
class MessagePassing(torch.nn.Module):
    """The part of PyG's ``MessagePassing`` the reference uses (``pointnet.py:19,71,108``): ``propagate(edge_index, **kw)``
    with ``flow='source_to_target'`` and ``aggr='max'``.  ``edge_index[0]`` = source j, ``edge_index[1]`` = target i,
    grouped by target (as ``radius`` / ``knn`` return them).  ``message``'s parameters are collected the PyG way:
    ``<name>_j`` = ``kw[name]`` (its first element if a pair) gathered by source, ``<name>_i`` = (second element) by
    target, ``edge_index_i`` / ``edge_index_j`` the index rows; the messages are max-aggregated per target
    (``scatter_max``, HIP), targets without edges get 0.  The reference's own ``PointNetConv`` subclass runs on this
    base unchanged; ``PointNetConv`` below is the fused replacement of the whole layer."""

    def __init__(self, aggr="max", flow="source_to_target", **kw):
        super().__init__()
        if aggr != "max" or flow != "source_to_target":
            raise NotImplementedError("only aggr='max', flow='source_to_target' (what the reference uses)")
        self.aggr, self.flow = aggr, flow

    def reset_parameters(self):
        pass

    def propagate(self, edge_index, size=None, **kw):
        import inspect
        j, i = edge_index[0], edge_index[1]
        args = {}
        for name in inspect.signature(self.message).parameters:
            if name == "edge_index_i":
                args[name] = i
            elif name == "edge_index_j":
                args[name] = j
            elif name.endswith("_j") or name.endswith("_i"):
                v = kw[name[:-2]]
                side = 0 if name.endswith("_j") else 1
                v = v[side] if isinstance(v, (tuple, list)) else v
                args[name] = None if v is None else v[j if side == 0 else i]
            else:
                args[name] = kw[name]
        msg = self.message(**args)
        if size is not None:
            n_dst = size[1] if isinstance(size, (tuple, list)) else size
        else:
            n_dst = None
            for v in kw.values():   # number of targets = rows of the second element of any pair argument
                if isinstance(v, (tuple, list)) and v[1] is not None:
                    n_dst = v[1].shape[0]
                    break
                if torch.is_tensor(v):
                    n_dst = v.shape[0]
            if n_dst is None:
                n_dst = int(i.max()) + 1
        return scatter_max(msg, i, dim=0, dim_size=n_dst)[0]


def _local_nn_weights(local_nn):
    """(W1, b1, W2, b2, bn_scale, bn_shift) of ``MLP([F_in + 4, C1, C2])`` (model.py:198-202): Lin + ReLU, Lin + ReLU + BN."""
    try:
        lin1, lin2, bn = local_nn[0][0], local_nn[1][0], local_nn[1][2]
    except (TypeError, IndexError) as e:
        raise NotImplementedError("the fused PointNetConv supports local_nn = MLP([F_in + 4, C1, C2]) as the reference builds it") from e
    if bn.training:
        raise RuntimeError("the fused PointNetConv kernel is inference-only (its BatchNorm is folded from the running statistics): "
                           "call .eval() on the whole layer, or .train() on the whole layer for the route that trains")
    s = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps))
    t = bn.bias.double() - bn.running_mean.double() * s
    return lin1.weight, lin1.bias, lin2.weight, lin2.bias, s.float(), t.float()


class PointNetConv(MessagePassing):
    """Drop-in for the reference's ``src.pointnet.PointNetConv`` (``pointnet.py:19-132``; built at ``model.py:94``, called
    at ``:123``): same constructor, same parameter names (``local_nn.*``), same
    ``forward(x, (pos_src, pos_dst), edge_index)`` with ``pos`` = [n, 4] (sf-scaled xyz, reflectance).

    Training mode: ``P = F.linear(x_src, W1[:, :F_in], b1)`` once per source point, ``edge_layer1`` (HIP, deterministic backward),
    the module's own ``local_nn[1]`` (Linear, ReLU, training-mode BatchNorm1d: the running statistics update as in the
    reference), ``scatter_max`` (HIP), ``global_nn``.  Gradients reach ``x``, ``pos_src[:, 3]`` and every parameter; xyz gets none.
    Any number of edges per target.

    Eval mode (under ``no_grad``): message MLP + max aggregation by ONE fused HIP kernel (``p2w_sa_conv``, fp32 MFMA: the [E, C] edge tensors are never formed) after a
    hoisted layer-1 GEMM (``p2w_gemm``).  Edges must be grouped by target with at most ``P2W_MAX_K_CONV`` = 32 per target
    (``radius(max_num_neighbors=32)`` / ``knn(k=32)`` as the reference calls them); ``global_nn`` is applied afterwards as
    in the reference; ``add_self_loops`` must be False (the reference passes False).

    ``fused_bn_max`` (default False; set it on the instance or the class): the training route computes everything after the layer-2
    GEMM with ``relu_bn_max`` instead of ReLU, BatchNorm1d and ``scatter_max`` one after the other - no [E, C2] tensor besides the
    GEMM's output, the same bits on every run; under autocast that output goes to the kernels in its float16 or bfloat16 as it is
    (``half_io``).  False leaves every launch and bit of the training route as it was; eval mode does
    not look at it."""

    fused_bn_max = False

    def __init__(self, local_nn=None, global_nn=None, add_self_loops=True, **kw):
        self.radius = kw.pop("radius", None)
        kw.setdefault("aggr", "max")
        super().__init__(**kw)
        self.local_nn, self.global_nn, self.add_self_loops = local_nn, global_nn, add_self_loops

    def forward(self, x, pos, edge_index):
        return self._forward_train(x, pos, edge_index) if self.training else self._forward_fused(x, pos, edge_index)

    def _forward_train(self, x, pos, edge_index):
        from torch.nn import BatchNorm1d, Linear, ReLU
        if self.add_self_loops:
            raise NotImplementedError("add_self_loops=True is not supported (the reference builds the layer with False)")
        if x is None or (isinstance(x, (tuple, list)) and x[0] is None):
            raise NotImplementedError("PointNetConv: x = None is not supported (the reference's layers all carry features)")
        x_src = x[0] if isinstance(x, (tuple, list)) else x
        pos_src, pos_dst = pos if isinstance(pos, (tuple, list)) else (pos, pos)
        _lib.require_cuda(x_src, pos_src, pos_dst, edge_index)
        nn = self.local_nn
        try:
            ok = (len(nn) == 2 and len(nn[0]) == 2 and len(nn[1]) == 3 and isinstance(nn[0][0], Linear) and isinstance(nn[0][1], ReLU)
                  and isinstance(nn[1][0], Linear) and isinstance(nn[1][1], ReLU) and isinstance(nn[1][2], BatchNorm1d))
        except TypeError:
            ok = False
        if not ok:
            raise NotImplementedError("PointNetConv supports local_nn = MLP([F_in + 4, C1, C2]) as the reference builds it")
        lin1, F_in = nn[0][0], x_src.shape[1]
        if lin1.weight.shape[1] != F_in + 4 or pos_src.shape[1] != 4 or pos_dst.shape[1] != 4:
            raise RuntimeError("PointNetConv: local_nn must take F_in + 4 inputs, pos must be [n, 4]")
        P = torch.nn.functional.linear(x_src, lin1.weight[:, :F_in], lin1.bias)     # hoisted layer 1, once per source point
        # (under autocast with half_io, H1 goes to local_nn[1][0] in the autocast dtype as the kernel stored it)
        H1 = edge_layer1(P, lin1.weight[:, F_in:F_in + 4].t(), pos_src, pos_dst, edge_index, out_dtype=_gemm_dtype(P))
        if self.fused_bn_max:       # (edge_layer1 has checked that the targets ascend inside [0, M))
            out = _relu_bn_max_sorted(nn[1][0](H1), edge_index[1], nn[1][2], pos_dst.shape[0])
        else:
            out = scatter_max(nn[1](H1), edge_index[1], dim=0, dim_size=pos_dst.shape[0])[0]
        if self.global_nn is not None:
            out = self.global_nn(out)
        return out

    @torch.no_grad()
    def _forward_fused(self, x, pos, edge_index):
        import ctypes as C
        if self.add_self_loops:
            raise NotImplementedError("add_self_loops=True is not supported (the reference builds the layer with False)")
        x_src = x[0] if isinstance(x, (tuple, list)) else x
        pos_src, pos_dst = pos if isinstance(pos, (tuple, list)) else (pos, pos)
        _lib.require_cuda(x_src, pos_src, pos_dst, edge_index)
        dev = pos_src.device
        W1, b1, W2, b2, bn_s, bn_t = _local_nn_weights(self.local_nn)
        n_src, M, F_in = pos_src.shape[0], pos_dst.shape[0], x_src.shape[1]
        C1, C2 = W1.shape[0], W2.shape[0]
        if W1.shape[1] != F_in + 4 or pos_src.shape[1] != 4 or C1 % 4:
            raise RuntimeError("PointNetConv: local_nn must take F_in + 4 inputs, pos must be [n, 4], C1 a multiple of 4")
        j, i = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
        E = j.numel()
        deg = torch.bincount(i, minlength=M)
        if E and (int(deg.max()) > 32 or bool((i[1:] < i[:-1]).any())):
            raise RuntimeError("PointNetConv: edges must be grouped by target, at most 32 per target")
        start = torch.cumsum(deg, 0) - deg
        nbr = torch.full((M, 32), -1, dtype=torch.int32, device=dev)
        if E:
            nbr[i, torch.arange(E, device=dev) - start[i]] = j.to(torch.int32)
        deg = deg.to(torch.int32)
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        # hoisted layer 1: P = x_src W1x^T + b1 once per source point
        Np, Kp = _lib.packed_dims(C1, F_in)
        Wx = torch.zeros((Np, Kp), dtype=torch.float32, device=dev)
        Wx[:C1, :F_in] = f32(W1[:, :F_in])
        xs = f32(x_src)
        if F_in % 4:
            xs = torch.nn.functional.pad(xs, (0, 4 - F_in % 4)).contiguous()
        # (+ M zero rows: an empty neighbour slot is addressed through the target's own record, which follows the sources)
        P = torch.zeros((n_src + M, C1), dtype=torch.float32, device=dev)
        b1d = f32(b1)
        ep = _lib.Epilogue(ptr(b1d), None, None, None, None, None, 0, 0, 0, 0, 0)
        check(lib().p2w_gemm(ptr(xs), xs.shape[1], ptr(Wx), n_src, C1, F_in, C.byref(ep), ptr(P), C1, stream()), "PointNetConv hoist")
        _, C1p = _lib.packed_dims(C2, C1)
        w1r4 = torch.zeros((4, C1p), dtype=torch.float32, device=dev)
        w1r4[:, :C1] = f32(W1[:, F_in:F_in + 4]).t()
        N2p, _ = _lib.packed_dims(C2, C1)
        W2p = torch.zeros((N2p, C1p), dtype=torch.float32, device=dev)
        W2p[:C2, :C1] = f32(W2)
        # sources and targets in one record array (the kernel addresses a target through an index into the sources)
        rec = torch.cat([f32(pos_src), f32(pos_dst)], 0)
        idx = torch.arange(n_src, n_src + M, dtype=torch.int32, device=dev)
        one, zb = torch.ones(1, dtype=torch.float32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
        b2d, sd, td = f32(b2), f32(bn_s), f32(bn_t)
        out = torch.empty((M, C2), dtype=torch.float32, device=dev)
        check(lib().p2w_sa_conv(ptr(P), C1, ptr(rec), ptr(idx), ptr(zb), ptr(one), ptr(nbr), ptr(deg), 32, M, ptr(w1r4),
                                ptr(W2p), C1, C2, ptr(b2d), ptr(sd), ptr(td), ptr(out), C2, stream()), "PointNetConv")
        if self.global_nn is not None:
            out = self.global_nn(out)
        return out


# --------------------------------------------------------------------------- chains of BatchNorms between two GEMMs
def _chain_stage_array(meta, vec, running):
    """The host array of ``p2w_bn_stage`` for ``meta`` = [(bn, relu, has_dw)] over the flat fp32 vectors ``vec`` (per stage gamma, beta
    and, with a depthwise convolution, its weight and bias); ``running`` = [(running_mean, running_var)] or None (backward)."""
    arr, i = (_lib.BnStage * len(meta))(), 0
    for t, (bn, relu, has_dw) in enumerate(meta):
        gamma, beta = vec[i], vec[i + 1]
        dw_w, dw_b = (vec[i + 2], vec[i + 3]) if has_dw else (None, None)
        i += 4 if has_dw else 2
        rm, rv = running[t] if running is not None else (None, None)
        arr[t] = _lib.BnStage(ptr(dw_w), ptr(dw_b), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), float(bn.momentum), float(bn.eps), int(bool(relu)))
    return arr


def _bn_chain_forward(zc, rc, meta, vec, out_dtype=torch.float32):
    """(out, mean, invstd) of ``p2w_bn_chain_io`` on a contiguous fp32, float16 or bfloat16 z (everything else fp32, contiguous); every bn's
    running statistics move in place."""
    (M, C), L, dev = zc.shape, len(meta), zc.device
    out = torch.empty((M, C), dtype=out_dtype, device=dev)
    mean, invstd = (torch.empty((L, C), dtype=torch.float32, device=dev) for _ in range(2))
    bns = [bn for bn, _, _ in meta]
    running = _running(bns)
    ws = _ws("bn_chain", M, C, L, device=dev)
    check(lib().p2w_bn_chain_io(ptr(zc), _code(zc), C, ptr(rc), C, _chain_stage_array(meta, vec, running), L, M, C, ptr(out), _code(out), C,
                                ptr(mean), ptr(invstd), ptr(ws), ws.numel(), stream()), "bn_chain")
    _write_back(bns, running)
    return out, mean, invstd


class _BnChain(torch.autograd.Function):
    """``p2w_bn_chain`` forward, ``p2w_bn_chain_bwd`` backward: gradients with respect to z, the residual, every BatchNorm's weight and
    bias and every depthwise weight and bias.  Saved for backward: z, the output where the chain has a residual (its sign is the last
    ReLU's mask; the residual itself is not needed), and [L, C] / [C] tensors - no other [M, C] tensor.  The gradient with respect
    to a depthwise bias is exactly zero: BatchNorm subtracts the column mean, which removes any bias added in front of it."""

    @staticmethod
    def _forward(ctx, z, residual, meta, out_dtype, *params, keeps_half=False):
        zc = z.detach().contiguous() if keeps_half else _f32c(z)
        rc = None if residual is None else _f32c(residual)
        vec = [_f32c(p.reshape(-1)) for p in params]
        out, mean, invstd = _bn_chain_forward(zc, rc, meta, vec, out_dtype)
        ctx.save_for_backward(zc, mean, invstd, *vec, *([out] if rc is not None else []))
        ctx.meta, ctx.has_res = meta, rc is not None
        ctx.like = [(t.dtype, t.shape) for t in (z, *params)] + ([(residual.dtype, residual.shape)] if rc is not None else [])
        return out

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, z, residual, meta, out_dtype, *params):   # (meta holds modules and flags, no tensors: custom_fwd passes it through)
        return _BnChain._forward(ctx, z, residual, meta, out_dtype, *params)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        return _BnChain._backward(ctx, grad_out)

    @staticmethod
    def _backward(ctx, grad_out):
        saved = ctx.saved_tensors
        z, mean, invstd = saved[:3]
        meta, n_vec = ctx.meta, sum(4 if m[2] else 2 for m in ctx.meta)
        vec, out = saved[3:3 + n_vec], (saved[3 + n_vec] if ctx.has_res else None)
        (M, C), L, dev = z.shape, len(meta), z.device
        g = _grad_for(grad_out, z)
        dz = torch.empty((M, C), dtype=z.dtype, device=dev)
        dres = torch.empty((M, C), dtype=torch.float32, device=dev) if ctx.has_res and ctx.needs_input_grad[1] else None
        dgamma, dbeta = (torch.empty((L, C), dtype=torch.float32, device=dev) for _ in range(2))
        any_dw = any(m[2] for m in meta)
        ddw_w, ddw_b = (torch.empty((L, C), dtype=torch.float32, device=dev) for _ in range(2)) if any_dw else (None, None)
        ws = _ws("bn_chain", M, C, L, device=dev)
        check(lib().p2w_bn_chain_bwd_io(ptr(g), _code(g), C, ptr(z), _code(z), C, ptr(out), C, _chain_stage_array(meta, vec, None), L, ptr(mean),
                                        ptr(invstd), M, C, ptr(dz), C, ptr(dres), C, ptr(dgamma), ptr(dbeta), ptr(ddw_w), ptr(ddw_b), ptr(ws),
                                        ws.numel(), stream()), "bn_chain backward")
        grads = []
        for t, (_, _, has_dw) in enumerate(meta):
            grads += [dgamma[t], dbeta[t]] + ([ddw_w[t], ddw_b[t]] if has_dw else [])
        like = ctx.like
        grads = [gr.to(dt).reshape(shape) for gr, (dt, shape) in zip(grads, like[1:1 + n_vec])]
        return (dz.to(like[0][0]), None if dres is None else dres.to(like[-1][0]), None, None, *grads)


_BnChainHalf = _half_twin(_BnChain, """``_BnChain`` on a float16 or bfloat16 ``z`` as it is (``half_io``): ``z`` itself is saved, the output is fp32
    or ``z``'s dtype, its gradient is read in the dtype it arrives in and ``dz`` is written in ``z``'s dtype by the kernel.  Parameters, the
    residual and the saved output of a chain with a residual stay fp32.""")


def _chain_normalise(stages, C, who="bn_chain"):
    meta = []
    for st in stages:
        bn, relu, dw = st if len(st) == 3 else (*st, None)
        _check_bn(bn, who, f"{who}: every stage is (BatchNorm1d, relu) or (BatchNorm1d, relu, depthwise Conv1d or None)")
        if bn.num_features != C:
            raise RuntimeError(f"{who}: z [M, C] with C = num_features of every BatchNorm1d")
        if dw is not None:
            if not (isinstance(dw, torch.nn.Conv1d) and dw.in_channels == dw.out_channels == dw.groups == C and dw.kernel_size == (1,)
                    and dw.stride == (1,) and dw.padding == (0,)):
                raise TypeError(f"{who}: a depthwise convolution is Conv1d(C, C, 1, groups=C)")
            if dw.bias is None:
                raise NotImplementedError(f"{who} supports a depthwise Conv1d with a bias as the reference builds it")
        meta.append((bn, bool(relu), dw))
    return meta


def _out_dtype(out_dtype, z, who):
    if out_dtype not in (None, torch.float32, *_HALF_TYPES):
        raise RuntimeError(f"{who}: out_dtype is None (float32), torch.float32, torch.float16 or torch.bfloat16")
    if out_dtype in _HALF_TYPES and z.dtype != out_dtype:
        name = str(out_dtype).split(".")[-1]
        raise RuntimeError(f"{who}: out_dtype=torch.{name} needs a {name} z")
    return torch.float32 if out_dtype is None else out_dtype


def bn_chain(z, stages, residual=None, out_dtype=None):
    """Everything the reference's ``InvertedResidualBlock`` (``model.py:46-85``) runs between two of its 1x1 convolutions, on the
    pre-activation ``z`` [M, C] in rows: for every stage of ``stages``, in order, an optional depthwise ``Conv1d(C, C, 1, groups=C)``
    (``w[c] * x + b[c]``), a ``torch.nn.BatchNorm1d`` and an optional ReLU; then, with ``residual`` [M, C], ``relu(x + residual)``.
    ``stages`` is a list of ``(bn, relu)`` or ``(bn, relu, depthwise_conv)``, one to three of them.

    Training mode (``csrc/p2w_bnchain.hip``): once a BatchNorm's two statistics are known every stage is a map per column, so the chain
    is computed from ``z`` alone - one read of ``z`` per BatchNorm for its fp64 column sums (the stages in front of it recomputed on
    the way; the statistics of ``w * u + b`` follow from those of ``u``), one read and one write to apply the chain; the backward reads
    ``z`` and the output's gradient once per BatchNorm for its two column sums and once more to write the gradient with respect to
    ``z``.  Saved for backward: ``z``, the output where there is a residual, and [L, C] tensors; no intermediate activation.
    Gradients go to ``z``, ``residual``, every ``bn.weight`` and ``bn.bias`` and every depthwise weight and bias in their dtypes.  The
    gradient with respect to a depthwise bias is exactly zero - BatchNorm removes a bias added in front of it - and is returned as
    zeros; the one with respect to a depthwise weight is tiny against its terms (only ``eps`` keeps it from zero) and is taken from
    fp64 sums.  Running statistics (unbiased variance) and ``num_batches_tracked`` of every stage update as PyTorch's.  No
    floating-point atomics: the same bits on every run.  Computes in fp32 under autocast.  Under ``no_grad`` the forward runs, the
    statistics move and nothing is saved.

    dtypes: the result is fp32 (``out_dtype=None``).  A float16 ``z`` with a gradient to track is read as it is, is itself the tensor
    saved for the backward, and gets its gradient written in float16 by the kernel (module switch ``half_io``, default True; False
    casts it to fp32 first and saves that copy - the same bits, more passes).  ``out_dtype=torch.float16``, legal with a float16 ``z``
    and no residual only, stores the fp32 result rounded to nearest even, which is what a following autocast GEMM would make of it:
    ask for it only where the result goes into ``F.linear`` and nowhere else - never where a ReLU mask is taken from it.  A bfloat16
    ``z`` (autocast with ``dtype=torch.bfloat16``) is treated the same way, with ``out_dtype=torch.bfloat16``.

    Every ``bn`` must be in the same mode.  In eval mode this is the plain composition on the running statistics.  ``affine=False``,
    ``track_running_stats=False``, ``momentum=None`` and a depthwise convolution without a bias raise ``NotImplementedError``; fewer
    than two rows in training mode raise PyTorch's ``ValueError``."""
    _lib.require_cuda(z, residual)
    if z.dim() != 2:
        raise RuntimeError("bn_chain: z [M, C]")
    out_dtype = _out_dtype(out_dtype, z, "bn_chain")
    if out_dtype in _HALF_TYPES and residual is not None:
        raise RuntimeError("bn_chain: out_dtype=torch.float16 / torch.bfloat16 is for a chain without a residual (its output is the last ReLU's mask)")
    if not 1 <= len(stages) <= _lib.BN_CHAIN_MAX:
        raise RuntimeError(f"bn_chain: one to {_lib.BN_CHAIN_MAX} stages")
    meta = _chain_normalise(stages, z.shape[1])
    if residual is not None and residual.shape != z.shape:
        raise RuntimeError("bn_chain: residual has z's shape")
    if len({bn.training for bn, _, _ in meta}) != 1:
        raise RuntimeError("bn_chain: every BatchNorm1d must be in the same mode")
    if not meta[0][0].training:
        x = z
        for bn, relu, dw in meta:
            if dw is not None:
                x = x * dw.weight.reshape(-1) + dw.bias
            x = bn(x)
            if relu:
                x = torch.relu(x)
        x = x if residual is None else torch.relu(x + residual)
        return x.to(out_dtype) if out_dtype in _HALF_TYPES else x
    _training_tick(z, [bn for bn, _, _ in meta])
    params = []
    for bn, _, dw in meta:
        params += [bn.weight, bn.bias] + ([dw.weight, dw.bias] if dw is not None else [])
    flags = [(bn, relu, dw is not None) for bn, relu, dw in meta]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (z, residual, *params)):
        if _keeps_half(z):
            return _BnChainHalf.apply(z, residual, flags, out_dtype, *params)
        return _BnChain.apply(z, residual, flags, torch.float32, *params).to(out_dtype)
    return _bn_chain_forward(_f32c(z), None if residual is None else _f32c(residual), flags, [_f32c(p.reshape(-1)) for p in params])[0].to(out_dtype)


class _DepthwiseSeparable(torch.nn.Module):
    """Holds the four submodules of the reference's ``DepthwiseSeparableConv1d(C, C, kernel_size=1)`` under its names."""

    def __init__(self, channels):
        super().__init__()
        self.depthwise_conv = torch.nn.Conv1d(channels, channels, kernel_size=1, groups=channels)
        self.depthwise_bn = torch.nn.BatchNorm1d(channels)
        self.pointwise_conv = torch.nn.Conv1d(channels, channels, kernel_size=1)
        self.pointwise_bn = torch.nn.BatchNorm1d(channels)


def _gemm_dtype(z):
    """The ``out_dtype`` of a result that goes straight into ``F.linear`` and nowhere else: ``z``'s float16 or bfloat16 where ``half_io``
    is on and the GEMM that made ``z`` ran in that dtype under autocast - the next one would round an fp32 result the same way - else
    None (fp32)."""
    if half_io and z.dtype in _HALF_TYPES and torch.is_autocast_enabled("cuda") and z.dtype == torch.get_autocast_dtype("cuda"):
        return z.dtype
    return None


def _rows_conv(conv, x):
    """A ``Conv1d(kernel_size=1)`` on rows: a Linear over the channels."""
    return torch.nn.functional.linear(x, conv.weight[:, :, 0], conv.bias)


class InvertedResidualBlock(torch.nn.Module):
    """Drop-in for the reference's ``InvertedResidualBlock`` (``model.py:46-85``): the same constructor, the same submodule tree and
    therefore the same ``state_dict`` keys (``expand.0/1``, ``conv.0.*``, ``conv.1``, ``conv.3.*``, ``conv.4``, ``project.0/1``,
    ``shortcut.0/1`` where ``in_channels != out_channels``), the same ``forward(x)`` on ``x`` [M, in_channels] in rows - without the
    transposed [1, C, M] view.

    Training mode: the four 1x1 convolutions are ``F.linear`` on ``weight[:, :, 0]``, and everything between them - eight training-mode
    BatchNorms (nine with a shortcut), seven ReLUs, two depthwise convolutions, the residual add - is four ``bn_chain`` calls (five with a shortcut), so no
    activation besides the four GEMM outputs is kept for the backward.  Eval mode is the plain composition statement by statement."""

    def __init__(self, in_channels, out_channels, expansion_factor=4):
        super().__init__()
        from torch.nn import BatchNorm1d, Conv1d, ReLU, Sequential
        self.expansion_factor = expansion_factor
        e = in_channels * expansion_factor
        self.expand = Sequential(Conv1d(in_channels, e, kernel_size=1), BatchNorm1d(e), ReLU())
        self.conv = Sequential(_DepthwiseSeparable(e), BatchNorm1d(e), ReLU(), _DepthwiseSeparable(e), BatchNorm1d(e))
        self.project = Sequential(Conv1d(e, out_channels, kernel_size=1), BatchNorm1d(out_channels))
        self.shortcut = (Sequential(Conv1d(in_channels, out_channels, kernel_size=1), BatchNorm1d(out_channels))
                         if in_channels != out_channels else Sequential())

    def forward(self, x):
        if x.dim() != 2 or x.shape[1] != self.expand[0].in_channels:
            raise RuntimeError("InvertedResidualBlock: x [M, in_channels]")
        if not self.training:
            return self._forward_plain(x)
        d0, d3 = self.conv[0], self.conv[3]
        # (the first three results go into the next GEMM and nowhere else: float16 where the GEMMs run in float16, _gemm_dtype)
        z = _rows_conv(self.expand[0], x)
        h = bn_chain(z, [(self.expand[1], True), (d0.depthwise_bn, True, d0.depthwise_conv)], out_dtype=_gemm_dtype(z))
        z = _rows_conv(d0.pointwise_conv, h)
        h = bn_chain(z, [(d0.pointwise_bn, True), (self.conv[1], True), (d3.depthwise_bn, True, d3.depthwise_conv)], out_dtype=_gemm_dtype(z))
        z = _rows_conv(d3.pointwise_conv, h)
        h = bn_chain(z, [(d3.pointwise_bn, True), (self.conv[4], False)], out_dtype=_gemm_dtype(z))
        res = bn_chain(_rows_conv(self.shortcut[0], x), [(self.shortcut[1], False)]) if len(self.shortcut) else x
        return bn_chain(_rows_conv(self.project[0], h), [(self.project[1], False)], residual=res)

    def _forward_plain(self, x):
        relu = torch.relu
        out = relu(self.expand[1](_rows_conv(self.expand[0], x)))
        for i in (0, 3):
            d = self.conv[i]
            out = out * d.depthwise_conv.weight[:, 0, 0] + d.depthwise_conv.bias
            out = relu(d.depthwise_bn(out))
            out = relu(d.pointwise_bn(_rows_conv(d.pointwise_conv, out)))
            if i == 0:
                out = relu(self.conv[1](out))
        out = self.conv[4](out)
        out = self.project[1](_rows_conv(self.project[0], out))
        res = self.shortcut[1](_rows_conv(self.shortcut[0], x)) if len(self.shortcut) else x
        return relu(out + res)


# --------------------------------------------------------------------------- the feature-propagation module for training
def _interp_add_relu_forward(Pc, S, rc, rf, nbr, deg, k):
    """H [m, C padded to a multiple of 4] of ``p2w_interp_add_relu`` (the pad columns are zeros)."""
    (pc, C), (sc, _) = _pad4(Pc.detach()), _pad4(S.detach())
    pc, sc = _lib.aligned16(pc), _lib.aligned16(sc)
    m, n_c = sc.shape[0], pc.shape[0]
    H = torch.empty((m, C), dtype=torch.float32, device=sc.device)
    check(lib().p2w_interp_add_relu(ptr(pc), C, ptr(sc), C, ptr(rc), ptr(rf), ptr(nbr), ptr(deg), int(k), m, n_c, C, ptr(H), C, stream()),
          "interp_add_relu")
    return H


class _InterpAddRelu(torch.autograd.Function):
    """``p2w_interp_add_relu`` forward, ``p2w_interp_add_relu_bwd`` backward: gradients with respect to Pc and S.  Saved for backward:
    the output H (its sign is the ReLU's mask) and the index tensors - neither Pc nor S."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, Pc, S, rc, rf, nbr, deg, k):
        H = _interp_add_relu_forward(Pc, S, rc, rf, nbr, deg, k)
        C0 = S.shape[1]
        out = H if H.shape[1] == C0 else H[:, :C0].contiguous()
        ctx.save_for_backward(H, rc, rf, nbr, deg)
        ctx.k, ctx.n_c, ctx.C0, ctx.dtypes = int(k), Pc.shape[0], C0, (Pc.dtype, S.dtype)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        H, rc, rf, nbr, deg = ctx.saved_tensors
        (m, C), n_c, C0, dev = H.shape, ctx.n_c, ctx.C0, H.device
        g = _lib.aligned16(_pad4(grad_out)[0])
        dS = torch.empty((m, C), dtype=torch.float32, device=dev)
        dPc = torch.empty((n_c, C), dtype=torch.float32, device=dev)
        ws = _ws("interp_add_relu_bwd", m, ctx.k, n_c, device=dev)
        check(lib().p2w_interp_add_relu_bwd(ptr(g), C, ptr(H), C, ptr(rc), ptr(rf), ptr(nbr), ptr(deg), ctx.k, m, n_c, C, ptr(dS), C, ptr(dPc), C,
                                            ptr(ws), ws.numel(), stream()), "interp_add_relu backward")
        if C != C0:
            dS, dPc = dS[:, :C0].contiguous(), dPc[:, :C0].contiguous()
        return dPc.to(ctx.dtypes[0]), dS.to(ctx.dtypes[1]), None, None, None, None, None


def interp_add_relu(Pc, S, pos_x, pos_y, batch_x=None, batch_y=None, k=3):
    """``torch.relu(knn_interpolate(Pc, pos_x, pos_y, batch_x, batch_y, k) + S)`` in one HIP kernel (``csrc/p2w_fp.hip``), bit for
    bit: layer 0 of the reference's ``FPModule`` (``model.py:142-153``) with the interpolation hoisted behind the GEMM.
    ``knn_interpolate`` is linear in its features and its weights sum to 1, so for ``W0 = [Wc | Ws]``

        ``relu(Linear0(cat[interp(xc), x_skip])) = relu(interp(xc @ Wc.T) + (x_skip @ Ws.T + b0))``:

    the caller computes ``Pc = xc @ Wc.T`` [n_c, C] on the coarse rows and ``S = x_skip @ Ws.T + b0`` [m, C] on the fine rows, and
    neither the interpolated [m, Fc] tensor nor the [m, Fc + Fs] concatenation is formed.  Any 1 <= k <= 100, any width (rows are
    padded to a multiple of 4 floats for the kernel's 16-byte accesses).

    Differentiable with respect to ``Pc`` and ``S`` (positions and batch vectors get none): ``dS = g [H > 0]`` in one pass, ``dPc`` =
    ``knn_interpolate``'s backward of ``dS`` (``p2w_interp_bwd``'s code: no floating-point atomics, the same bits on every run).
    Saved for backward: the output itself and the index tensors, neither ``Pc`` nor ``S``.  Computes in fp32 under autocast.
    Without a gradient to track the forward runs alone and nothing is saved."""
    _lib.require_cuda(Pc, S, pos_x, pos_y)
    if not 1 <= k <= 100:
        raise RuntimeError("interp_add_relu: k must be in 1..100")
    if Pc.dim() != 2 or S.dim() != 2 or Pc.shape[1] != S.shape[1] or Pc.shape[0] != pos_x.shape[0] or S.shape[0] != pos_y.shape[0]:
        raise RuntimeError("interp_add_relu: Pc [n_c, C] with pos_x [n_c, 3+], S [m, C] with pos_y [m, 3+]")
    nbr, deg = _search("knn", pos_x, pos_y, None, batch_x, batch_y, int(k))
    rc, rf = _xyzr(pos_x), _xyzr(pos_y)
    if torch.is_grad_enabled() and (Pc.requires_grad or S.requires_grad):
        return _InterpAddRelu.apply(Pc, S, rc, rf, nbr, deg, int(k))
    H = _interp_add_relu_forward(Pc, S, rc, rf, nbr, deg, k)
    return H if H.shape[1] == S.shape[1] else H[:, :S.shape[1]].contiguous()


def _relu_bn_forward(zc, gamma, beta, bn, out_dtype=torch.float32):
    """(out, mean, invstd) of ``p2w_relu_bn_io`` on a contiguous fp32, float16 or bfloat16 z (the vectors fp32); bn's running statistics move in
    place."""
    (M, C), dev = zc.shape, zc.device
    out = torch.empty((M, C), dtype=out_dtype, device=dev)
    mean, invstd = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(2))
    running = _running([bn])
    rm, rv = running[0]
    ws = _ws("relu_bn", M, C, device=dev)
    check(lib().p2w_relu_bn_io(ptr(zc), _code(zc), C, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), float(bn.momentum), float(bn.eps), M, C, ptr(out),
                               _code(out), C, ptr(mean), ptr(invstd), ptr(ws), ws.numel(), stream()), "relu_bn")
    _write_back([bn], running)
    return out, mean, invstd


class _ReluBn(torch.autograd.Function):
    """``p2w_relu_bn`` forward, ``p2w_relu_bn_bwd`` backward: gradients with respect to z, gamma and beta.  Saved for backward: z, mean,
    invstd and gamma - no [M, C] tensor besides z itself."""

    @staticmethod
    def _forward(ctx, z, gamma, beta, bn, out_dtype, keeps_half=False):
        zc, gc = z.detach().contiguous() if keeps_half else _f32c(z), _f32c(gamma)
        out, mean, invstd = _relu_bn_forward(zc, gc, _f32c(beta), bn, out_dtype)
        ctx.save_for_backward(zc, mean, invstd, gc)
        ctx.dtypes = (z.dtype, gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def _backward(ctx, grad_out):
        z, mean, invstd, gamma = ctx.saved_tensors
        (M, C), dev = z.shape, z.device
        g = _grad_for(grad_out, z)
        dz = torch.empty((M, C), dtype=z.dtype, device=dev)
        dgamma, dbeta = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(2))
        ws = _ws("relu_bn", M, C, device=dev)
        check(lib().p2w_relu_bn_bwd_io(ptr(g), _code(g), C, ptr(z), _code(z), C, ptr(gamma), ptr(mean), ptr(invstd), M, C, ptr(dz), C, ptr(dgamma),
                                       ptr(dbeta), ptr(ws), ws.numel(), stream()), "relu_bn backward")
        return dz.to(ctx.dtypes[0]), dgamma.to(ctx.dtypes[1]), dbeta.to(ctx.dtypes[2]), None, None

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, z, gamma, beta, bn, out_dtype):
        return _ReluBn._forward(ctx, z, gamma, beta, bn, out_dtype)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        return _ReluBn._backward(ctx, grad_out)


_ReluBnHalf = _half_twin(_ReluBn, """``_ReluBn`` on a float16 or bfloat16 ``z`` as it is (``half_io``): ``z`` itself is saved, the output is fp32 or
    ``z``'s dtype, its gradient is read in the dtype it arrives in and ``dz`` is written in ``z``'s dtype by the kernel.""")


def relu_bn(z, bn, out_dtype=None):
    """``bn(torch.relu(z))`` for a ``torch.nn.BatchNorm1d`` ``bn`` in training mode on the pre-activation ``z`` [M, C] in rows: the tail
    of every later layer of the reference's ``MLP`` (``model.py:198-202``: Linear, ReLU, BatchNorm1d).  By definition the one-stage
    ``bn_chain`` on ``relu(z)`` - the same device code with the ReLU applied as ``z`` is loaded (``csrc/p2w_bnchain.hip``), so the output,
    the statistics and every gradient equal ``bn_chain(torch.relu(z), [(bn, False)])`` bit for bit, without the [M, C] tensor
    ``relu(z)`` and without its copy kept for the backward.  Forward: ``z`` read twice, the output written once; backward: ``z`` and the
    gradient read twice, the gradient with respect to ``z`` written once (``dz = 0`` where ``z <= 0``); three launches each way.
    Gradients go to ``z``, ``bn.weight`` and ``bn.bias`` in their dtypes.  Running statistics (unbiased variance) and
    ``num_batches_tracked`` update as PyTorch's.  No floating-point atomics: the same bits on every run.  Computes in fp32 under
    autocast.  Under ``no_grad`` the forward runs, the statistics move and nothing is saved.  dtypes, ``half_io`` and ``out_dtype`` as
    ``bn_chain``'s: a float16 ``z`` is read and saved as it is, ``out_dtype=torch.float16`` only where the result goes into ``F.linear``
    alone.

    In eval mode this is ``bn(torch.relu(z))`` itself.  ``affine=False``, ``track_running_stats=False`` and ``momentum=None`` raise
    ``NotImplementedError``; fewer than two rows in training mode raise PyTorch's ``ValueError``."""
    _lib.require_cuda(z)
    _check_bn(bn, "relu_bn")
    if z.dim() != 2 or z.shape[1] != bn.num_features:
        raise RuntimeError("relu_bn: z [M, C] with C = bn.num_features")
    out_dtype = _out_dtype(out_dtype, z, "relu_bn")
    if not bn.training:
        x = bn(torch.relu(z))
        return x.to(out_dtype) if out_dtype in _HALF_TYPES else x
    _training_tick(z, [bn])
    if torch.is_grad_enabled() and (z.requires_grad or bn.weight.requires_grad or bn.bias.requires_grad):
        if _keeps_half(z):
            return _ReluBnHalf.apply(z, bn.weight, bn.bias, bn, out_dtype)
        return _ReluBn.apply(z, bn.weight, bn.bias, bn, torch.float32).to(out_dtype)
    return _relu_bn_forward(_f32c(z), _f32c(bn.weight), _f32c(bn.bias), bn)[0].to(out_dtype)


# --------------------------------------------------------------------------- the head behind conv1 for training
def _bn_relu_rowdot_forward(zc, gamma, beta, w, b, bn):
    """(logit, mean, invstd) of ``p2w_bn_relu_rowdot_io`` (``_bf16``) on a contiguous fp32 or float16 (bfloat16) z (the vectors fp32); bn's running statistics
    move in place."""
    (M, C), dev = zc.shape, zc.device
    logit = torch.empty(M, dtype=torch.float32, device=dev)
    mean, invstd = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(2))
    running = _running([bn])
    rm, rv = running[0]
    ws = _ws("bn_relu_rowdot", M, C, device=dev)
    tail = (ptr(gamma), ptr(beta), ptr(w), ptr(b), ptr(rm), ptr(rv), float(bn.momentum), float(bn.eps), M, C, ptr(logit), ptr(mean), ptr(invstd),
            ptr(ws), ws.numel(), stream())
    fn, code = _entry("bn_relu_rowdot", zc)
    check(fn(ptr(zc), *code, C, *tail), "bn_relu_rowdot")
    _write_back([bn], running)
    return logit, mean, invstd


class _BnReluRowdot(torch.autograd.Function):
    """``p2w_bn_relu_rowdot`` forward, ``p2w_bn_relu_rowdot_bwd`` backward: gradients with respect to z, gamma, beta, the weight and the
    bias.  Saved for backward: z and [C] vectors - neither ``relu(bn(z))`` nor its gradient exists."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, z, gamma, beta, weight, bias, bn):
        return _BnReluRowdot._forward(ctx, z, gamma, beta, weight, bias, bn)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        return _BnReluRowdot._backward(ctx, grad_out)

    @staticmethod
    def _forward(ctx, z, gamma, beta, weight, bias, bn, keeps_half=False):
        zc = z.detach().contiguous() if keeps_half else _f32c(z)
        gc, bc, wc = _f32c(gamma), _f32c(beta), _lib.aligned16(_f32c(weight.reshape(-1)))
        logit, mean, invstd = _bn_relu_rowdot_forward(zc, gc, bc, wc, _f32c(bias.reshape(-1)), bn)
        ctx.save_for_backward(zc, mean, invstd, gc, bc, wc)
        ctx.like = [(t.dtype, t.shape) for t in (z, gamma, beta, weight, bias)]
        return logit

    @staticmethod
    def _backward(ctx, grad_out):
        z, mean, invstd, gamma, beta, w = ctx.saved_tensors
        (M, C), dev = z.shape, z.device
        g = _f32c(grad_out)
        dz = torch.empty((M, C), dtype=z.dtype, device=dev)
        dgamma, dbeta, dw = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(3))
        dbias = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _ws("bn_relu_rowdot", M, C, device=dev)
        tail = (ptr(gamma), ptr(beta), ptr(w), ptr(mean), ptr(invstd), M, C, ptr(dz), C, ptr(dgamma), ptr(dbeta), ptr(dw), ptr(dbias), ptr(ws),
                ws.numel(), stream())
        fn, code = _entry("bn_relu_rowdot_bwd", z)
        check(fn(ptr(g), ptr(z), *code, C, *tail), "bn_relu_rowdot backward")
        return (*[gr.to(dt).reshape(shape) for gr, (dt, shape) in zip((dz, dgamma, dbeta, dw, dbias), ctx.like)], None)


_BnReluRowdotHalf = _half_twin(_BnReluRowdot, """``_BnReluRowdot`` on a float16 or bfloat16 ``z`` as it is (``half_io``): ``z`` itself is saved and
    ``dz`` is written in its dtype by the kernel; the logits and their gradient stay fp32.""")


def bn_relu_rowdot(z, bn, weight, bias):
    """``F.linear(torch.relu(bn(z)), weight, bias)[:, 0]`` for a ``torch.nn.BatchNorm1d`` ``bn`` in training mode and ONE output channel,
    on the pre-activation ``z`` [M, C] in rows: the reference's head behind ``conv1`` (``model.py:242-243``) as the trainer builds it,
    ``num_classes = 1``.  ``weight`` is [1, C] or [1, C, 1] (``conv2.weight``), ``bias`` has one element; the result is [M] float32.

    One operator (``csrc/p2w_head.hip``): the statistics are the one-stage ``bn_chain``'s own device code (the same bits), and the
    third launch reads ``z`` once more and writes M floats - ``relu(bn(z))`` [M, C] is never formed, nor is its gradient on the way
    back: the backward takes three column sums per work item from ``z`` and the M gradients of the logits, reduces them in a fixed
    order and writes ``dz`` in one more pass over ``z``.  ``z`` is read twice in each direction.  Saved for backward: ``z`` and [C]
    vectors.  Gradients go to ``z``, ``bn.weight``, ``bn.bias``, ``weight`` and ``bias`` in their dtypes and shapes.  A row's sum runs
    in an order fixed by C alone (``include/p2w.h``); no floating-point atomics: the same bits on every run.  Running statistics
    (unbiased variance) and ``num_batches_tracked`` update as PyTorch's.  Computes in fp32 under autocast.  Under ``no_grad`` the
    forward runs, the statistics move and nothing is saved.  A float16 ``z`` with a gradient to track is read and saved as it is and
    gets a float16 gradient from the kernel (``half_io``; a bfloat16 ``z`` likewise, in bfloat16); the logits are fp32 either way.

    In eval mode this is the plain composition on the running statistics.  ``affine=False``, ``track_running_stats=False`` and
    ``momentum=None`` raise ``NotImplementedError``; fewer than two rows in training mode raise PyTorch's ``ValueError``."""
    _lib.require_cuda(z, weight, bias)
    _check_bn(bn, "bn_relu_rowdot")
    if z.dim() != 2 or z.shape[1] != bn.num_features:
        raise RuntimeError("bn_relu_rowdot: z [M, C] with C = bn.num_features")
    C = z.shape[1]
    if weight.dim() not in (2, 3) or tuple(weight.shape) != (1, C, 1)[:weight.dim()] or bias is None or bias.numel() != 1:
        raise RuntimeError("bn_relu_rowdot: weight [1, C] or [1, C, 1] and a bias of one element (one output channel)")
    if not bn.training:
        return torch.nn.functional.linear(torch.relu(bn(z)), weight.reshape(1, C), bias.reshape(1))[:, 0]
    _training_tick(z, [bn])
    if torch.is_grad_enabled() and any(t.requires_grad for t in (z, bn.weight, bn.bias, weight, bias)):
        return (_BnReluRowdotHalf if _keeps_half(z) else _BnReluRowdot).apply(z, bn.weight, bn.bias, weight, bias, bn)
    return _bn_relu_rowdot_forward(_f32c(z), _f32c(bn.weight), _f32c(bn.bias), _lib.aligned16(_f32c(weight.reshape(-1))),
                                   _f32c(bias.reshape(-1)), bn)[0]


class FPModule(torch.nn.Module):
    """Drop-in for the reference's ``FPModule`` (``model.py:142-153``): the same constructor (``k``, the channel list ``NN``), ``self.NN``
    built as the reference's ``MLP(NN)`` (``model.py:198-202``) and therefore the same ``state_dict`` keys (``NN.0.0.weight``,
    ``NN.0.0.bias``, ``NN.1.0.*``, ``NN.1.2.*``, ...), the same
    ``forward(x, pos, batch, x_skip, pos_skip, batch_skip) -> (x, pos_skip, batch_skip)``.

    Training mode with ``x_skip`` given: layer 0 is hoisted behind the interpolation -
    ``Pc = F.linear(x, W0[:, :Fc])`` on the coarse rows, ``S = F.linear(x_skip, W0[:, Fc:], b0)`` on the fine rows,
    ``interp_add_relu(Pc, S, ...)`` - and every later layer is ``relu_bn(F.linear(h, Wi, bi), NN[i][2])``.  The GEMMs are PyTorch's in
    both directions; neither the interpolated tensor nor the concatenation is formed, and no activation is kept for the backward
    besides the GEMMs' outputs and layer 0's output.  The same function as the plain composition, other roundings.

    Eval mode, ``x_skip is None`` and ``fused = False`` (class attribute, default True; set it on the class or an instance) run the
    reference's statements one by one: ``knn_interpolate``, ``torch.cat``, ``self.NN``."""

    fused = True

    def __init__(self, k, NN):
        super().__init__()
        from torch.nn import BatchNorm1d, Linear, ReLU, Sequential
        self.k = k
        self.NN = Sequential(*[Sequential(*([Linear(NN[i - 1], NN[i]), ReLU()] + ([BatchNorm1d(NN[i])] if i != 1 else [])))
                               for i in range(1, len(NN))])

    def forward(self, x, pos, batch, x_skip, pos_skip, batch_skip):
        if not (self.training and self.fused and x_skip is not None):
            h = knn_interpolate(x, pos, pos_skip, batch, batch_skip, k=self.k)
            if x_skip is not None:
                h = torch.cat([h, x_skip], dim=1)
            return self.NN(h), pos_skip, batch_skip
        lin0, Fc = self.NN[0][0], x.shape[1]
        if lin0.in_features != Fc + x_skip.shape[1]:
            raise RuntimeError("FPModule: NN[0] must take x.shape[1] + x_skip.shape[1] inputs")
        Pc = torch.nn.functional.linear(x, lin0.weight[:, :Fc])                     # layer 0 on the coarse rows, no bias
        S = torch.nn.functional.linear(x_skip, lin0.weight[:, Fc:], lin0.bias)      # ... and on the fine rows
        h = interp_add_relu(Pc, S, pos, pos_skip, batch, batch_skip, k=self.k)
        layers = list(self.NN)[1:]
        for i, layer in enumerate(layers):      # (an inner result goes into the next GEMM alone: float16 where that GEMM's is; the last is returned)
            z = layer[0](h)
            h = relu_bn(z, layer[2], out_dtype=_gemm_dtype(z) if i + 1 < len(layers) else None)
        return h, pos_skip, batch_skip


def random_subset(n, k, seed, counter=(0, 0), device="cuda", keys=None, return_keys=False):
    """A uniformly random ``k``-subset of ``range(n)`` as an ascending int64 ``[k]`` device tensor (``p2w_random_subset``,
    ``csrc/p2w_sample.hip``): the ``k`` rows with the smallest ``(key, row)``, ``key`` = word 0 of Philox4x32-10 at counter
    ``(row, counter[0], counter[1], P2W_SAMPLE_STREAM)`` under ``seed`` - a function of ``(seed, counter, n, k)`` alone, the same bits on
    every run.  ``n``, ``k``, ``seed`` and the counter words are Python integers; the call is enqueued on the current stream and waits
    for nothing.  ``keys`` (an int32 ``[n]`` device tensor holding the 32-bit patterns) replaces the generator; ``return_keys`` also
    returns the key of every row, stored as int32."""
    n, k, seed, c1, c2 = int(n), int(k), int(seed), int(counter[0]), int(counter[1])
    if not 0 <= k <= n <= _lib.SAMPLE_N_MAX:
        raise ValueError(f"random_subset: need 0 <= k <= n <= {_lib.SAMPLE_N_MAX}, got n = {n}, k = {k}")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("random_subset needs an MI355X (cuda) device; there is no CPU fallback")
    if keys is not None:
        _lib.require_cuda(keys)
        if keys.dtype != torch.int32 or keys.shape != (n,):
            raise ValueError("random_subset: keys must be an int32 tensor of n elements")
        keys, device = keys.contiguous(), keys.device
    with torch.cuda.device(device):
        idx = torch.empty(k, dtype=torch.int64, device=device)
        keys_out = torch.empty(n, dtype=torch.int32, device=device) if return_keys else None
        if n > 0 and k > 0:
            ws = _ws("random_subset", n, device=device)
            check(lib().p2w_random_subset(n, k, seed & 0xffffffffffffffff, c1 & 0xffffffff, c2 & 0xffffffff, ptr(keys), ptr(idx),
                                          ptr(keys_out), ptr(ws), ws.numel(), stream()), "p2w_random_subset")
        elif return_keys and n > 0:                              # k = 0 launches nothing: the keys come from a draw of one row
            keys_out = random_subset(n, 1, seed, (c1, c2), device, keys, True)[1]
    return (idx, keys_out) if return_keys else idx


def cap_subset(n, seg_start, seg_count, k, seed, counter=(0, 0), weight=None, row_id=None, keys=None, return_keys=False):
    """``k`` rows of every one of ``S`` segments of a row space of ``n`` rows in one call, as an int64 ``[S, k]`` device tensor of
    positions (``p2w_cap_subset``, ``csrc/p2w_sample.hip``): the voxeliser's cap.  ``seg_start``, ``seg_count``: int64 ``[S]`` device
    tensors, disjoint segments in ascending order.

    With ``weight`` (float32 ``[n]``) a segment keeps the ``k`` rows smallest in ``(key, position)``, ascending by position, ``key =
    float32(-log(u) / weight)`` with ``u`` from word 0 of Philox4x32-10 at counter ``(row_id, counter[0], counter[1], P2W_CAP_STREAM)``
    under ``seed`` - the law of ``torch.multinomial(weight, k)`` without replacement; a row whose weight is not finite and positive is
    taken only when the others run out; a segment of at most ``k`` rows gives all of them, then ``-1``.  ``row_id`` (int64 ``[n]``;
    default: the position) is what the generator knows a row by, so a segment's sample depends on its own ``(row_id, weight)`` pairs
    alone.  ``keys`` (int32 ``[n]`` holding the 32-bit patterns) replaces generator and weights; ``return_keys`` also returns the key of
    every row of every segment (int32 ``[n]``, other rows unwritten).

    Without ``weight`` and ``keys``: ``k`` uniform draws with replacement per segment, in draw order.

    ``n``, ``k``, ``seed`` and the counter words are Python integers; the call is enqueued on the current stream and waits for nothing."""
    n, k, seed, c1, c2 = int(n), int(k), int(seed), int(counter[0]), int(counter[1])
    _lib.require_cuda(seg_start, seg_count, weight, row_id, keys)
    device, S = seg_start.device, seg_start.numel()
    if seg_start.dtype != torch.int64 or seg_count.dtype != torch.int64 or seg_start.dim() != 1 or seg_count.shape != seg_start.shape:
        raise ValueError("cap_subset: seg_start and seg_count must be int64 vectors of one length")
    if not (0 <= n <= _lib.CAP_N_MAX and S <= _lib.CAP_S_MAX and 1 <= k <= _lib.CAP_N_MAX and S * k <= _lib.CAP_OUT_MAX):
        raise ValueError(f"cap_subset: need 0 <= n <= {_lib.CAP_N_MAX}, S <= {_lib.CAP_S_MAX}, 1 <= k <= {_lib.CAP_N_MAX} and "
                         f"S k <= {_lib.CAP_OUT_MAX}, got n = {n}, S = {S}, k = {k}")
    for name, t, dtype in (("weight", weight, torch.float32), ("row_id", row_id, torch.int64), ("keys", keys, torch.int32)):
        if t is not None and (t.dtype != dtype or t.shape != (n,)):
            raise ValueError(f"cap_subset: {name} must be a {dtype} tensor of n elements")
    select = weight is not None or keys is not None
    if return_keys and not select:
        raise ValueError("cap_subset: there are no keys without weight or keys (replacement mode)")
    cont = lambda t: None if t is None else t.contiguous()
    seg_start, seg_count, weight, row_id, keys = cont(seg_start), cont(seg_count), cont(weight), cont(row_id), cont(keys)
    with torch.cuda.device(device):
        idx = torch.empty((S, k), dtype=torch.int64, device=device)
        keys_out = torch.empty(n, dtype=torch.int32, device=device) if return_keys else None
        if S > 0:
            ws = _ws("cap_subset", n, S, device=device) if select else None
            check(lib().p2w_cap_subset(n, ptr(seg_start), ptr(seg_count), S, k, ptr(weight), ptr(row_id), seed & 0xffffffffffffffff,
                                       c1 & 0xffffffff, c2 & 0xffffffff, ptr(keys), ptr(idx), ptr(keys_out), ptr(ws),
                                       0 if ws is None else ws.numel(), stream()), "p2w_cap_subset")
    return (idx, keys_out) if return_keys else idx
