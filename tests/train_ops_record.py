"""What the host code of the training operators does, recorded: for ``global_max_pool``, ``edge_layer1``, ``relu_bn_max``, ``bn_chain``,
``relu_bn``, ``interp_add_relu`` and ``bn_relu_rowdot`` of ``pointstowood_amd.ops``, case by case, the bits that come out, what is
saved for the backward and what a refusal says (tests/golden/train_ops_host.json, compared by tests/test_gpu_train_ops_host.py).

A case calls the public operator on small inputs drawn from a seeded CPU ``torch.Generator`` - no GEMM is involved: the operators' own
kernels give the same bits on every run - and records

    out        sha256 over dtype, shape and bytes of the output
    grads      one sha256 over dtype, shape and bytes of every input's and every parameter's gradient, in order (a missing one as None)
    stats      one sha256 over ``running_mean`` / ``running_var`` of every BatchNorm1d afterwards;  nbt: their ``num_batches_tracked``
    grad_fn    the class name of the output's ``grad_fn``
    saved      "shape:dtype" of every tensor saved for the backward, in order (``torch.autograd.graph.saved_tensors_hooks``)
    saved_bits one sha256 over those tensors: mean / invstd, the winners' tables and the saved z itself

or, where the operator refuses: the exception's type and message, and whether the statistics and counters stood still.  An eval-mode
case records the output's shape and dtype and that nothing moved (its arithmetic is PyTorch's own).  The hashes are cut to ``HEX`` hex
digits (80 bits) to keep the fixture small.

Sizes: 67 rows (above P2W_BN_CHAIN_ROWS = 32 and P2W_BN_GROUP = 16: more than one work item) at C = 8 (16-byte accesses) and C = 7
(4-byte accesses); ``edge_layer1`` on 301 edges from 40 sources to 23 targets, one of them without edges, C1 = 8; k = 3.  ``view``
passes ``z[1:]`` of a tensor with one more row - at C = 7 it starts off a 16-byte boundary, the view that ``_lib.aligned16`` copies -
and ``transposed`` a ``z`` whose memory is [C, rows].  16-bit cases run under autocast of their dtype with ``ops.half_io`` on and off.

Re-record (from the commit whose behaviour is the reference, on an MI355X):  python -m tests.train_ops_record <its commit>
"""
import contextlib
import hashlib
import json
import os
import sys

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_ops_host.json")
HEX = 20
ROWS = 67
F16, BF16 = torch.float16, torch.bfloat16
# name -> (dtype of the big input and of autocast; None: fp32, no autocast), ops.half_io
ROUTES = {"f32": (None, True), "f16-on": (F16, True), "f16-off": (F16, False), "bf16-on": (BF16, True), "bf16-off": (BF16, False)}
LAYOUTS = ("plain", "view", "transposed")


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _digest(named):
    h = hashlib.sha256()
    for name, t in named:
        if t is None:
            h.update(f"{name}:None;".encode())
            continue
        t = t.detach().cpu().contiguous()
        h.update(f"{name}:{_name(t.dtype)}:{tuple(t.shape)};".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:HEX]


def _bns(mods):
    return [m for m in mods if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def _state(mods):
    """(digest of the running statistics, the counters) of every BatchNorm among ``mods``."""
    named, nbt = [], []
    for i, m in enumerate(_bns(mods)):
        named += [(f"{i}.{k}", getattr(m, k)) for k in ("running_mean", "running_var")]
        nbt.append(None if m.num_batches_tracked is None else int(m.num_batches_tracked))
    return _digest(named), nbt


class _Gen:
    """Seeded CPU draws, moved to the device."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.g)

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g)

    def big(self, rows, C, dtype, layout, grad):
        """(leaf, z): z [rows, C] in ``dtype`` (None: fp32) as ``layout`` says, a view of the leaf that gets the gradient."""
        dt = dtype or torch.float32
        if layout == "view":
            leaf = self.randn(rows + 1, C).to(dt).cuda().requires_grad_(grad)
            return leaf, leaf[1:]
        if layout == "transposed":
            leaf = self.randn(C, rows).to(dt).cuda().requires_grad_(grad)
            return leaf, leaf.t()
        leaf = self.randn(rows, C).to(dt).cuda().requires_grad_(grad)
        return leaf, leaf

    def bn(self, C, **kw):
        bn = torch.nn.BatchNorm1d(C, **kw)
        with torch.no_grad():
            if bn.affine:
                bn.weight.copy_(self.randn(C) * 0.5 + 0.6)              # some columns negative: relu_bn_max's minimum side
                bn.bias.copy_(self.randn(C))
            if bn.track_running_stats:
                bn.running_mean.copy_(self.randn(C))
                bn.running_var.copy_(self.rand(C) + 0.5)
        return bn.cuda().train()

    def dw(self, C):
        dw = torch.nn.Conv1d(C, C, 1, groups=C)
        with torch.no_grad():
            dw.weight.copy_(self.randn(C, 1, 1))
            dw.bias.copy_(self.randn(C))
        return dw.cuda()


def _observe(ops, call, leaves, mods, route, grad, seed, eval_mode=False):
    """The record of one call: ``call()`` runs the operator on prepared inputs; ``leaves`` get gradients, ``mods`` hold parameters and
    statistics."""
    dtype, half_io = ROUTES[route]
    saved, saved_named = [], []

    def pack(t):
        saved.append(f"{'x'.join(map(str, t.shape))}:{_name(t.dtype)}")
        saved_named.append((str(len(saved_named)), t))
        return t

    before = _state(mods)
    old, ops.half_io = ops.half_io, half_io
    try:
        with contextlib.ExitStack() as stack:
            if dtype is not None:
                stack.enter_context(torch.autocast("cuda", dtype=dtype))
            if not grad:
                stack.enter_context(torch.no_grad())
            if not eval_mode:
                stack.enter_context(torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t))
            out = call()
    except Exception as e:  # the refusal is the record
        return {"raises": type(e).__name__, "message": str(e), "state_unchanged": _state(mods) == before}
    finally:
        ops.half_io = old
    if eval_mode:
        return {"out_like": [list(out.shape), _name(out.dtype)], "state_unchanged": _state(mods) == before}
    rec = {"out": _digest([("out", out)]), "grad_fn": None if out.grad_fn is None else type(out.grad_fn).__name__,
           "saved": saved, "saved_bits": _digest(saved_named)}
    if grad:
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 1)).to(out.dtype).cuda()
        out.backward(cot)
        params = [p for m in mods for p in m.parameters()]
        rec["grads"] = _digest([(str(i), t.grad) for i, t in enumerate((*leaves, *params))])
    rec["stats"], rec["nbt"] = _state(mods)
    return rec


# ------------------------------------------------------------------------------------------------ the operators' cases
def _seed(*key):
    return int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little")


def _pool(ops, route, C, layout, grad):
    seed = _seed("pool", C, layout)
    g = _Gen(seed)
    leaf, x = g.big(ROWS, C, ROUTES[route][0], layout, grad)
    batch = torch.tensor([0] * 20 + [1] * 1 + [3] * 30 + [4] * 16).cuda()          # segment 2 is empty
    return _observe(ops, lambda: ops.global_max_pool(x, batch, size=5), [leaf], [], route, grad, seed)


EDGE = dict(n_src=40, M=23, C1=8, empty=5)


def _edge_inputs(g):
    i = torch.randint(0, EDGE["M"], (301,), generator=g.g)
    i = torch.where(i == EDGE["empty"], i + 1, i).sort().values                     # grouped by target; one target without edges
    j = torch.randint(0, EDGE["n_src"], (301,), generator=g.g)
    return torch.stack([j, i]).cuda(), g.rand(EDGE["n_src"], 4), g.rand(EDGE["M"], 4).cuda()


def _edge(ops, route, out, layout, grad):
    seed = _seed("edge", layout)
    g = _Gen(seed)
    edge_index, pos_src, pos_dst = _edge_inputs(g)
    dtype, (n, C1) = ROUTES[route][0], (EDGE["n_src"], EDGE["C1"])
    p_leaf, P = g.big(n, C1, dtype, layout, grad)
    if layout == "plain":
        w_leaf = g.randn(4, C1).cuda().requires_grad_(grad)
        Wg = w_leaf
    else:                                                     # as PointNetConv passes it: the transposed slice of W1
        w_leaf = g.randn(C1, 4).cuda().requires_grad_(grad)
        Wg = w_leaf.t()
    pos_src = pos_src.cuda().requires_grad_(grad)
    out_dtype = {"none": None, "f16": F16, "bf16": BF16}[out]
    return _observe(ops, lambda: ops.edge_layer1(P, Wg, pos_src, pos_dst, edge_index, out_dtype=out_dtype), [p_leaf, w_leaf, pos_src], [], route,
                    grad, seed)


def _index():
    return torch.repeat_interleave(torch.arange(9), torch.tensor([8, 1, 0, 20, 5, 9, 2, 15, 7])).cuda()      # target 2 has no rows


def _bn_max(ops, route, C, layout, grad):
    seed = _seed("bn_max", C, layout)
    g = _Gen(seed)
    leaf, z = g.big(ROWS, C, ROUTES[route][0], layout, grad)
    bn, index = g.bn(C), _index()
    return _observe(ops, lambda: ops.relu_bn_max(z, index, bn, dim_size=9), [leaf], [bn], route, grad, seed)


def _chain_stages(g, C, L, dw):
    """L stages, ReLU - none - ReLU, the last one behind a depthwise convolution where ``dw``."""
    bns = [g.bn(C) for _ in range(L)]
    conv = g.dw(C) if dw else None
    stages = [(bn, t % 2 == 0) if not (dw and t == L - 1) else (bn, t % 2 == 0, conv) for t, bn in enumerate(bns)]
    return stages, bns + ([conv] if dw else [])


def _chain(ops, route, C, L, dw, res, out, layout, grad):
    seed = _seed("chain", C, L, dw, res, layout)
    g = _Gen(seed)
    dtype = ROUTES[route][0]
    leaf, z = g.big(ROWS, C, dtype, layout, grad)
    stages, mods = _chain_stages(g, C, L, dw)
    residual = g.randn(ROWS, C).cuda().requires_grad_(grad) if res else None
    out_dtype = {"none": None, "f32": torch.float32, "own": dtype}[out]
    return _observe(ops, lambda: ops.bn_chain(z, stages, residual=residual, out_dtype=out_dtype), [leaf] + ([residual] if res else []), mods,
                    route, grad, seed)


def _relu_bn(ops, route, C, out, layout, grad):
    seed = _seed("relu_bn", C, layout)
    g = _Gen(seed)
    dtype = ROUTES[route][0]
    leaf, z = g.big(ROWS, C, dtype, layout, grad)
    bn = g.bn(C)
    out_dtype = {"none": None, "f32": torch.float32, "own": dtype}[out]
    return _observe(ops, lambda: ops.relu_bn(z, bn, out_dtype=out_dtype), [leaf], [bn], route, grad, seed)


def _interp(ops, route, C, layout, grad):
    seed = _seed("interp", C, layout)
    g = _Gen(seed)
    dtype, n_c = ROUTES[route][0], 20
    s_leaf, S = g.big(ROWS, C, dtype, layout, grad)
    p_leaf, Pc = g.big(n_c, C, dtype, layout, grad)
    pos_x, pos_y = g.rand(n_c, 3).cuda(), g.rand(ROWS, 3).cuda()
    return _observe(ops, lambda: ops.interp_add_relu(Pc, S, pos_x, pos_y, k=3), [p_leaf, s_leaf], [], route, grad, seed)


def _head(ops, route, C, layout, grad, conv_weight=True):
    seed = _seed("head", C, layout)
    g = _Gen(seed)
    leaf, z = g.big(ROWS, C, ROUTES[route][0], layout, grad)
    bn = g.bn(C)
    weight = g.randn(*((1, C, 1) if conv_weight else (1, C))).cuda().requires_grad_(grad)
    bias = g.randn(1).cuda().requires_grad_(grad)
    return _observe(ops, lambda: ops.bn_relu_rowdot(z, bn, weight, bias), [leaf, weight, bias], [bn], route, grad, seed)


# ------------------------------------------------------------------------------------------------ refusals and eval mode
def _refusals(ops):
    """name -> record of every refusal: wrong module, the BatchNorm1d variants nobody builds, one row, a width that is not the
    module's, a wrong ``out_dtype``, a residual with a 16-bit ``out_dtype``, a wrong weight shape."""
    C, out = 8, {}
    g = _Gen(_seed("refusals"))
    z = g.randn(ROWS, C).cuda().requires_grad_()
    zh = z.detach().half().requires_grad_()
    index = _index()
    w, b = g.randn(1, C, 1).cuda(), g.randn(1).cuda()
    calls = {
        "relu_bn_max": lambda zz, bn, **kw: ops.relu_bn_max(zz, index[:zz.shape[0]], bn, dim_size=9),
        "bn_chain": lambda zz, bn, **kw: ops.bn_chain(zz, [(bn, True)], **kw),
        "relu_bn": lambda zz, bn, **kw: ops.relu_bn(zz, bn, **kw),
        "bn_relu_rowdot": lambda zz, bn, **kw: ops.bn_relu_rowdot(zz, bn, kw.get("weight", w), b),
    }
    variants = {
        "module": lambda: torch.nn.LayerNorm(C).cuda(),
        "affine": lambda: g.bn(C, affine=False),
        "momentum": lambda: g.bn(C, momentum=None),
        "no_stats": lambda: g.bn(C, track_running_stats=False),
        "width": lambda: g.bn(C + 1),
    }
    for op, call in calls.items():
        for v, make in variants.items():
            bn = make()
            out[f"{op}-{v}"] = _observe(ops, lambda: call(z, bn), [], [bn], "f32", True, 0)
        bn = g.bn(C)
        out[f"{op}-one_row"] = _observe(ops, lambda: call(z[:1], bn), [], [bn], "f32", True, 0)
        out[f"{op}-one_row-f16"] = _observe(ops, lambda: call(zh[:1], bn), [], [bn], "f16-on", True, 0)
        out[f"{op}-three_dims"] = _observe(ops, lambda: call(z[None], bn), [], [bn], "f32", True, 0)
    for op in ("bn_chain", "relu_bn"):
        bn = g.bn(C)
        for v, kw, zz, route in (("out_f64", dict(out_dtype=torch.float64), z, "f32"), ("out_f16_of_f32", dict(out_dtype=F16), z, "f32"),
                                 ("out_bf16_of_f16", dict(out_dtype=BF16), zh, "f16-on"), ("out_f16_of_f32-off", dict(out_dtype=F16), z, "f16-off")):
            out[f"{op}-{v}"] = _observe(ops, lambda: calls[op](zz, bn, **kw), [], [bn], route, True, 0)
    bn, bn2 = g.bn(C), g.bn(C)
    res = g.randn(ROWS, C).cuda()
    for route in ("f16-on", "f16-off"):
        out[f"bn_chain-residual_f16-{route}"] = _observe(ops, lambda: ops.bn_chain(zh, [(bn, True)], residual=res, out_dtype=F16), [], [bn], route,
                                                         True, 0)
    out["bn_chain-residual_shape"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True)], residual=res[1:]), [], [bn], "f32", True, 0)
    out["bn_chain-no_stage"] = _observe(ops, lambda: ops.bn_chain(z, []), [], [bn], "f32", True, 0)
    out["bn_chain-four_stages"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True)] * 4), [], [bn], "f32", True, 0)
    out["bn_chain-second_module"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True), (torch.nn.Identity(), True)]), [], [bn], "f32", True, 0)
    out["bn_chain-second_affine"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True), (g.bn(C, affine=False), True)]), [], [bn], "f32", True, 0)
    bn2.eval()
    out["bn_chain-mixed_modes"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True), (bn2, True)]), [], [bn, bn2], "f32", True, 0)
    out["bn_chain-dw_groups"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True, torch.nn.Conv1d(C, C, 1).cuda())]), [], [bn], "f32", True, 0)
    out["bn_chain-dw_no_bias"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True, torch.nn.Conv1d(C, C, 1, groups=C, bias=False).cuda())]), [],
                                          [bn], "f32", True, 0)
    for v, ww in (("weight_rows", g.randn(2, C).cuda()), ("weight_width", g.randn(1, C + 1).cuda()), ("weight_dims", g.randn(C).cuda())):
        out[f"bn_relu_rowdot-{v}"] = _observe(ops, lambda: calls["bn_relu_rowdot"](z, bn, weight=ww), [], [bn], "f32", True, 0)
    out["bn_relu_rowdot-bias_two"] = _observe(ops, lambda: ops.bn_relu_rowdot(z, bn, w, g.randn(2).cuda()), [], [bn], "f32", True, 0)
    out["relu_bn_max-index_length"] = _observe(ops, lambda: ops.relu_bn_max(z, index[1:], bn, dim_size=9), [], [bn], "f32", True, 0)
    out["relu_bn_max-index_descends"] = _observe(ops, lambda: ops.relu_bn_max(z, index.flip(0), bn, dim_size=9), [], [bn], "f32", True, 0)
    out["relu_bn_max-index_outside"] = _observe(ops, lambda: ops.relu_bn_max(z, index, bn, dim_size=8), [], [bn], "f32", True, 0)
    edge_index, pos_src, pos_dst = _edge_inputs(g)
    P, Wg, pos_src = g.randn(EDGE["n_src"], 8).cuda().requires_grad_(), g.randn(4, 8).cuda(), pos_src.cuda()
    for v, fn in (("out_f32", lambda: ops.edge_layer1(P, Wg, pos_src, pos_dst, edge_index, out_dtype=torch.float32)),
                  ("weight_shape", lambda: ops.edge_layer1(P, Wg.t(), pos_src, pos_dst, edge_index)),
                  ("ungrouped", lambda: ops.edge_layer1(P, Wg, pos_src, pos_dst, edge_index.flip(1))),
                  ("source_outside", lambda: ops.edge_layer1(P[:-1], Wg, pos_src[:-1], pos_dst, torch.stack([edge_index[0].clamp(min=39), edge_index[1]])))):
        out[f"edge_layer1-{v}"] = _observe(ops, fn, [], [], "f32", True, 0)
    Pc, S = g.randn(20, C).cuda().requires_grad_(), g.randn(ROWS, C).cuda()
    pos_x, pos_y = g.rand(20, 3).cuda(), g.rand(ROWS, 3).cuda()
    out["interp_add_relu-k"] = _observe(ops, lambda: ops.interp_add_relu(Pc, S, pos_x, pos_y, k=0), [], [], "f32", True, 0)
    out["interp_add_relu-widths"] = _observe(ops, lambda: ops.interp_add_relu(Pc[:, :4], S, pos_x, pos_y), [], [], "f32", True, 0)
    out["interp_add_relu-rows"] = _observe(ops, lambda: ops.interp_add_relu(Pc, S[1:], pos_x, pos_y), [], [], "f32", True, 0)
    return out


def _evals(ops):
    """Eval mode once per operator with a BatchNorm1d (fp32 and float16 with a 16-bit ``out_dtype`` where there is one)."""
    C, out = 8, {}
    g = _Gen(_seed("evals"))
    z = g.randn(ROWS, C).cuda().requires_grad_()
    zh = z.detach().half().requires_grad_()
    index, w, b = _index(), g.randn(1, C, 1).cuda(), g.randn(1).cuda()
    bn, bn2, dw = g.bn(C).eval(), g.bn(C).eval(), g.dw(C)
    out["relu_bn_max"] = _observe(ops, lambda: ops.relu_bn_max(z, index, bn, dim_size=9), [], [bn], "f32", True, 0, eval_mode=True)
    out["bn_chain"] = _observe(ops, lambda: ops.bn_chain(z, [(bn, True), (bn2, False, dw)], residual=z.detach()), [], [bn, bn2], "f32", True, 0,
                               eval_mode=True)
    out["bn_chain-f16"] = _observe(ops, lambda: ops.bn_chain(zh, [(bn, True), (bn2, False, dw)], out_dtype=F16), [], [bn, bn2], "f16-on", True, 0,
                                   eval_mode=True)
    out["relu_bn"] = _observe(ops, lambda: ops.relu_bn(z, bn), [], [bn], "f32", True, 0, eval_mode=True)
    out["relu_bn-f16"] = _observe(ops, lambda: ops.relu_bn(zh, bn, out_dtype=F16), [], [bn], "f16-on", True, 0, eval_mode=True)
    out["bn_relu_rowdot"] = _observe(ops, lambda: ops.bn_relu_rowdot(z, bn, w, b), [], [bn], "f32", True, 0, eval_mode=True)
    out["relu_bn_max-one_row"] = _observe(ops, lambda: ops.relu_bn_max(z[:1], index[:1], bn, dim_size=9), [], [bn], "f32", True, 0, eval_mode=True)
    return out


# ------------------------------------------------------------------------------------------------ the list
def _outs(route, res=False):
    """The ``out_dtype`` requests of a route: None and - a 16-bit z without a residual - z's own dtype."""
    return ("none",) if route == "f32" or res else ("none", "own")


def _tag(C, lay, grad):
    return f"C{C}-{lay}-{'grad' if grad else 'no_grad'}"


def cases():
    """name -> function of ``ops`` that returns the record."""
    c = {}

    def add(name, fn, *args):
        assert name not in c
        c[name] = lambda ops: fn(ops, *args)

    # both widths with a gradient, one without; z[1:] at both widths (only C = 7 is copied); the transposed z
    combos = [(8, "plain", True), (7, "plain", True), (8, "plain", False), (7, "view", True), (8, "view", True), (7, "transposed", True)]
    for route in ROUTES:
        for C, lay, grad in combos:
            tag = f"{route}-{_tag(C, lay, grad)}"
            add(f"global_max_pool-{tag}", _pool, route, C, lay, grad)
            add(f"relu_bn_max-{tag}", _bn_max, route, C, lay, grad)
            add(f"interp_add_relu-{tag}", _interp, route, C, lay, grad)
            add(f"bn_relu_rowdot-{tag}", _head, route, C, lay, grad)
            for o in _outs(route):
                add(f"relu_bn-out_{o}-{tag}", _relu_bn, route, C, o, lay, grad)
        add(f"relu_bn-out_f32-{route}-{_tag(8, 'plain', True)}", _relu_bn, route, 8, "f32", "plain", True)
        add(f"bn_relu_rowdot-{route}-C8-linear_weight", _head, route, 8, "plain", True, False)
        for o, lay, grad in [(o, "plain", grad) for o in ("none", "f16", "bf16") for grad in (True, False)] + \
                            [("none", "view", True), ("f16", "view", True), ("bf16", "transposed", True)]:
            add(f"edge_layer1-{route}-out_{o}-{lay}-{'grad' if grad else 'no_grad'}", _edge, route, o, lay, grad)
        # bn_chain: every structure at C = 8 with a gradient; three of them without one, at C = 7 and in the other layouts
        for L in (1, 2, 3):
            for dw in (False, True):
                for res in (False, True):
                    for o in _outs(route, res):
                        add(f"bn_chain-{route}-L{L}{'-dw' if dw else ''}{'-res' if res else ''}-out_{o}-{_tag(8, 'plain', True)}", _chain, route, 8,
                            L, dw, res, o, "plain", True)
        add(f"bn_chain-{route}-L2-out_f32-{_tag(8, 'plain', True)}", _chain, route, 8, 2, False, False, "f32", "plain", True)
        for L, dw, res in ((1, False, False), (2, True, True), (3, True, False)):
            o = _outs(route, res)[-1]
            for C, lay, grad in combos[1:]:
                add(f"bn_chain-{route}-L{L}{'-dw' if dw else ''}{'-res' if res else ''}-out_{o}-{_tag(C, lay, grad)}", _chain, route, C, L, dw, res,
                    o, lay, grad)
    return c


GROUPS = {"refusals": _refusals, "evals": _evals}


def record(ops, names=None):
    c = cases()
    return {n: c[n](ops) for n in (names or c)}


def record_all(ops):
    out = {"cases": record(ops)}
    for k, fn in GROUPS.items():
        out[k] = fn(ops)
    return out


if __name__ == "__main__":
    from pointstowood_amd import ops as _ops
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    text = json.dumps({"recorded_from": sys.argv[1], "device": torch.cuda.get_device_name(0), **record_all(_ops)}, sort_keys=True,
                      separators=(",", ":"))
    with open(path, "w") as f:
        f.write(text.replace('},"', '},\n"') + "\n")                  # one record per line
    print("wrote", path)
