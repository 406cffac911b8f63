"""Operator-level reference for the fused PointNetConv (p2w_sa_conv, p2w_sa_conv_h, p2w_sa_conv_h_rows; include/p2w.h).

``make_case`` builds seeded inputs on the CPU, ``reference`` is the exact result (fp32 geometry as the ABI states it, everything
behind it in float64) together with a per-output hard error cap derived from the number formats, ``emulate`` is the same
function with the kernel's arithmetic modelled.  No GPU is needed: tests/test_sa_conv_ref_cpu.py checks this module on its own,
tests/test_gpu_sa_conv.py holds the kernels against it.
"""
import numpy as np
import torch

PRECS = ("f16x3", "fp16", "bf16", "fp32")
PREC_NAME = {0: "f16x3", 1: "fp16", 2: "bf16"}
K_GRAN = {"f16x3": 32, "fp16": 64, "bf16": 64, "fp32": 32}            # K granularity = row pitch granularity of P
U_PREC = {"f16x3": 2.0 ** -20, "fp32": 2.0 ** -20, "fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
DEG_POLICIES = ("mix", "zero", "full", "over", "uniform", "set", "neg", "self", "small", "large")


def round_up(n, g):
    return (n + g - 1) // g * g


def _split(total, B):
    """`total` items over B voxels, unequal (sizes proportional to 1, 2, ..., B), every voxel at least one: CSR pointer [B + 1]."""
    assert total >= B
    w = np.arange(1, B + 1, dtype=np.float64)
    sizes = np.maximum(1, np.floor(total * w / w.sum()).astype(np.int64))
    sizes[-1] += total - sizes.sum()
    while sizes[-1] < 1:                      # the floor of 1 per voxel overdrew the last one: take from the largest
        i = int(np.argmax(sizes))
        sizes[i] -= 1
        sizes[-1] += 1
    return np.concatenate([[0], np.cumsum(sizes)])


def make_case(M, n_src, C1, C2, kw, B=1, seed=0, deg="mix"):
    """Seeded CPU inputs of one call.  All randomness comes from one torch.Generator.

    deg policies: "mix" half the rows full, the others uniform in 0..kw; "zero"; "full"; "over" kw + 5 on a third of the rows
    (the pre-pass clamps it), uniform otherwise; "uniform" 0..kw; "set" only {0, 1, 8, 9, 32} (those <= kw); "neg" uniform with a
    fifth of the valid slots holding -1 (the target's own point stands in) - these four always hold one row without neighbours
    when M >= 3; "self" as mix, but voxel 0's targets list only themselves (dmax = 0); "small" 0..min(8, kw); "large" 9..kw (kw
    itself where kw < 9)."""
    assert deg in DEG_POLICIES and C1 % 4 == 0 and 1 <= kw <= 32
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    nrm = lambda *s: torch.randn(*s, generator=g)
    ri = lambda lo, hi, s: torch.randint(lo, hi, s, generator=g)            # [lo, hi)
    xyzr = torch.cat([rnd(n_src, 3) * 2 - 1, rnd(n_src, 1)], 1).float().contiguous()
    ptr_src, ptr_dst = _split(n_src, B), _split(M, B)
    batch_dst = torch.from_numpy(np.repeat(np.arange(B), np.diff(ptr_dst))).to(torch.int32)
    sf = (1.0 + 2.0 * (torch.randperm(B, generator=g).float() + rnd(B)) / B).float()     # distinct, in [1, 3)
    lo = torch.from_numpy(ptr_src[:-1])[batch_dst.long()]
    n_b = torch.from_numpy(np.diff(ptr_src))[batch_dst.long()]
    idx = (lo + (rnd(M) * n_b).long().clamp(max=n_b - 1)).to(torch.int32)
    nbr = (lo[:, None] + (rnd(M, kw) * n_b[:, None]).long().clamp(max=(n_b - 1)[:, None])).to(torch.int32)
    uni = lambda a, b: ri(a, b + 1, (M,))
    if deg == "mix":
        d = torch.where(rnd(M) < 0.5, torch.full((M,), kw), uni(0, kw))
    elif deg == "zero":
        d = torch.zeros(M, dtype=torch.int64)
    elif deg == "full":
        d = torch.full((M,), kw)
    elif deg == "over":
        d = torch.where(torch.arange(M) % 3 == 1, torch.full((M,), kw + 5), uni(0, kw))
    elif deg in ("uniform", "neg"):
        d = uni(0, kw)
    elif deg == "set":
        vals = torch.tensor([v for v in (0, 1, 8, 9, 32) if v <= kw])
        d = vals[ri(0, len(vals), (M,))]
    elif deg == "self":
        d = torch.where(rnd(M) < 0.5, torch.full((M,), kw), uni(0, kw))
        own = batch_dst == 0
        nbr[own] = idx[own][:, None].expand(-1, kw)
        d[own] = d[own].clamp(min=1)
    elif deg == "small":
        d = uni(0, min(8, kw))
    else:
        d = uni(min(9, kw), kw)
    if deg in ("mix", "uniform", "neg", "over") and M >= 3:
        d[M // 2] = 0                                                        # always one target without neighbours
    if deg == "neg":
        hole = (rnd(M, kw) < 0.2) & (torch.arange(kw)[None, :] < d[:, None])
        nbr[hole] = -1
    P = nrm(n_src, C1).float()
    W1r = (0.5 * nrm(4, C1)).float()
    W2 = (nrm(C2, C1) * (2.0 / C1) ** 0.5).float()
    b2 = (0.1 * nrm(C2)).float()
    bn_s = ((0.6 + 0.9 * rnd(C2)) * torch.where(rnd(C2) < 0.3, -1.0, 1.0)).float()
    bn_s[int(ri(0, C2, (1,)))] = 0.0
    bn_t = (0.2 * nrm(C2)).float()
    return dict(M=M, n_src=n_src, C1=C1, C2=C2, kw=kw, B=B, seed=seed, policy=deg, xyzr=xyzr, ptr_src=torch.from_numpy(ptr_src),
                ptr_dst=torch.from_numpy(ptr_dst), batch_dst=batch_dst, sf=sf, idx=idx, nbr=nbr.contiguous(), deg=d.to(torch.int32),
                P=P, W1r=W1r, W2=W2, b2=b2, bn_s=bn_s, bn_t=bn_t)


def padded_P(case, prec, rows=None):
    """P as the H entry points take it: [n_src + 1, ldp], ldp = round_up(C1, K granularity of `prec`), zero pad columns, and row
    n_src prefilled with 1.0 (the call must zero it).  `rows` > n_src + 1 gives a larger allocation (more 1.0 rows behind)."""
    n_src, C1 = case["n_src"], case["C1"]
    ldp = round_up(C1, K_GRAN[prec])
    Pp = torch.zeros(max(rows or 0, n_src + 1), ldp)
    Pp[:n_src, :C1] = case["P"]
    Pp[n_src:] = 1.0
    return Pp, ldp


def geometry(case, slot_mask=None):
    """fp32 geometry stage, operations and order as include/p2w.h / sa_edge_meta_kernel state them.
    Returns j [M, kw] (source index per slot, the target's own point for a negative entry), g [M, kw, 4] fp32, valid [M, kw]."""
    kw, M = case["kw"], case["M"]
    xyzr, own = case["xyzr"], case["idx"].long()
    d = case["deg"].long().clamp(max=kw)
    valid = torch.arange(kw)[None, :] < d[:, None]
    if slot_mask is not None:
        valid = valid & slot_mask
    j = case["nbr"].long()
    j = torch.where(j < 0, own[:, None].expand(-1, kw), j)
    j = torch.where(valid, j, own[:, None].expand(-1, kw))
    s = case["sf"][case["batch_dst"].long()].float()[:, None, None]
    pj, pi = xyzr[j], xyzr[own][:, None, :]
    rel = pj[..., :3] / s - pi[..., :3] / s
    x, y, z = rel[..., 0], rel[..., 1], rel[..., 2]
    nrm = torch.sqrt(((x * x) + (y * y)) + (z * z))
    nrm = torch.where(valid, nrm, torch.zeros_like(nrm))
    dmax = nrm.max(dim=1).values if kw else torch.zeros(M)
    den = dmax + torch.tensor(1e-8, dtype=torch.float32)
    g = torch.cat([rel / den[:, None, None], pj[..., 3:4]], dim=-1)
    g = torch.where(valid[..., None], g, torch.zeros_like(g))
    return j, g.float(), valid


def _masked_max(y, valid):
    """max over the valid slots of y [M, kw, C2]; rows without a valid slot give 0."""
    neg = torch.full_like(y, -float("inf"))
    m = torch.where(valid[..., None], y, neg).max(dim=1).values
    return torch.where(valid.any(dim=1)[:, None], m, torch.zeros_like(m))


def cap_constant(prec, C1):
    """Relative error of one output against sum_k |a_k| |w_k|: two operand roundings (u_prec), the fp32 layer-1 chain (2^-21) and
    a linear fp32 accumulation over the padded K (round_up(C1) * 2^-24)."""
    return U_PREC[prec] + 2.0 ** -21 + round_up(C1, K_GRAN[prec]) * 2.0 ** -24


def reference(case, prec="f16x3"):
    """(exact result [M, C2] float64, hard cap [M, C2] float64 for `prec`).  Geometry in fp32, everything after it in float64.
    cap[slot, n] = c(prec, C1) * (sum_k A_k |W2[n, k]| + |b2[n]|) * |bn_s[n]| + 1e-6 |bn_t[n]| with A_k = |P[j, k]| + sum_c |g_c|
    |W1r[c, k]| >= |pre-ReLU value|; ReLU is 1-Lipschitz and |max_a - max_b| <= max |a_i - b_i| carries the largest cap of the
    valid slots through the max."""
    j, g, valid = geometry(case)
    Pd, W1, W2 = case["P"].double(), case["W1r"].double(), case["W2"].double()
    b2, s, t = case["b2"].double(), case["bn_s"].double(), case["bn_t"].double()
    pre = Pd[j] + g.double() @ W1
    y = torch.relu(torch.relu(pre) @ W2.t() + b2) * s + t
    ref = _masked_max(y, valid)
    A = Pd[j].abs() + g.double().abs() @ W1.abs()
    cap = cap_constant(prec, case["C1"]) * (A @ W2.abs().t() + b2.abs()) * s.abs() + 1e-6 * t.abs()
    cap = torch.where(valid[..., None], cap, torch.zeros_like(cap)).max(dim=1).values
    return ref, cap


def _f32(x64):
    return x64.float()


def _rtz_half(x):
    """fp16 of fp32 x rounded toward zero, saturating (v_cvt_pkrtz_f16_f32)."""
    h = x.clamp(-65504.0, 65504.0).half()
    over = h.float().abs() > x.abs()
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(torch.float16)


def scaled_w2(case):
    """(W2 * 2^e in float64, 2^-e) with the exponent tests/h_util._pack_h chooses."""
    W2 = case["W2"].double()
    e = int(np.floor(np.log2(1024.0 / float(W2.abs().max()))))
    return W2 * 2.0 ** e, 2.0 ** -e


def emulate(case, prec, drop_a_lo=False, drop_last_slot=False, zero_last_k=0, a_hi="rne"):
    """The result with the kernel's arithmetic modelled ([M, C2] float64 holding fp32 values).
    Layer 1 in fp32 (the kernels' chain of four fused multiply-adds onto P[j]); h1 and W2 * 2^e rounded to the operand format (fp16:
    saturating RNE; bf16: RNE; f16x3: hi = half(x), lo = half(x - hi), products lo*hi + hi*lo + hi*hi); products and sums in fp32
    matmuls; wscale, bias, ReLU and BN in fp32.  "fp32" (p2w_sa_conv): all of it in fp32 on unrounded operands.
    The keyword arguments are the mutations tests/test_sa_conv_ref_cpu.py proves the criteria against (drop_a_lo: f16x3 without
    the a_lo * w_hi term; drop_last_slot: the last valid slot of every target masked; zero_last_k: the last k columns of h1
    zeroed) and a_hi = "rtz": the hi plane of h1 rounded toward zero as split_pair does it."""
    kw = case["kw"]
    mask = None
    if drop_last_slot:
        d = case["deg"].long().clamp(max=kw)
        mask = torch.arange(kw)[None, :] < (d - 1)[:, None]
    j, g, valid = geometry(case)             # dmax from all valid slots (the pre-pass is not what the mutation breaks)
    if mask is not None:
        valid = valid & mask
    W1 = case["W1r"].double()
    v = case["P"][j]                                                         # [M, kw, C1] fp32
    for c in range(4):                                                       # fmaf(g_c, w_c, v): exact product, one rounding
        v = _f32(g[..., c:c + 1].double() * W1[c] + v.double())
    h1 = torch.relu(v)
    if zero_last_k:
        h1 = h1.clone()
        h1[..., case["C1"] - zero_last_k:] = 0.0
    b2, s, t = case["b2"], case["bn_s"], case["bn_t"]
    if prec == "fp32":
        acc, wscale = h1 @ case["W2"].t(), 1.0
    else:
        Ws, wscale = scaled_w2(case)
        if prec == "f16x3":
            w_hi = Ws.float().half()
            w_lo = (Ws - w_hi.double()).float().half()
            a_hi_ = _rtz_half(h1) if a_hi == "rtz" else h1.clamp(-65504.0, 65504.0).half()
            a_lo = (h1 - a_hi_.float()).half()
            acc = a_hi_.float() @ w_lo.float().t() + a_hi_.float() @ w_hi.float().t()
            if not drop_a_lo:
                acc = a_lo.float() @ w_hi.float().t() + acc
        elif prec == "fp16":
            acc = h1.clamp(-65504.0, 65504.0).half().float() @ Ws.float().half().float().t()
        else:
            acc = h1.bfloat16().float() @ Ws.float().bfloat16().float().t()
    y = torch.relu(acc * torch.tensor(wscale, dtype=torch.float32) + b2) * s + t
    return _masked_max(y, valid).double()


def rms(x):
    return float(torch.sqrt(torch.mean(x.double() ** 2))) if x.numel() else 0.0


def rows_with_neighbours(case):
    return case["deg"].long().clamp(max=case["kw"]) > 0
