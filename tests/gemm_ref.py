"""Operator-level reference for the H GEMM family (p2w_gemm_h2, p2w_gemm_h2_sk, p2w_gemm_h2_rowdot; csrc/p2w_hgemm.h) and, with
prec = "fp32", for p2w_gemm.

``make_case`` builds seeded fp32 inputs on the CPU for one named epilogue class (``EPI_CLASSES``: one entry per compile-time class
of gemm_epilogue_dispatch16, + "all_on" and "none" for the guarded path), ``operands`` gives the exact values the kernel
multiplies - decoded from the H planes, so operand rounding is NOT part of the error that is judged - ``reference`` is the result
in float64 from those operands with a per-element hard cap derived from the number formats, ``emulate`` is the same function with
the kernel's arithmetic modelled (and the mutations tests/test_gemm_ref_cpu.py proves the criteria against).  No GPU is needed:
tests/test_gemm_ref_cpu.py checks this module on its own, tests/test_gpu_gemm.py holds the kernels against it.
"""
from collections import namedtuple

import numpy as np
import torch

from tests import feat_ref as F
from tests.sa_conv_ref import _rtz_half

U = 2.0 ** -24                                   # unit roundoff of fp32
PRECS = (0, 1, 2)
PREC_NAME = dict(F.PREC_NAME)
PREC_NAME["fp32"] = "fp32"
K_ALIGN = {0: 32, 1: 64, 2: 64, "fp32": 32}       # K_pad granularity = K-slab width (HCfg::kalign, p2w_packed_dims)
H_DTYPE = {0: torch.float16, 1: torch.float16, 2: torch.bfloat16}
DOT_B = 0.25

# One epilogue: relu = (relu0, relu1, relu2, relu_final), vectors = (bias, sc0/sh0, sc1/sh1) given or not, residual in (None,
# "f32", "h", "interp"), outputs a subset of ("f32", "h", "dot"), ef = the class word launch_gemm_h computes for it.
Epi = namedtuple("Epi", "relu vectors residual outputs ef")
EPI_CLASSES = {
    "128": Epi((0, 0, 0, 0), (0, 0, 0), None, ("f32",), 128),               # the raw accumulators (x wscale): no epilogue at all
    "129": Epi((1, 0, 0, 0), (1, 0, 0), None, ("f32",), 129),
    "131": Epi((1, 0, 0, 0), (1, 1, 0), None, ("f32",), 131),               # MLP layer 1: Lin + ReLU + BN, fp32 out
    "224": Epi((0, 0, 0, 1), (1, 0, 0), "f32", ("f32",), 224),
    "257": Epi((1, 0, 0, 0), (1, 0, 0), None, ("h",), 257),
    "259": Epi((1, 0, 0, 0), (1, 1, 0), None, ("h",), 259),
    "263": Epi((1, 1, 0, 0), (1, 1, 0), None, ("h",), 263),                 # residual block, expand
    "287": Epi((1, 1, 1, 0), (1, 1, 1), None, ("h",), 287),                 # residual block, second layer: the longest chain
    "387": Epi((1, 0, 0, 0), (1, 1, 0), None, ("f32", "h"), 387),
    "480": Epi((0, 0, 0, 1), (1, 0, 0), "f32", ("f32", "h"), 480),          # residual block, project (single-plane modes)
    "1376": Epi((0, 0, 0, 1), (1, 0, 0), "h", ("h",), 1376),                # ... f16x3: the residual read from an H tensor
    "1504": Epi((0, 0, 0, 1), (1, 0, 0), "h", ("f32", "h"), 1504),
    "2400": Epi((0, 0, 0, 1), (1, 0, 0), "interp", ("h",), 2400),           # FP module layer 0 on the skip columns
    "513": Epi((1, 0, 0, 0), (1, 0, 0), None, ("dot",), 513),               # the head, row-dot kernel only
    "all_on": Epi((1, 1, 1, 1), (1, 1, 1), "f32", ("f32", "h"), 511),       # no class: guarded path everywhere
    "none": Epi((0, 0, 0, 0), (0, 0, 0), None, ("f32", "h"), 384),          # no class either
}
SPECIALISED = frozenset(e.ef for n, e in EPI_CLASSES.items() if n not in ("all_on", "none"))
H_ONLY = tuple(n for n, e in EPI_CLASSES.items() if e.outputs == ("h",))

# The distinct (N, K, class) of the H GEMMs Net(num_classes=1, C=32)'s forward launches in f16x3 (engine.py, the _gemm_h2 call sites
# of _hoist, res_chunk, the global module, fp_chunk and the row-dot head).  FP layer 1 leaves fp32 rows (131) where the next module
# interpolates them and H rows (259) where it hoists or the head follows: both occur, by level size.  The single-plane modes run
# the project layers with an fp32 residual instead (480 with the fp32 output, the guarded path without).
LAYERS_C32 = (
    [(64, 32, "128"), (192, 128, "128"), (384, 256, "128")]                                     # hoisted layer 1 of SA1..3
    + [(E, E // 4, "263") for E in (512, 1024, 2048)] + [(E, E, c) for E in (512, 1024, 2048) for c in ("287", "257")]
    + [(128, 512, "1376"), (256, 1024, "1376"), (512, 2048, "1504")]                            # project (+ fp32 rows at level 3)
    + [(512, 515, "257"), (512, 512, "131")]                                                    # global module
    + [(768, 512, "128"), (768, 512, "2400"), (640, 512, "128"), (640, 256, "2400"), (512, 512, "128"), (512, 128, "2400"),
       (512, 32, "2400")]                                                                       # FP layer 0, hoisted: W_i | W_s
    + [(768, 1024, "257"), (640, 768, "257"), (512, 640, "257"), (512, 544, "257")]             # FP layer 0, not hoisted
    + [(512, 768, "131"), (512, 768, "259"), (512, 640, "131"), (512, 640, "259"), (512, 512, "259")]   # FP layer 1
    + [(512, 512, "513")])                                                                      # conv1 + BN + ReLU + conv2


def round_up(n, g):
    return (n + g - 1) // g * g


def ef_of(relu0=0, sc0=0, relu1=0, sc1=0, relu2=0, residual=None, relu_final=0, out_f32=0, out_h=0, dot=0):
    """The class word of launch_gemm_h: 1 relu0, 2 sc0, 4 relu1, 8 sc1, 16 relu2, 32 residual, 64 relu_final, 128 fp32 out, 256 H
    out, 512 row-dot, 1024 the residual is an H tensor, 2048 it is interpolated.  (The bias is not part of it.)"""
    return ((1 if relu0 else 0) | (2 if sc0 else 0) | (4 if relu1 else 0) | (8 if sc1 else 0) | (16 if relu2 else 0)
            | (32 if residual else 0) | (64 if relu_final else 0) | (128 if out_f32 else 0) | (256 if out_h else 0) | (512 if dot else 0)
            | (1024 if residual == "h" else 0) | (2048 if residual == "interp" else 0))


def ef_of_class(e):
    return ef_of(e.relu[0], e.vectors[1], e.relu[1], e.vectors[2], e.relu[2], e.residual, e.relu[3], "f32" in e.outputs,
                 "h" in e.outputs, "dot" in e.outputs)


# ----------------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------------
def make_case(M, N, K, prec, epi, seed=0):
    """Seeded fp32 inputs of one launch: A [M, round_up(K, 4)] (zero behind K), W [N, K] / sqrt(K), the per-column vectors the
    class takes (scales of both signs), its residual ([M, round_up(N, 4)] fp32, zero behind N; "interp": Z [Mx, N] of a coarser
    level + the interpolation geometry in tests/feat_ref's form, kw = 2, rows of degree 1 and rows ON a coarse point) and, for
    the row-dot class, dot_w.  ldh_a / ldr are the pitches of the H forms tests/h_util._to_h needs (>= columns + 4)."""
    e = EPI_CLASSES[epi]
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    ka = K_ALIGN[prec]
    Kc, Nc = round_up(K, 4), round_up(N, 4)
    A = torch.randn(M, Kc, generator=g)
    A[:, K:] = 0
    W = torch.randn(N, K, generator=g) / K ** 0.5
    vec = lambda: torch.randn(N, generator=g)
    case = dict(M=M, N=N, K=K, prec=prec, epi=epi, seed=seed, A=A, W=W, ldh_a=round_up(Kc + 4, ka), Kpad=round_up(K, ka),
                bias=vec() if e.vectors[0] else None, sc0=vec() if e.vectors[1] else None, sh0=vec() if e.vectors[1] else None,
                sc1=vec() if e.vectors[2] else None, sh1=vec() if e.vectors[2] else None)
    if e.residual in ("f32", "h"):
        R = torch.randn(M, Nc, generator=g)
        R[:, N:] = 0
        case.update(R=R, ldr=round_up(Nc + 4, ka) if e.residual == "h" else Nc)
    elif e.residual == "interp":
        Mx = max(8, M // 4)
        pc, pf = torch.rand(Mx, 4, generator=g), torch.rand(M, 4, generator=g)
        nbr = torch.randint(0, Mx, (M, 2), generator=g, dtype=torch.int32)
        deg = torch.full((M,), 2, dtype=torch.int32)
        deg[::7] = 1
        pf[::11, :3] = pc[nbr[::11, 0].long(), :3]                       # a fine point ON its first neighbour
        Z = torch.randn(Mx, N, generator=g)
        case.update(Z=Z, ldr=N, interp=dict(Fc=N, kw=2, m=M, n_c=Mx, xyzr_c=pc.contiguous(), xyzr_f=pf.contiguous(),
                                             nbr=nbr.contiguous(), deg=deg, xc=Z))
    if "dot" in e.outputs:
        case["dotw"] = vec()
    return case


def pack_w(W, prec):
    """The H weight planes tests/h_util._pack_h writes, on the CPU: (tensor [N_pad, planes * K_pad], wscale = 2^-e, K_pad)."""
    N, K = W.shape
    Np, Kp = round_up(N, 256), round_up(K, K_ALIGN[prec])
    Wp = torch.zeros(Np, Kp, dtype=torch.float64)
    Wp[:N, :K] = W.double()
    e = int(np.floor(np.log2(1024.0 / float(Wp.abs().max()))))
    Ws = Wp * 2.0 ** e
    if prec == 0:
        hi = Ws.float().half()
        lo = (Ws - hi.double()).float().half()
        w = torch.stack([hi.view(Np, Kp // 32, 32), lo.view(Np, Kp // 32, 32)], dim=2).reshape(Np, 2 * Kp)
    else:
        w = Ws.float().to(H_DTYPE[prec])
    return w.contiguous(), 2.0 ** -e, Kp


def decode_planes(t, prec, ldh):
    """(hi, lo) float64 [m, ldh] of a raw H tensor (lo = None for the single-plane modes)."""
    v = t.cpu().double()
    if prec != 0:
        return v[:, :ldh], None
    b = v.view(v.shape[0], ldh // 32, 2, 32)
    return b[:, :, 0].reshape(v.shape[0], ldh), b[:, :, 1].reshape(v.shape[0], ldh)


def _h_of(x, prec, ldh):
    """The raw H tensor the device conversion leaves for fp32 x in rows of pitch ldh (feat_ref.h_planes is pinned bit-equal to it)."""
    return F.h_planes(x, prec, ldh, fill=0.0)


Operands = namedtuple("Operands", "a_hi a_lo w_hi w_lo wscale res")


def operands(case, a_planes=None, r_planes=None, w_planes=None):
    """The exact values the kernel multiplies and adds, as float64: A's planes [M, K_pad] (a_lo = None for one plane), W's
    [N, K_pad], wscale, and the residual [M, N] (fp32 values, the decoded H tensor, or None; the interpolated one is feat_ref's).
    a_planes / r_planes: the raw H tensors the DEVICE produced from the case's fp32 A / R (tests/test_gpu_gemm.py passes them); on
    the CPU feat_ref.h_convert stands in, which tests/test_gpu_feat.py pins bit-equal to the device conversion.  prec "fp32":
    the fp32 values themselves."""
    prec, M, N, K, Kp = case["prec"], case["M"], case["N"], case["K"], case["Kpad"]
    e = EPI_CLASSES[case["epi"]]
    if prec == "fp32":
        a = torch.zeros(M, Kp, dtype=torch.float64)
        a[:, :K] = case["A"][:, :K].double()
        w = torch.zeros(N, Kp, dtype=torch.float64)
        w[:, :K] = case["W"].double()
        res = case["R"][:, :N].double() if e.residual == "f32" else None
        return Operands(a, None, w, None, 1.0, res)
    if a_planes is None:
        a_planes = _h_of(case["A"], prec, case["ldh_a"])
    a_hi, a_lo = decode_planes(a_planes, prec, case["ldh_a"])
    assert float(a_hi[:, K:].abs().max() if a_hi.shape[1] > K else 0.0) == 0.0           # K padding must be zero in A
    a_hi, a_lo = a_hi[:, :Kp], (None if a_lo is None else a_lo[:, :Kp])
    if w_planes is None:
        w_planes, wscale, _ = pack_w(case["W"], prec)
    else:
        wscale = pack_w(case["W"], prec)[1]
    w_hi, w_lo = decode_planes(w_planes[:N], prec, Kp)
    res = None
    if e.residual == "f32":
        res = case["R"][:, :N].double()
    elif e.residual == "h":
        if r_planes is None:
            r_planes = _h_of(case["R"], prec, case["ldr"])
        r_hi, r_lo = decode_planes(r_planes, prec, case["ldr"])
        res = (r_hi if r_lo is None else r_hi + r_lo)[:, :N]
    return Operands(a_hi, a_lo, w_hi, w_lo, wscale, res)


# ----------------------------------------------------------------------------------------------------------------------------
# reference and cap
# ----------------------------------------------------------------------------------------------------------------------------
def acc_terms(case):
    """Roundings behind one accumulator: one addition per product and padded k (f16x3: three products per k; the fp32 engine: the
    product of two fp32 values rounds as well)."""
    return {0: 3, "fp32": 2}.get(case["prec"], 1) * case["Kpad"]


def _gamma(n):
    return n * U / (1.0 - n * U)


def nslices(N):
    return (N + 63) // 64


def reference(case, ops=None):
    """(ref, cap): the launch's result in float64 from the operands the kernel sees, and a hard bound on |kernel - ref| per
    element of the fp32 output ([M, N]; the row-dot class: [M]).

    Accumulator.  The kernel adds, in fp32 and in an order this bound does not assume, the products a_lo w_hi, a_hi w_lo, a_hi
    w_hi (one product per k in the single-plane modes) over the padded K: every product of two 11-bit (8-bit) significands is
    exact in fp32 (the fp32 engine's rounds: two roundings per k there), every addition rounds once (u = 2^-24) on a partial sum of at most sum_k |a_k| |w_k|, so the sum is within
    gamma_n sum |a||w|, n = acc_terms(case), gamma_n = n u / (1 - n u) (linear, worst case).  f16x3 omits a_lo w_lo: A's hi plane
    is truncated (|a_lo| <= 2^-10 |a|), W's is rounded to nearest (|w_lo| <= 2^-11 |w|): at most 2^-21 sum |a||w|.  With
    S = wscale sum_k |a_k||w_k| (wscale is a power of two: exact): e_acc = (gamma_n + 2^-21 [f16x3]) S.
    Epilogue (value() of gemm_epilogue_16, fp32, contraction off).  Each statement maps an input within e of its exact value v_in
    to an output within L e (1 + u) + u |v_out| of the exact v_out: L = 1 for fmaf(acc, wscale, bias) and the ReLUs (which round
    nothing), L = |sc| for fmaf(v, sc, sh), and the residual adds its own error e_res and one rounding.  Without a bias pointer
    the first statement adds 0: exact.  e_res = 0 for an fp32 or H residual (hi + lo is exact in fp32), (2 d + 14) u sum_s a_s
    |z_s| for the interpolated one (feat_ref.interp_reference: the records of p2w_interp_weights carry (2 d + 12) u, the
    epilogue's a0 z0 and fmaf(a1, z1, .) two more roundings).
    Row-dot: out_i = sum_c v_ic dw_c + b, a chain of four fmaf per lane and 64-column slice, four butterfly levels, the slices
    added in order, then b: at most 8 + slices roundings on partial sums of at most T = sum_c |v_ic dw_c| + |b| (the bound of
    feat_ref.rowdot_reference with this kernel's chain lengths), plus the elements' own errors: sum_c e_ic |dw_c| + gamma (T + sum_c
    e_ic |dw_c|)."""
    ops = operands(case) if ops is None else ops
    e = EPI_CLASSES[case["epi"]]
    prec = case["prec"]
    a = ops.a_hi if ops.a_lo is None else ops.a_hi + ops.a_lo
    w = ops.w_hi if ops.w_lo is None else ops.w_hi + ops.w_lo
    v = (a @ w.t()) * ops.wscale
    S = (a.abs() @ w.abs().t()) * ops.wscale
    err = (_gamma(acc_terms(case)) + (2.0 ** -21 if prec == 0 else 0.0)) * S
    d = lambda t: t.double()[None, :]

    def step(v_out, L):
        nonlocal v, err
        err = L * err * (1 + U) + U * v_out.abs()
        v = v_out
    if case["bias"] is not None:
        step(v + d(case["bias"]), 1.0)
    if e.relu[0]:
        v = torch.relu(v)
    if case["sc0"] is not None:
        step(v * d(case["sc0"]) + d(case["sh0"]), d(case["sc0"]).abs())
    if e.relu[1]:
        v = torch.relu(v)
    if case["sc1"] is not None:
        step(v * d(case["sc1"]) + d(case["sh1"]), d(case["sc1"]).abs())
    if e.relu[2]:
        v = torch.relu(v)
    if e.residual == "interp":
        res, e_res = F.interp_reference(case["interp"])
        err = err + e_res
        step(v + res, 1.0)
    elif e.residual:
        step(v + ops.res, 1.0)
    if e.relu[3]:
        v = torch.relu(v)
    if "dot" not in e.outputs:
        return v, err
    dw = case["dotw"].double()
    b = float(np.float32(DOT_B))
    own = err @ dw.abs()
    T = v.abs() @ dw.abs() + abs(b)
    return v @ dw + b, own + _gamma(8 + nslices(case["N"])) * (T + own)


def h_cap(case, ref, cap):
    """Bound on |decoded H output - ref| for a launch that leaves only the H form: the cap plus the conversion's half ulp of the
    fp32 value v (|v| <= |ref| + cap): f16x3 lo = nearest fp16 of a remainder below one ulp of the truncated hi: 2^-21 |v|;
    fp16 2^-11 |v| (11 significant bits); bf16 2^-8 |v| (8); + 2^-25, half the spacing of fp16's subnormals."""
    rel = {0: 2.0 ** -21, 1: 2.0 ** -11, 2: 2.0 ** -8}[case["prec"]]
    return cap + rel * (ref.abs() + cap) + 2.0 ** -25


# ----------------------------------------------------------------------------------------------------------------------------
# emulation
# ----------------------------------------------------------------------------------------------------------------------------
def _rtz_bf16(x):
    bits = x.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).bfloat16()


def h_output(v, prec, truncate=False):
    """The 16-bit plane(s) of the epilogue's fp32 values (split_pair / pack_pair).  truncate: the mutation - a plane the kernel
    rounds to nearest (f16x3 lo, fp16, bf16) rounded toward zero instead."""
    if not truncate:
        return F.h_convert(v, prec)
    v = v.float()
    if prec == 0:
        h = _rtz_half(v)
        return h, _rtz_half(v - h.float())
    return (_rtz_half(v),) if prec == 1 else (_rtz_bf16(v),)


Emulated = namedtuple("Emulated", "v h")


def emulate(case, ops=None, drop_a_lo=False, drop_a_lo_from_k=None, zero_k=None, zero_block=(0, 0), skip_relu=None,
            neighbour_column_params=False, next_row_residual=False, h_truncate=False):
    """Emulated(v, h): the fp32 result (as float64; [M, N], the row-dot class [M]) with the kernel's arithmetic modelled, and the H
    planes of it where the class writes an H output.  fp32 matmuls over the decoded planes, f16x3 in the kernel's order a_lo w_hi,
    a_hi w_lo, a_hi w_hi (each a matmul of its own, added in fp32), the epilogue statement by statement with feat_ref._fma.
    Mutations: drop_a_lo (the whole a_lo w_hi term), drop_a_lo_from_k = k0 (lost from column k0 on: the last slab), zero_k =
    (k0, k1) (these k missing in the 16 x 32 block zero_block of the output only), skip_relu = i (0, 1, 2; 3 = the final one),
    neighbour_column_params (bias / scales / dot_w of column c ^ 1), next_row_residual (row r adds row r + 1's), h_truncate."""
    ops = operands(case) if ops is None else ops
    e = EPI_CLASSES[case["epi"]]
    prec, M, N = case["prec"], case["M"], case["N"]
    f = lambda t: t.float()
    if prec == "fp32":
        acc = f(ops.a_hi) @ f(ops.w_hi).t()
    elif prec == 0:
        a_lo = f(ops.a_lo).clone()
        if drop_a_lo_from_k is not None:
            a_lo[:, drop_a_lo_from_k:] = 0
        acc = f(ops.a_hi) @ f(ops.w_lo).t()
        if not drop_a_lo:
            acc = a_lo @ f(ops.w_hi).t() + acc
        acc = acc + f(ops.a_hi) @ f(ops.w_hi).t()
    else:
        acc = f(ops.a_hi) @ f(ops.w_hi).t()
    if zero_k is not None:
        rb, cb = zero_block
        rs, cs = slice(16 * rb, min(M, 16 * rb + 16)), slice(32 * cb, min(N, 32 * cb + 32))
        a_cut = f(ops.a_hi if ops.a_lo is None else ops.a_hi + ops.a_lo)[rs].clone()
        a_cut[:, zero_k[0]:zero_k[1]] = 0
        acc = acc.clone()
        acc[rs, cs] = a_cut @ f(ops.w_hi if ops.w_lo is None else ops.w_hi + ops.w_lo)[cs].t()
    swap = (torch.arange(N) ^ 1).clamp(max=N - 1) if neighbour_column_params else torch.arange(N)
    col = lambda name: None if case[name] is None else case[name][swap][None, :]
    relu = [bool(r) and skip_relu != i for i, r in enumerate(e.relu)]
    bias = col("bias")
    v = F._fma(acc, torch.tensor(ops.wscale, dtype=torch.float32), torch.zeros(1, N) if bias is None else bias)
    if relu[0]:
        v = torch.relu(v)
    if case["sc0"] is not None:
        v = F._fma(v, col("sc0"), col("sh0"))
    if relu[1]:
        v = torch.relu(v)
    if case["sc1"] is not None:
        v = F._fma(v, col("sc1"), col("sh1"))
    if relu[2]:
        v = torch.relu(v)
    if e.residual:
        if e.residual == "interp":
            ic = case["interp"]
            _, _, j = F._slots(ic)
            aw = F.interp_weights_emulate(ic)
            n0 = j[:, 0]
            n1 = torch.where(ic["deg"].long() >= 2, j[:, 1], n0)
            res = F._fma(aw[:, 1:2], case["Z"][n1], aw[:, 0:1] * case["Z"][n0])
        else:
            res = f(ops.res)
        if next_row_residual:
            res = torch.roll(res, -1, 0)
        v = v + res
    if relu[3]:
        v = torch.relu(v)
    if "dot" in e.outputs:
        return Emulated(_emulate_dot(v, case["dotw"][swap], N).double(), None)
    return Emulated(v.double(), h_output(v, prec, truncate=h_truncate) if ("h" in e.outputs and prec != "fp32") else None)


def _emulate_dot(v, dw, N):
    """The row-dot epilogue and its finishing pass: per 64-column slice lane c of 16 chains fmaf over columns 2 c, 2 c + 1, 32 + 2 c,
    33 + 2 c of the slice, the DPP butterfly (lane ^ 1, ^ 2, ^ 7, ^ 15) adds the lanes, the slices are added in order, then b."""
    M = v.shape[0]
    Np = round_up(N, 64)
    vp, dp = torch.zeros(M, Np), torch.zeros(Np)
    vp[:, :N], dp[:N] = v, dw
    lanes = torch.arange(16)
    out = torch.zeros(M)
    for s in range(Np // 64):
        acc = torch.zeros(M, 16)
        for off in (0, 1, 32, 33):
            cols = 64 * s + 2 * lanes + off
            acc = F._fma(vp[:, cols], dp[cols][None, :], acc)
        for x in (1, 2, 7, 15):
            acc = acc + acc[:, lanes ^ x]
        out = out + acc[:, 0]
    return out + torch.tensor(DOT_B, dtype=torch.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# criteria
# ----------------------------------------------------------------------------------------------------------------------------
def block_rms(err, br=16, bc=32, min_count=64):
    """(rms [ceil(M / br), ceil(N / bc)] float64, counted [same] bool): RMS of err over the blocks of br rows x bc columns aligned to
    (0, 0) - one MFMA row tile times the column pairs a lane owns in two adjacent column tiles.  Blocks cut by M or N are counted
    when they hold at least min_count elements; the others are covered by the cap only."""
    M, N = err.shape
    nb, mb = (M + br - 1) // br, (N + bc - 1) // bc
    sq = torch.zeros(nb * br, mb * bc, dtype=torch.float64)
    sq[:M, :N] = err.double() ** 2
    one = torch.zeros(nb * br, mb * bc, dtype=torch.float64)
    one[:M, :N] = 1.0
    fold = lambda t: t.view(nb, br, mb, bc).sum(dim=(1, 3))
    cnt = fold(one)
    return torch.sqrt(fold(sq) / cnt.clamp(min=1.0)), cnt >= min_count


def rms_floor(ref, br=16, bc=32):
    """What a block's RMS error is compared against at the least: u / 2 times the block's RMS of |ref| - a result that is the
    correctly rounded fp32 value of the exact sum may already be that far off, whatever the emulation's own summation order
    happened to lose (sums of a few products of short significands are often exact on the CPU)."""
    return 0.5 * U * block_rms(ref, br, bc)[0]
