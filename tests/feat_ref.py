"""Operator-level references for the small feature and geometry kernels (include/p2w.h: p2w_stem*, p2w_interp_concat*,
p2w_interp_weights, p2w_rowdot, p2w_concat_xyz*, p2w_segment_max, p2w_pack_xyzr, p2w_level_gather, p2w_fill_batch_nbr) and for the
fp32 -> H conversion every H producer shares.

Per operator: seeded CPU inputs (``*_case`` / ``*_CASES``: the GPU tests use exactly these), the reference in float64 from the same
fp32 inputs, an emulation - the kernel's statements restated in fp32 on the CPU, one rounding per kernel operation (the library is
built with -ffp-contract=off: a product and a sum round separately unless the source says fmaf) - and a per-element hard cap on
|result - reference|, derived from the roundings (u = 2^-24, the unit roundoff of fp32).  No GPU is needed:
tests/test_feat_ref_cpu.py checks this module on its own, tests/test_gpu_feat.py holds the kernels against it.
"""
import numpy as np
import torch

from tests.sa_conv_ref import _rtz_half

U = 2.0 ** -24
PREC_NAME = {0: "f16x3", 1: "fp16", 2: "bf16"}
K_ALIGN = {0: 32, 1: 64, 2: 64}            # K-slab width = granularity of the zero pad behind an H producer's columns
CLAMP = torch.tensor(1e-16, dtype=torch.float32)   # the interpolation's floor on d2, as the kernels hold it (1e-16f)


def round_up(n, g):
    return (n + g - 1) // g * g


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _fma(a, b, c):
    """fmaf(a, b, c) on fp32 tensors: the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


# ----------------------------------------------------------------------------------------------------------------------------
# fp32 -> H: an exact function of the fp32 value (split_pair / pack_pair / h_store4, p2w_hgemm.h)
# ----------------------------------------------------------------------------------------------------------------------------
def h_convert(v, prec, hi="rtz"):
    """The 16-bit plane(s) of fp32 `v`.  f16x3: (hi, lo), hi = fp16 of v rounded TOWARD ZERO (saturating at +-65504), lo = fp16
    round-to-nearest of the fp32 remainder v - hi (exact in fp32); fp16: round-to-nearest of clamp(v, +-65504); bf16:
    round-to-nearest.  hi = "rne" is the mutation tests/test_feat_ref_cpu.py rejects."""
    v = v.float()
    if prec == 0:
        h = _rtz_half(v) if hi == "rtz" else v.clamp(-65504.0, 65504.0).half()
        return h, (v - h.float()).half()
    if prec == 1:
        return (v.clamp(-65504.0, 65504.0).half(),)
    return (v.bfloat16(),)


def h_planes(v, prec, ldh, hcols=None, fill=3.0, hi="rtz", pad_value=0.0):
    """The raw H tensor [m, planes * ldh] a producer leaves for fp32 values v [m, F] in rows of pitch ldh prefilled with `fill`:
    columns < F = the conversion of v, columns F .. hcols = `pad_value` (zero: the pad up to the K-slab boundary), columns from
    hcols on still `fill`.  The inverse of tests/h_util._from_h: f16x3 rows are blocks of 32 columns stored [hi(32) | lo(32)]."""
    m, F = v.shape
    hcols = ldh if hcols is None else hcols
    assert F <= hcols <= ldh and (prec != 0 or ldh % 32 == 0)
    full = torch.full((m, ldh), float(pad_value), dtype=torch.float32)
    full[:, :F] = v
    keep = (torch.arange(ldh) < hcols)[None, :]
    planes = []
    for p in h_convert(full, prec, hi=hi):
        planes.append(torch.where(keep, p, torch.full_like(p, fill)))
    if prec != 0:
        return planes[0].contiguous()
    return torch.stack([planes[0].view(m, ldh // 32, 32), planes[1].view(m, ldh // 32, 32)], dim=2).reshape(m, 2 * ldh).contiguous()


def same_bits(a, b):
    """16-bit or 32-bit tensors equal bit for bit (NaNs and the sign of zero included)."""
    it = torch.int16 if a.element_size() == 2 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def hcols_of(prec, cols, ldh):
    """Columns a stem / interpolation launch covers in an H row of pitch ldh: its own + the zero pad to the K-slab boundary."""
    return min(ldh, round_up(cols, K_ALIGN[prec]))


# ----------------------------------------------------------------------------------------------------------------------------
# stem: out[i, c] = relu(fma(z, w[c,2], fma(y, w[c,1], fma(x, w[c,0], b[c]))))
# ----------------------------------------------------------------------------------------------------------------------------
STEM_CASES = [(n, C) for n in (1, 255, 1000) for C in (4, 8, 36, 64)]


def stem_case(n, C):
    """Coordinates in [-1, 1] (negatives: ReLU zeros occur), the record's .w = reflectance, must not enter."""
    g = _gen(1000 * n + C)
    xyzr = torch.cat([torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(n, 1, generator=g) + 5.0], 1).float().contiguous()
    w = torch.randn(C, 3, generator=g).float()
    b = (0.3 * torch.randn(C, generator=g)).float()
    return dict(n=n, C=C, xyzr=xyzr, w=w, b=b)


def stem_reference(case):
    """(relu(W xyz + b) in float64, cap).  Cap: three fused multiply-adds, each one rounding of a partial sum that is bounded by
    S = |b| + |x w0| + |y w1| + |z w2| (3 u S to first order, 4 u S with the second-order terms to spare); ReLU is 1-Lipschitz."""
    p, w, b = case["xyzr"][:, :3].double(), case["w"].double(), case["b"].double()
    pre = p @ w.t() + b
    S = p.abs() @ w.abs().t() + b.abs()
    return torch.relu(pre), 4 * U * S


def stem_emulate(case, relu=True):
    p, w, b = case["xyzr"], case["w"], case["b"]
    v = b[None, :].expand(case["n"], -1)
    for a in range(3):
        v = _fma(p[:, a:a + 1], w[None, :, a], v)
    return torch.relu(v) if relu else v


# ----------------------------------------------------------------------------------------------------------------------------
# knn_interpolate (+ concat with the skip features) and its weights alone
# ----------------------------------------------------------------------------------------------------------------------------
INTERP_FC = (4, 24, 256, 260, 512, 516, 1028)     # 256: no fast step; 260: lane 0 only; 512: all lanes, no tail; 516 / 1028: fast steps + tail
INTERP_CASES = [(Fc, 2) for Fc in INTERP_FC] + [(24, 3), (260, 3), (24, 6), (516, 6)]      # (Fc, kw)
INTERP_M, INTERP_NC, INTERP_FS = 601, 150, 8


def interp_case(Fc, kw, m=INTERP_M, n_c=INTERP_NC):
    """Geometry of one interpolation: m fine points over n_c coarse ones, nbr [m, kw] random, deg cycling through 0 .. kw + 1
    (deg > kw: the kernels clamp it).  Rows 5 (mod 16): the query sits ON its first neighbour; 6 (mod 16): on its second; 7 (mod
    16): on both (the two slots name the same coarse point).  skip [m, INTERP_FS] for the calls that concatenate."""
    g = _gen(7 * Fc + kw)
    pc = torch.cat([torch.rand(n_c, 3, generator=g), torch.rand(n_c, 1, generator=g)], 1).float().contiguous()
    pf = torch.cat([torch.rand(m, 3, generator=g), torch.rand(m, 1, generator=g)], 1).float().contiguous()
    nbr = torch.randint(0, n_c, (m, kw), generator=g, dtype=torch.int32)
    deg = (torch.arange(m) % (kw + 2)).to(torch.int32)
    r = torch.arange(m)
    on0, on1, both = r % 16 == 5, (r % 16 == 6) & (kw >= 2), (r % 16 == 7) & (kw >= 2)
    deg[on0 | on1 | both] = kw
    pf[on0, :3] = pc[nbr[on0, 0].long(), :3]
    if kw >= 2:
        pf[on1, :3] = pc[nbr[on1, 1].long(), :3]
        nbr[both, 1] = nbr[both, 0]
        pf[both, :3] = pc[nbr[both, 0].long(), :3]
    xc = torch.randn(n_c, Fc, generator=g).float()
    skip = torch.randn(m, INTERP_FS, generator=g).float()
    return dict(Fc=Fc, kw=kw, m=m, n_c=n_c, xyzr_c=pc, xyzr_f=pf.contiguous(), nbr=nbr.contiguous(), deg=deg, xc=xc, skip=skip,
                on0=on0, on1=on1, both=both)


def _slots(case):
    kw = case["kw"]
    d = case["deg"].long().clamp(max=kw)
    valid = torch.arange(kw)[None, :] < d[:, None]
    j = torch.where(valid, case["nbr"].long(), torch.zeros_like(case["nbr"].long()))
    return d, valid, j


def interp_d2_f64(case):
    """Squared distances [m, kw] in float64 from the fp32 coordinates (invalid slots: inf)."""
    d, valid, j = _slots(case)
    diff = case["xyzr_c"][j][..., :3].double() - case["xyzr_f"][:, None, :3].double()
    d2 = (diff * diff).sum(-1)
    return torch.where(valid, d2, torch.full_like(d2, float("inf")))


def interp_weights_f64(case):
    """a [m, kw] float64: w_s / sum_s w_s with w_s = 1 / max(d2, 1e-16f) over the valid slots, 0 elsewhere."""
    d, valid, j = _slots(case)
    w = torch.where(valid, 1.0 / torch.maximum(interp_d2_f64(case), CLAMP.double()), torch.zeros(1, dtype=torch.float64))
    den = w.sum(1, keepdim=True)
    return torch.where(den > 0, w / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(w))


def interp_reference(case):
    """(sum_s a_s x_s in float64 [m, Fc], cap [m, Fc]).  Cap (2 d + 14) u sum_s a_s |x_s| for a row of degree d: a weight carries
    <= 6 u relative (each difference u, so each square 3 u, their two sums u each, the division u), each product w x one
    more u, the numerator's and the denominator's sums of d terms (d - 1) u each, the final division u:
    6 + 6 (the denominator's weights) + 1 + 2 (d - 1) + 1 = 2 d + 12, and 2 u for the second-order terms.  d = 0: exactly 0."""
    d, valid, j = _slots(case)
    a = interp_weights_f64(case)
    x = case["xc"].double()[j]                                        # [m, kw, Fc]
    ref = (a[..., None] * x).sum(1)
    cap = (2 * d[:, None] + 14).double() * U * (a[..., None] * x.abs()).sum(1)
    return ref, cap


def _emu_weights(case, clamp=True, inv_d=False):
    """fp32 w [m, kw] (0 on invalid slots) as the kernels compute it: dx, dy, dz, d2 = ((dx dx) + (dy dy)) + (dz dz), 1 / max(d2, 1e-16f)."""
    d, valid, j = _slots(case)
    diff = case["xyzr_c"][j][..., :3] - case["xyzr_f"][:, None, :3]
    dx, dy, dz = diff[..., 0], diff[..., 1], diff[..., 2]
    d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
    if inv_d:
        d2 = torch.sqrt(d2)
    if clamp:
        d2 = torch.maximum(d2, CLAMP)
    w = torch.tensor(1.0, dtype=torch.float32) / d2
    return torch.where(valid, w, torch.zeros_like(w)), valid, j


def interp_emulate(case, clamp=True, inv_d=False, stale_den=False):
    """Products and sums in slot order from 0, then a literal division - all fp32.  Mutations: clamp = False (no floor on d2),
    inv_d (1 / d for 1 / d2), stale_den (row q divides by the denominator of row q - 1)."""
    w, valid, j = _emu_weights(case, clamp, inv_d)
    x = case["xc"][j]
    num = torch.zeros(case["m"], case["Fc"])
    den = torch.zeros(case["m"])
    for s in range(case["kw"]):
        num = torch.where(valid[:, s:s + 1], num + x[:, s] * w[:, s:s + 1], num)
        den = torch.where(valid[:, s], den + w[:, s], den)
    if stale_den:
        den = torch.roll(den, 1)
    has = valid.any(1)[:, None]
    return torch.where(has, num / den[:, None], torch.zeros_like(num))


def interp_weights_reference(case):
    """For kw <= 2: (n0, n1 [m] int, a [m, 2] float64, relative cap [m]) of the records {n0, n1, a0, a1}.  a_s within (2 d + 12) u
    relative: own weight 6 u, the denominator's weights 6 u, its sum (d - 1) u, the division u, the rest second order."""
    assert case["kw"] <= 2
    d, valid, j = _slots(case)
    a = interp_weights_f64(case)
    a = torch.cat([a, torch.zeros(case["m"], 2 - case["kw"], dtype=torch.float64)], 1)
    n0 = j[:, 0]
    n1 = torch.where(d >= 2, j[:, min(1, case["kw"] - 1)], n0)
    return n0, n1, a, (2 * d + 12).double() * U


def interp_weights_emulate(case):
    w, valid, j = _emu_weights(case)
    w = torch.cat([w, torch.zeros(case["m"], 2 - case["kw"])], 1)
    den = w[:, 0] + w[:, 1]
    d = valid.sum(1)
    one = torch.ones_like(den)
    a0 = torch.where(d > 0, w[:, 0] / torch.where(d > 0, den, one), torch.zeros_like(den))
    a1 = torch.where(d > 1, w[:, 1] / torch.where(d > 0, den, one), torch.zeros_like(den))
    return torch.stack([a0, a1], 1)


# ----------------------------------------------------------------------------------------------------------------------------
# rowdot: one wave per row, lane l takes columns 4 l + 256 i, a chain of fmaf per lane, a 6-level butterfly, + b
# ----------------------------------------------------------------------------------------------------------------------------
ROWDOT_CASES = [(F, F + pad, m) for F in (4, 252, 256, 260, 1024) for pad in (0, 4) for m in (1, 5, 1000)]


def rowdot_case(F, ldx, m):
    g = _gen(F + 3 * ldx + 11 * m)
    x = torch.randn(m, ldx, generator=g).float()
    w = torch.randn(F, generator=g).float()
    return dict(F=F, ldx=ldx, m=m, x=x, w=w, b=0.3)


def rowdot_reference(case):
    """(dot(x[i, :F], w) + b in float64, cap).  Cap: a lane's chain is 4 ceil(F / 256) fused multiply-adds, the butterfly adds 6
    levels, the bias one more rounding: (4 ceil(F / 256) + 7) u (sum |x_i w_i| + |b|)."""
    F = case["F"]
    x, w = case["x"][:, :F].double(), case["w"].double()
    b = float(np.float32(case["b"]))
    return x @ w + b, (4 * ((F + 255) // 256) + 7) * U * (x.abs() @ w.abs() + abs(b))


def rowdot_emulate(case):
    F, m = case["F"], case["m"]
    Fp = round_up(F, 256)
    x = torch.zeros(m, Fp)
    x[:, :F] = case["x"][:, :F]
    w = torch.zeros(Fp)
    w[:F] = case["w"]
    acc = torch.zeros(m, 64)
    for i in range(Fp // 256):                      # (a zero column adds +0: exact, as if the lane had skipped it)
        for e in range(4):
            cols = 256 * i + 4 * torch.arange(64) + e
            acc = _fma(x[:, cols], w[cols][None, :], acc)
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0] + torch.tensor(case["b"], dtype=torch.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# exact operators
# ----------------------------------------------------------------------------------------------------------------------------
CONCAT_CASES = [(F, m) for F in (4, 60, 256) for m in (1, 300)]


def concat_case(F, m, kind="randn"):
    """kind: "randn"; "tiny" |x| in [2^-26, 2^-13] (the f16x3 lo plane and the single fp16 plane are subnormal or vanish); "huge"
    |x| in (65504, 1.2e5] (hi saturates, fp16 saturates).  The record's .w is 7.0: it must not show up in column F + 3."""
    g = _gen(13 * F + m + {"randn": 0, "tiny": 1, "huge": 2}[kind])
    sign = torch.where(torch.rand(m, F, generator=g) < 0.5, -1.0, 1.0)
    if kind == "randn":
        x = torch.randn(m, F, generator=g)
    elif kind == "tiny":
        x = sign * torch.exp2(-26.0 + 13.0 * torch.rand(m, F, generator=g))
    else:
        x = sign * (65504.0 + (1.2e5 - 65504.0) * (1.0 - torch.rand(m, F, generator=g)))
    xyzr = torch.cat([torch.randn(m, 3, generator=g), torch.full((m, 1), 7.0)], 1)
    if kind == "tiny":
        xyzr[:, :3] = xyzr[:, :3] * 2.0 ** -18
    elif kind == "huge":
        xyzr[:, :3] = 7.0e4 + 1.0e4 * xyzr[:, :3].abs().clamp(max=4.0)
    return dict(F=F, m=m, x=x.float().contiguous(), xyzr=xyzr.float().contiguous(), kind=kind)


def concat_reference(case, ldo):
    """[x | x y z | 0 ...] of width ldo, fp32, exact."""
    out = torch.zeros(case["m"], ldo)
    out[:, :case["F"]] = case["x"]
    out[:, case["F"]:case["F"] + 3] = case["xyzr"][:, :3]
    return out


SEG_LENGTHS = [0, 1, 3, 15, 16, 17, 0, 1025, 0]        # the 16-way row split against short segments, empty ones at both ends
SEG_F = (1, 40, 64, 65, 130)


def segment_case(F, pad, lengths=None):
    """x [n, F + pad] (pad columns hold NaN: they must not be read into a result) and ptr.  Column 0 is all negative; with F >= 3
    column 1 holds -inf (whole segments 3 and 4, scattered rows elsewhere) and column 2 +inf in one row of segment 5 and -inf in
    its first; the last row of every segment holds that segment's maximum of column F - 1."""
    lengths = SEG_LENGTHS if lengths is None else lengths
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
    n, B = int(ptr[-1]), len(lengths)
    g = _gen(F * 10 + pad + B)
    x = torch.randn(n, F + pad, generator=g).float()
    x[:, F:] = float("nan")
    x[:, 0] = -(x[:, 0].abs() + 1.0)
    seg = torch.repeat_interleave(torch.arange(B), torch.tensor(lengths))
    if F >= 3:
        x[(seg == 3) | (seg == 4) | (torch.arange(n) % 5 == 0), 1] = -float("inf")
        five = torch.nonzero(seg == 5).flatten()
        if len(five) > 3:
            x[five[0], 2] = -float("inf")
            x[five[3], 2] = float("inf")
    last = (ptr[1:][torch.tensor(lengths) > 0] - 1).long()
    x[last, F - 1] = 1000.0 if F > 1 else -0.5
    return dict(F=F, ldx=F + pad, B=B, n=n, x=x.contiguous(), ptr=ptr)


def segment_max_reference(case, empty=0.0):
    """[B, F] float64: the maximum over rows ptr[b] .. ptr[b + 1], `empty` (0, as the reference's scatter gives it) for none."""
    F, ptr = case["F"], case["ptr"].tolist()
    out = torch.full((case["B"], F), float(empty), dtype=torch.float64)
    for b in range(case["B"]):
        if ptr[b + 1] > ptr[b]:
            out[b] = case["x"][ptr[b]:ptr[b + 1], :F].double().max(0).values
    return out


def segment_max_matches(got, ref):
    """Bit-equal where the reference is non-zero, zero where it is zero."""
    r32 = ref.float()
    nz = r32 != 0
    return bool(torch.equal(got[nz].view(torch.int32), r32[nz].view(torch.int32)) and (got[~nz] == 0).all())


PACK_CASES = [(stride, refl, n) for stride in (3, 7) for refl in (True, False) for n in (1, 257, 3000)]


def pack_case(stride, refl, n):
    """CSR over 7 voxels, empty ones first, in the middle (two in a row) and last."""
    g = _gen(stride + 2 * int(refl) + 5 * n)
    a, b = n // 3, n // 2
    ptr = torch.tensor([0, 0, a, a, a, b, n, n], dtype=torch.int32)
    pos = torch.randn(n, stride, generator=g).float()
    r = torch.rand(n, generator=g).float() if refl else None
    return dict(stride=stride, n=n, B=7, ptr=ptr, pos=pos, refl=r)


def pack_reference(case):
    n = case["n"]
    xyzr = torch.zeros(n, 4)
    xyzr[:, :3] = case["pos"][:, :3]
    if case["refl"] is not None:
        xyzr[:, 3] = case["refl"]
    batch = torch.repeat_interleave(torch.arange(case["B"]), torch.diff(case["ptr"].long())).to(torch.int32)
    return xyzr, batch


LEVEL_SF = (0.37, 3.0, 1.0)     # per voxel


def level_case():
    """B = 3 with the last voxel empty, random idx into 500 source records, m_bound = ptr[B] + 50; voxel b is scaled by
    LEVEL_SF[b].  The round trip through 0.37 changes coordinates.  The one through 3.0 cannot: (x / 3) * 3 == x for every binary
    floating-point x short of over- and underflow (true of every divisor 2^i + 2^j) - it is kept as the case where the kernel must
    NOT change a bit."""
    g = _gen(77)
    src = torch.cat([torch.randn(500, 3, generator=g) * 3, torch.rand(500, 1, generator=g)], 1).float().contiguous()
    ptr = torch.tensor([0, 140, 300, 300], dtype=torch.int32)
    m, bound = 300, 350
    idx = torch.randint(0, 500, (bound,), generator=g, dtype=torch.int32)
    batch = torch.zeros(bound, dtype=torch.int32)
    batch[140:] = 1
    return dict(src=src, ptr=ptr, m=m, bound=bound, B=3, idx=idx, batch=batch, sf=torch.tensor(LEVEL_SF, dtype=torch.float32))


def level_reference(case):
    """((p / s) * s, refl) in torch's CPU fp32 arithmetic for the first ptr[B] rows."""
    m = case["m"]
    p = case["src"][case["idx"][:m].long()]
    s = case["sf"][case["batch"][:m].long()][:, None]
    return torch.cat([(p[:, :3] / s) * s, p[:, 3:4]], 1)
