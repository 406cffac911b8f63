"""The 16-bit route of layer 1 of the edge MLP (csrc/p2w_edge.hip: p2w_edge_l1_io / p2w_edge_l1_bwd_io; ops.edge_layer1(out_dtype=)):
the planted values that separate a ReLU mask recomputed in fp32 from one read back from the stored float16 / bfloat16 H1, and a numpy
restatement of the backward with either mask.

Why the mask is recomputed: H1 = relu(h) is stored once, rounded to nearest even.  An fp32 h in (0, 2^-25] stores as float16 zero
(2^-25 is the tie between 0 and the smallest subnormal 2^-24, and ties go to the even mantissa); an fp32 subnormal of at most 2^-134
stores as bfloat16 zero.  The cast-first route (ops.half_io = False) takes its mask from the fp32 H1, where these elements pass their
gradient on; a mask read from the stored tensor would drop it.  Nothing here has a tolerance: the 16-bit patterns are
torch.Tensor.half() / .bfloat16() of the fp32 value, and the planted columns have Wg = 0, so h = P[j, c] exactly."""
import numpy as np
import torch

# (fp32 pattern, float16 pattern, bfloat16 pattern) - the 16-bit ones as torch.Tensor.half() / .bfloat16() give them on the CPU
# (tests/test_edge_io_ref_cpu.py asserts that).  All of them are > 0 in fp32.
TABLE = [
    (0x33000000, 0x0000, 0x3300),      # 2^-25: the tie between 0 and 2^-24 goes to the even one, 0
    (0x32800000, 0x0000, 0x3280),      # 2^-26
    (0x0DA24260, 0x0000, 0x0DA2),      # 1e-30
    (0x000116C2, 0x0000, 0x0001),      # 1e-40, an fp32 subnormal: bfloat16 keeps it as its smallest subnormal
    (0x33000001, 0x0001, 0x3300),      # nextafter(2^-25): above the tie
    (0x33800000, 0x0001, 0x3380),      # 2^-24, the smallest float16 subnormal
    (0x477FEFFF, 0x7BFF, 0x4780),      # 65519.996: the largest fp32 below the tie to float16 inf
    (0x477FF000, 0x7C00, 0x4780),      # 65520: the tie goes to the even one, inf
    (0x00000007, 0x0000, 0x0000),      # 1e-44 = 7 * 2^-149, below 2^-134: zero in both
    (0x7F7F8000, 0x7C00, 0x7F80),      # the tie above bfloat16's largest finite value carries to inf
    (0x7F7F7FFF, 0x7C00, 0x7F7F),      # one below it does not
    (0x3F800000, 0x3C00, 0x3F80),      # 1.0
]
# planted beside the table on the GPU (fp32 patterns): -0.0, a negative tiny value, a NaN, +inf.  relu gives +0, 0, 0 (fmaxf drops
# the NaN) and inf; none of the first three passes a gradient on, inf does.
EXTRA32 = [0x80000000, 0x8DA24260, 0x7FC00000, 0x7F800000]

TABLE32 = np.array([t[0] for t in TABLE], dtype=np.uint32).view(np.float32)
TABLE_F16 = np.array([t[1] for t in TABLE], dtype=np.uint16)
TABLE_BF16 = np.array([t[2] for t in TABLE], dtype=np.uint16)
PLANTED32 = np.concatenate([TABLE32.view(np.uint32), np.array(EXTRA32, dtype=np.uint32)]).view(np.float32)
N_PLANTED = PLANTED32.size                  # 16

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def store_bits(h32, kind):
    """The uint16 patterns of an fp32 numpy array stored as float16 / bfloat16 by torch on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(h32, dtype=np.float32)).to(DTYPES[kind])
    return t.view(torch.int16).numpy().view(np.uint16)


def stored(h32, kind):
    """h32 after the round trip through the 16-bit type, as fp32 (the widening is exact)."""
    return torch.from_numpy(np.ascontiguousarray(h32, dtype=np.float32)).to(DTYPES[kind]).float().numpy()


def planted_case(C1):
    """16 sources, 4 targets of 4 edges each, every source referenced by exactly one edge (so gP[s] is one edge's term, no sum).
    Columns 1 and 2 of Wg are zero and carry the planted values in P: P[s, 1] = PLANTED32[s], P[s, 2] = PLANTED32[(s + 5) % 16]."""
    assert C1 >= 4
    g = torch.Generator().manual_seed(900 + C1)
    n, M = N_PLANTED, 4
    P, Wg = torch.randn(n, C1, generator=g), torch.randn(4, C1, generator=g)
    Wg[:, 1:3] = 0
    planted = torch.from_numpy(PLANTED32.copy())
    P[:, 1], P[:, 2] = planted, planted.roll(-5)
    src = torch.randperm(n, generator=g).to(torch.int32)
    ptr = torch.arange(0, n + 1, 4, dtype=torch.int32)
    pos_src, pos_dst = torch.rand(n, 4, generator=g), torch.rand(M, 4, generator=g)
    return dict(P=P, Wg=Wg, src=src, ptr=ptr, pos_src=pos_src, pos_dst=pos_dst, n_src=n, M=M, E=n, cols=(1, 2))


def h_fp32(P, geo, src, Wg, n_src):
    """The forward's pre-ReLU-then-ReLU value per edge in fp32 numpy, every product and sum rounded on its own, in the kernel's order;
    0 for a source outside [0, n_src)."""
    P, geo, Wg = (np.asarray(a, dtype=np.float32) for a in (P, geo, Wg))
    j = np.asarray(src, dtype=np.int64)
    ok = (j >= 0) & (j < n_src)
    h = P[np.where(ok, j, 0)].copy()
    with np.errstate(all="ignore"):
        for d in range(4):
            h = (h + (geo[:, d:d + 1] * Wg[d][None, :]).astype(np.float32)).astype(np.float32)
        h = np.where(h > 0, h, np.float32(0))           # fmaxf(h, 0): a NaN gives 0
    h[~ok] = 0
    return h


def backward(gH, P, geo, src, Wg, n_src, mask_from=None):
    """(gP, gR, gWg) in float64 with gZ = gH where the mask holds.  mask_from None: the mask recomputed in fp32 (h > 0) - what
    p2w_edge_l1_bwd_io does and what the fp32 route's saved H1 gives; "f16" / "bf16": the mask read back from the stored 16-bit H1 -
    what the kernels must NOT do."""
    h = h_fp32(P, geo, src, Wg, n_src)
    if mask_from is not None:
        h = stored(h, mask_from)
    j = np.asarray(src, dtype=np.int64)
    ok = (j >= 0) & (j < n_src)
    gZ = np.where((h > 0) & ok[:, None], np.asarray(gH, dtype=np.float64), 0.0)
    gP = np.zeros((n_src, gZ.shape[1]))
    np.add.at(gP, j[ok], gZ[ok])
    gR = gP @ np.asarray(Wg, dtype=np.float64)[3]
    gWg = np.asarray(geo, dtype=np.float64).T @ gZ
    return gP, gR, gWg
