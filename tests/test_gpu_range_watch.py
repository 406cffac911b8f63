"""The range watch (p2w_epilogue.range, the `range` argument of p2w_stem_h2*; include/p2w.h) tested directly: the two thresholds to
the last bit, and ONE value over the limit anywhere in a launch - first and last element, every wave's quadrant of an interior
tile, the partly filled last row tile, the last odd column - through every GEMM tile, the specialised and the generic epilogue,
the stream-K fix-up, the row-dot head and the interpolated residual.

Outputs are exact by construction: A is all zeros in H form, so every output is the epilogue of 0: bias (+ residual) bit for bit.
A report is P2W_RANGE_WORDS zeroed words: OVER = the OR of words 64 s, SEEN = the OR of words 64 s + 1 over the slots s; every
other word must still be zero after a launch.  SEEN is conservative on purpose (wave 0 of a workgroup's first tile reports it):
only its two ends are asserted - every output above P2W_RANGE_LO -> 1, none -> 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.h_util import _from_h, _pack_h

pytestmark = pytest.mark.gpu

WORDS, SLOTS = 1024, 16                      # P2W_RANGE_WORDS, P2W_RANGE_SLOTS
HI, LO = np.float32(6.0e4), np.float32(0.03125)
INF = np.float32(np.inf)
HI_NEXT, LO_NEXT = np.nextafter(HI, INF), np.nextafter(LO, INF)
TILE_128, TILE_256, GENERIC, STREAMK, TILE_64 = 1, 2, 4, 64, 1 << 24
PLANES = {0: 2, 1: 1, 2: 1}
HDT = {0: torch.float16, 1: torch.float16, 2: torch.bfloat16}


def _abi():
    from pointstowood_amd._lib import Epilogue, check, lib, ptr, stream
    return lib(), Epilogue, check, ptr, stream


def _new_report(n=1):
    return torch.zeros((n, WORDS), dtype=torch.int32, device="cuda")


def _read(rep):
    """[(OVER, SEEN)] per report row; asserts that no other word was touched and that the words hold 0 or 1."""
    r = rep.cpu().view(-1, SLOTS, 64)
    assert bool((r[:, :, 2:] == 0).all()) and bool(((r == 0) | (r == 1)).all())
    return [(int(x[:, 0].any()), int(x[:, 1].any())) for x in r]


class _Gemm:
    """M x N outputs of a zero A (H form) times ones: every accumulator is 0, the epilogue alone makes the value."""
    def __init__(self, prec, M, N, K):
        ka = 32 if prec == 0 else 64
        self.prec, self.M, self.N, self.K = prec, M, N, K
        self.ldh_a = (K + ka - 1) // ka * ka
        self.ldh_o = (N + ka - 1) // ka * ka
        self.A = torch.zeros((M, PLANES[prec] * self.ldh_a), dtype=HDT[prec], device="cuda")
        self.W, self.wscale, _ = _pack_h(torch.ones(N, K), prec)

    def run(self, ep, flags, f32=True, h=False, ws=None):
        L, _, check, ptr, stream = _abi()
        out = torch.full((self.M, self.N), float("nan"), device="cuda") if f32 else None
        outh = torch.full((self.M, PLANES[self.prec] * self.ldh_o), float("nan"), dtype=HDT[self.prec], device="cuda") if h else None
        a = (self.prec, ptr(self.A), self.ldh_a, ptr(self.W), self.wscale, self.M, self.N, self.K, C.byref(ep), ptr(out), self.N, ptr(outh),
             self.ldh_o)
        if ws is None:
            check(L.p2w_gemm_h2(*a, flags, stream()))
        else:
            check(L.p2w_gemm_h2_sk(*a, ptr(ws), ws.numel(), flags, stream()))
        return out, outh


def _bits(t):
    return t.contiguous().view(torch.int32)


THRESHOLDS = [  # (name, value of every output, OVER, SEEN or None = not asserted)
    ("hi", HI, 0, 1), ("hi_next", HI_NEXT, 1, 1), ("minus_hi_next", -HI_NEXT, 1, 1), ("inf", INF, 1, 1), ("nan", np.float32(np.nan), 1, None),
    ("lo", LO, 0, 0), ("lo_next", LO_NEXT, 0, 1), ("minus_one", np.float32(-1.0), 0, 1)]


@pytest.mark.parametrize("flags", [0, GENERIC, TILE_64, TILE_256, TILE_256 | GENERIC])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_gemm_thresholds_to_the_last_bit(prec, flags):
    """All outputs = one value, every ReLU off: 6.0e4 is in range, the next float (either sign), inf and NaN are OVER; 0.03125 is
    not SEEN, the next float and -1.0 are.  M = 300, N = 200: interior tiles (the specialised epilogue unless P2W_GEMM_GENERIC_EPI)
    and edge tiles (the guarded one) in every launch.  range = NULL gives the same output bits."""
    _, Epilogue, _, ptr, _ = _abi()
    g = _Gemm(prec, 300, 200, 64)
    rep = _new_report(len(THRESHOLDS))
    for i, (name, value, over, seen) in enumerate(THRESHOLDS):
        bias = torch.full((g.N,), float(value), device="cuda")
        out, _ = g.run(Epilogue(ptr(bias), None, None, None, None, None, 0, 0, 0, 0, 0, ptr(rep[i])), flags)
        want = torch.full((g.M, g.N), float(value))
        if name == "nan":
            assert bool(torch.isnan(out).all())
        else:
            assert torch.equal(_bits(out.cpu()), _bits(want)), name                    # v == bias, bit for bit
        plain, _ = g.run(Epilogue(ptr(bias), None, None, None, None, None, 0, 0, 0, 0, 0, None), flags)
        assert torch.equal(_bits(plain), _bits(out)), name
    for (name, value, over, seen), (got_over, got_seen) in zip(THRESHOLDS, _read(rep)):
        assert got_over == over, (name, got_over)
        assert seen is None or got_seen == seen, (name, got_seen)


@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_stem_thresholds_to_the_last_bit(prec, indexed):
    """The same on the stem (w = 0, b = the value; its outputs pass a ReLU, so a negative bias gives 0: in range, not seen).  The
    report is also held against the launch's own fp32 output: OVER iff an output is not <= 6.0e4, SEEN iff one is > 0.03125.
    n = 300, C = 8: two workgroups (p2w_stem_h2), resp. records that carry their row (p2w_stem_h2_indexed)."""
    L, _, check, ptr, stream = _abi()
    n, Cc = 300, 8
    ldh = 32 if prec == 0 else 64
    gen = torch.Generator().manual_seed(3)
    x = torch.cat([torch.rand(n, 3, generator=gen) * 2 - 1, torch.zeros(n, 1)], 1)
    x[:, 3] = torch.arange(n, dtype=torch.int32).view(torch.float32)                  # (indexed: record i carries row i)
    x, w = x.cuda().contiguous(), torch.zeros((Cc, 3), device="cuda")
    fn = L.p2w_stem_h2_indexed if indexed else L.p2w_stem_h2
    rep = _new_report(len(THRESHOLDS))
    outs = []
    for i, (name, value, over, seen) in enumerate(THRESHOLDS):
        b = torch.full((Cc,), float(value), device="cuda")
        out = torch.full((n, Cc), float("nan"), device="cuda")
        oh = torch.full((n, PLANES[prec] * ldh), float("nan"), dtype=HDT[prec], device="cuda")
        check(fn(prec, ptr(x), n, ptr(w), ptr(b), Cc, ptr(out), ptr(oh), ldh, ptr(rep[i]), stream()))
        out2 = torch.full((n, Cc), float("nan"), device="cuda")
        oh2 = torch.full((n, PLANES[prec] * ldh), float("nan"), dtype=HDT[prec], device="cuda")
        check(fn(prec, ptr(x), n, ptr(w), ptr(b), Cc, ptr(out2), ptr(oh2), ldh, None, stream()))
        assert torch.equal(_bits(out), _bits(out2)) and torch.equal(oh.view(torch.int16), oh2.view(torch.int16)), name
        outs.append(out.cpu())
    for (name, value, over, seen), (got_over, got_seen), out in zip(THRESHOLDS, _read(rep), outs):
        if name != "nan":
            want = torch.full((n, Cc), max(float(value), 0.0))
            assert torch.equal(out, want), name
            assert (got_over, got_seen) == (over if value > 0 else 0, seen if value > 0 else 0), (name, got_over, got_seen)
        assert got_over == int(bool((~(out.abs() <= float(HI))).any())), name
        assert got_seen == int(bool((out > float(LO)).any())), name


def _positions(M, N):
    """(row, column) of the planted value: first and last element; one in every wave's part of the first (interior) tile of each
    kernel - the 128 x 128 tile has 2 x 2 waves of 64 x 64 (rows 40 / 100 x columns 33 / 100, and 70 / 20 for the other column half
    of each), the 256 x 256 tile 2 x 4 waves of 128 x 64 (rows 40 / 200 x columns 33 / 100 / 130 / 190), the 64 x 128 tile 2 x 2 waves
    of 32 x 64 (rows 20 / 40 x columns 33 / 70 / 100); the partly filled last row tile; the last odd column."""
    return [(0, 0), (M - 1, N - 1),
            (40, 33), (40, 100), (100, 33), (100, 100), (100, 70), (100, 20),
            (200, 33), (200, 100), (200, 130), (200, 190), (40, 130), (40, 190),
            (20, 33), (20, 70), (20, 100), (40, 70),
            (M - 5, 70), (17, N - 1), (M - 1, 0)]


@pytest.mark.parametrize("generic", [0, GENERIC])
@pytest.mark.parametrize("tile", [TILE_128, TILE_256, TILE_64])
@pytest.mark.parametrize("M,N", [(300, 200), (700, 256)])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_one_planted_value_raises_over_wherever_it_sits(prec, M, N, tile, generic):
    """Ordinary outputs 1.0 (bias) + an fp32 residual that is zero but for ONE element, 69999.0: that output is 7.0e4.  Residual +
    final ReLU + fp32 output is a specialised epilogue class on interior tiles; P2W_GEMM_GENERIC_EPI and the edge tiles run the
    guarded one.  Every position must raise OVER; without a plant OVER = 0 and SEEN = 1."""
    _, Epilogue, _, ptr, _ = _abi()
    g = _Gemm(prec, M, N, 64)
    bias = torch.ones(N, device="cuda")
    res = torch.zeros((M, N), device="cuda")
    pos = _positions(M, N)
    rep = _new_report(len(pos) + 1)
    ep = lambda i: Epilogue(ptr(bias), None, None, None, None, ptr(res), N, 0, 0, 0, 1, ptr(rep[i]))
    out, _ = g.run(ep(len(pos)), tile | generic)
    assert bool((out == 1.0).all())
    for i, (r, c) in enumerate(pos):
        res[r, c] = 69999.0
        out, _ = g.run(ep(i), tile | generic)
        res[r, c] = 0.0
        assert float(out[r, c]) == 7.0e4 and int((out == 1.0).sum()) == M * N - 1, (r, c)
    got = _read(rep)
    assert got[-1] == (0, 1)
    assert [o for o, _ in got[:-1]] == [1] * len(pos), [p for p, (o, _) in zip(pos, got) if o != 1]


@pytest.mark.parametrize("M,N,K,pos", [(300, 200, 256, [(5, 3), (299, 199), (290, 40), (100, 199)]),
                                       (70000, 512, 512, [(69999, 511), (69990, 3), (69900, 300), (5, 3)])])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_planted_value_through_the_stream_k_fixup(prec, M, N, K, pos):
    """p2w_gemm_h2_sk with P2W_GEMM_STREAMK; the fix-up pass runs the epilogue - the specialised one on full 16-row blocks, the
    guarded one at the edges.  M = 300, N = 200, K = 256 has no whole round of the chip, so every row is a tail row.  This rests on
    launch_gemm_h's plan: no 64 x 128 tile (N > 192 and the 128 x 128 tiles' last round is no emptier than the smaller tile's), no
    whole round (q = 0), P2W_GEMM_STREAMK forcing the split tail.  M = 70000, N = K = 512 (a shape tests/test_gpu_ops.py forces
    through the split tail as well) has whole rounds in front of the tail: the plants sit in the last rows, which belong to the
    tail whatever the chip's size, and one in the first rows, which the main launch reports.
    That the split tail ran is checked: it sums the K range in pieces, so a NaN workspace stays NaN only if nobody wrote it."""
    L, Epilogue, _, ptr, _ = _abi()
    g = _Gemm(prec, M, N, K)
    ws = torch.full((int(L.p2w_gemm_h2_sk_ws_bytes()) // 4,), float("nan"), device="cuda").view(torch.uint8)
    bias = torch.ones(N, device="cuda")
    res = torch.zeros((M, N), device="cuda")
    rep = _new_report(len(pos) + 1)
    ep = lambda i: Epilogue(ptr(bias), None, None, None, None, ptr(res), N, 0, 0, 0, 1, ptr(rep[i]))
    out, _ = g.run(ep(len(pos)), STREAMK, ws=ws)
    assert bool((out == 1.0).all())
    assert not bool(torch.isnan(ws.view(torch.float32)[:128 * 128]).any())            # the first piece of the split tail was written
    for i, (r, c) in enumerate(pos):
        res[r, c] = 69999.0
        out, _ = g.run(ep(i), STREAMK, ws=ws)
        res[r, c] = 0.0
        assert float(out[r, c]) == 7.0e4 and int((out == 1.0).sum()) == M * N - 1, (r, c)
    got = _read(rep)
    assert got[-1] == (0, 1) and [o for o, _ in got[:-1]] == [1] * len(pos), got


@pytest.mark.parametrize("flags", [0, GENERIC, TILE_256])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_planted_bias_column_through_the_rowdot_head(prec, flags):
    """p2w_gemm_h2_rowdot takes no residual: the plant is one bias column (bias + ReLU = its specialised class), in an interior
    tile and in the last, partly filled column tile."""
    L, Epilogue, check, ptr, stream = _abi()
    M, N, K = 300, 200, 64
    g = _Gemm(prec, M, N, K)
    need = int(L.p2w_gemm_h2_rowdot_ws_bytes(M, N))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    dotw = torch.ones(N, device="cuda")
    cols = [None, 3, 70, N - 1]
    rep = _new_report(len(cols))
    for i, c in enumerate(cols):
        bias = torch.ones(N, device="cuda")
        if c is not None:
            bias[c] = 7.0e4
        ep = Epilogue(ptr(bias), None, None, None, None, None, 0, 1, 0, 0, 0, ptr(rep[i]))
        out = torch.full((M,), float("nan"), device="cuda")
        check(L.p2w_gemm_h2_rowdot(prec, ptr(g.A), g.ldh_a, ptr(g.W), g.wscale, M, N, K, C.byref(ep), ptr(dotw), 0.5, ptr(out), ptr(ws), need,
                                   flags, stream()))
        want = (N + 0.5) if c is None else (N - 1 + 7.0e4 + 0.5)                       # small integers and halves: exact in any order
        assert bool((out == want).all()), (c, float(out[0]))
    assert _read(rep) == [(0, 1), (1, 1), (1, 1), (1, 1)]


@pytest.mark.parametrize("generic", [0, GENERIC])
@pytest.mark.parametrize("prec", [0, 1])
def test_planted_value_through_the_interpolated_residual(prec, generic):
    """p2w_epilogue.interp: the residual of row r is a0 Z[n0] + a1 Z[n1]; one-neighbour records {n0, n0, 1, 0} from
    p2w_interp_weights make it Z[n0] exactly, the plant sits in the coarse matrix Z.  Bias + interpolated residual + ReLU with an H
    output is the specialised class of the 128 x 128 kernel; P2W_GEMM_GENERIC_EPI and the edge tiles run the guarded one."""
    L, Epilogue, check, ptr, stream = _abi()
    M, N, Mx = 300, 256, 40
    g = _Gemm(prec, M, N, 64)
    gen = torch.Generator().manual_seed(9)
    pc, pf = torch.rand(Mx, 4, generator=gen).cuda(), torch.rand(M, 4, generator=gen).cuda()
    nbr = (torch.arange(M, dtype=torch.int32) % Mx).cuda()
    deg = torch.ones(M, dtype=torch.int32, device="cuda")
    rec = torch.empty((M, 4), dtype=torch.int32, device="cuda")
    check(L.p2w_interp_weights(ptr(pc), ptr(pf), ptr(nbr), ptr(deg), 1, M, ptr(rec), stream()))
    bias = torch.ones(N, device="cuda")
    Z = torch.zeros((Mx, N), device="cuda")
    pos = [None, (0, 0), (Mx - 1, N - 1), (17, 131)]            # coarse row 39 feeds fine rows 39, 79, ..., 279 (the last row tile too)
    rep = _new_report(len(pos))
    for i, p in enumerate(pos):
        if p is not None:
            Z[p] = 69999.0
        ep = Epilogue(ptr(bias), None, None, None, None, ptr(Z), N, 0, 0, 0, 1, ptr(rep[i]), ptr(rec), Mx)
        _, outh = g.run(ep, generic, f32=False, h=True)
        if p is not None:
            Z[p] = 0.0
        v = _from_h(outh, prec, g.ldh_o)[:, :N]
        want = torch.ones(M, N, dtype=torch.float64)
        if p is not None:
            want[p[0]::Mx, p[1]] = 7.0e4 if prec == 0 else 65504.0                     # (the single fp16 plane saturates)
        assert torch.equal(v, want), p
    assert _read(rep) == [(0, 1), (1, 1), (1, 1), (1, 1)]
