"""The H GEMM's DMA addressing (gemm_hp_body: a 64-bit tile base in scalar registers + one 32-bit byte offset per lane) on A
operands that are not compact: every case of tests/test_gpu_gemm.py has ldh_a = K_pad + one slab, so a wrong pitch, a wrong
window start or a tile base cut to 32 bits would go unseen there.

Both tests run p2w_gemm_h2 twice - on A as a window of wider rows and on a compact copy of the same H values - and compare the
outputs bit for bit: the arithmetic is the same, so there is no tolerance.  Everything of the wide rows outside the window is
NaN (test 1) or never written (test 2: 4.6 GB), the outputs are allocated larger than the launch writes and filled with NaN."""
import ctypes as C

import pytest
import torch

from tests import gemm_ref as R
from tests.h_util import _pack_h, _to_h

pytestmark = pytest.mark.gpu

TILE_128, TILE_256, TILE_64 = 1, 2, 1 << 24
FORM_FLAGS = {"t64": TILE_64, "t128": TILE_128, "t256": TILE_256}
NAN32 = 0x7FC00000


def _launch(prec, A, ldh_a, W, wscale, M, N, K, flags):
    """fp32-output launch (raw accumulators x wscale); the output has 3 guard rows and one slab of guard columns, all NaN."""
    from pointstowood_amd._lib import Epilogue, check, lib, ptr, stream
    ldo = R.round_up(N, 2) + R.K_ALIGN[prec]
    out = torch.full((M + 3, ldo), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
    ep = Epilogue(None, None, None, None, None, None, 0, 0, 0, 0, 0, None, None, 0)
    check(lib().p2w_gemm_h2(prec, ptr(A), ldh_a, ptr(W), wscale, M, N, K, C.byref(ep), ptr(out), ldo, None, 0, flags, stream()))
    torch.cuda.synchronize()
    return out


def _assert_written_once(out, M, N):
    b = out.view(torch.int32)
    assert bool(torch.isfinite(out[:M, :N]).all()), "a NaN reached the output: the launch read outside A's window"
    assert bool((b[M:] == NAN32).all()) and bool((b[:, N:] == NAN32).all()), "the launch wrote outside its [M, N]"


_ops = {}


def _operands(M, N, K, prec):
    """fp32 A [M, K], packed W: once per shape and precision, never modified."""
    key = (M, N, K, prec)
    if key not in _ops:
        g = torch.Generator().manual_seed(7)
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) / K ** 0.5
        _ops[key] = (A,) + _pack_h(W, prec)
    return _ops[key]


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("form,M,N", [("t256", 600, 320), ("t128", 300, 192), ("t64", 150, 192)])
def test_a_as_column_window_of_wider_rows(form, M, N, prec):
    """A's K columns at column offset 512 of H rows of pitch 640 + one slab (the engine reads the columns of a concatenated
    tensor this way).  Three row tiles with a cut last one - the clamped sources - and two column tiles."""
    K, col0 = 100, 512
    ka, planes = R.K_ALIGN[prec], (2 if prec == 0 else 1)
    Kpad, ldh_wide = R.round_up(K, ka), 640 + ka
    A, W, wscale, Kp = _operands(M, N, K, prec)
    assert Kp == Kpad
    compact = _to_h(A, prec, Kpad + ka)                   # [M, planes * (Kpad + ka)], pad columns zero
    assert not bool(torch.isnan(compact.float()).any())
    wide = torch.full((M, planes * ldh_wide), float("nan"), dtype=compact.dtype, device="cuda")
    wide[:, planes * col0:planes * (col0 + Kpad)] = compact[:, :planes * Kpad]
    window = wide[:, planes * col0:]
    assert window.data_ptr() == wide.data_ptr() + 2 * planes * col0
    flags = FORM_FLAGS[form]
    ref = _launch(prec, compact, Kpad + ka, W, wscale, M, N, K, flags)
    got = _launch(prec, window, ldh_wide, W, wscale, M, N, K, flags)
    _assert_written_once(ref, M, N)
    _assert_written_once(got, M, N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), "window launch differs from the compact launch"


@pytest.mark.parametrize("form", ["t256", "t128"])
def test_tile_bases_beyond_4_gib(form):
    """Rows of 32 KiB (f16x3, ldh_a = 8192): the row tiles from row 131 072 on start more than 4 GiB behind A.  Only the first 128
    halves of a row are written and read (K = 64: two slabs per tile); the last row tile is cut."""
    prec, M, N, K, ldh_wide = 0, 140_000, 256, 64, 8192
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 1024 ** 3:
        pytest.skip(f"needs 8 GB of free device memory, {free / 1024 ** 3:.1f} GB are free")
    A, W, wscale, Kp = _operands(M, N, K, prec)
    assert Kp == K
    compact = _to_h(A, prec, K + 32)
    wide = torch.empty((M, 2 * ldh_wide), dtype=torch.float16, device="cuda")
    assert wide.numel() * 2 > 4 * 1024 ** 3
    wide[:, :2 * K] = compact[:, :2 * K]
    flags = FORM_FLAGS[form]
    ref = _launch(prec, compact, K + 32, W, wscale, M, N, K, flags)
    got = _launch(prec, wide, ldh_wide, W, wscale, M, N, K, flags)
    _assert_written_once(ref, M, N)
    _assert_written_once(got, M, N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), "wide-row launch differs from the compact launch"


def test_pitch_beyond_the_lane_offset_is_refused():
    """A lane's offset within a tile is 32-bit: 256 rows x the row's bytes must stay below 2 GiB.  The launcher says so with its
    usual error return and launches nothing (the operands here are far too small for such a pitch)."""
    from pointstowood_amd._lib import Epilogue, lib, ptr, stream
    prec, M, N, K = 0, 64, 64, 32
    A, W, wscale, _ = _operands(M, N, K, prec)
    a = _to_h(A, prec, K + 32)
    out = torch.zeros((M, N), device="cuda")
    ep = Epilogue(None, None, None, None, None, None, 0, 0, 0, 0, 0, None, None, 0)
    args = lambda ldh_a: (prec, ptr(a), ldh_a, ptr(W), wscale, M, N, K, C.byref(ep), ptr(out), N, None, 0, 0, stream())
    assert lib().p2w_gemm_h2(*args(1 << 21)) != 0          # 256 rows x 2 planes x 2^21 halves x 2 B = 2 GiB
    assert lib().p2w_gemm_h2(*args(K + 32)) == 0
    torch.cuda.synchronize()
