"""tests/bf16_io_ref.py against PyTorch on the CPU: the references of tests/test_gpu_bf16_io.py."""
import numpy as np
import torch

from tests import bf16_io_ref as R


def _by_torch(x32):
    return torch.from_numpy(np.ascontiguousarray(x32).copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)


def test_named_cases_are_what_the_definition_gives():
    got = R.round_bits(np.array([u for u, _ in R.NAMED], dtype=np.uint32).view(np.float32))
    for (u, want), g in zip(R.NAMED, got.tolist()):
        assert g == want, (hex(u), hex(g), hex(want))
    assert len(R.TABLE32) == len(R.TABLE16) >= len(R.NAMED) + 10
    named = dict(R.NAMED)
    for u, want in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F808001, 0x3F81), (0x3FFF8000, 0x4000), (0x7F7F7FFF, 0x7F7F),
                    (0x7F7F8000, 0x7F80), (0x7F7FFFFF, 0x7F80), (0x00000001, 0x0000), (0x00008000, 0x0000), (0x80008000, 0x8000),
                    (0x00008001, 0x0001), (0x00018000, 0x0002), (0x007F8000, 0x0080), (0x7F800001, R.NAN16), (0xFF800001, R.NAN16)):
        assert named[u] == want, hex(u)


def test_table_is_torch_rounding():
    assert R.same_bits(R.TABLE16, _by_torch(R.TABLE32))
    # the signs of the zeros and of the infinities are bits, not NaNs: they are compared above
    nan = np.isnan(R.TABLE32)
    assert int(nan.sum()) >= 5 and bool(((R.TABLE16[nan] & 0x7fff) > 0x7f80).all())


def test_definition_on_random_bit_patterns():
    """2 x 10^6 uniformly random fp32 patterns (NaNs, infinities and subnormals among them), then every bfloat16 value's neighbourhood
    of ties: the definition, restated on arrays, and PyTorch's CPU conversion agree with round_bits, every NaN staying a NaN."""
    rng = np.random.default_rng(7)
    u = rng.integers(0, 1 << 32, size=2_000_000, dtype=np.uint64).astype(np.uint32)
    h = (np.arange(0x7f80, dtype=np.uint32) << 16)                                      # every finite non-negative bfloat16, widened
    ties = np.concatenate([h | 0x8000, h | 0x7fff, h | 0x8001, h])
    u = np.concatenate([u, ties, ties | 0x80000000])
    by_array = ((u.astype(np.uint64) + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7fffffff) > 0x7f800000
    by_array[nan] = R.NAN16
    got = _by_torch(u.view(np.float32))
    want = R.round_bits(u.view(np.float32))
    assert R.same_bits(got, want) and R.same_bits(by_array, want)
    assert bool(((got[nan] & 0x7fff) > 0x7f80).all()) and int(nan.sum()) > 1000


def test_widening_and_rounding_back_is_the_identity_on_every_pattern():
    bits = np.arange(65536, dtype=np.uint16)
    wide = (bits.astype(np.uint32) << 16).view(np.float32)
    assert R.same_bits(R.round_bits(wide), bits)
    t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    back = t.float().bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert R.same_bits(back, bits)
    live = ~np.isnan(wide)
    assert np.array_equal(t.float().numpy().view(np.uint32)[live], wide.view(np.uint32)[live])
