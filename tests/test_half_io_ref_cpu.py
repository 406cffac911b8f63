"""tests/half_io_ref.py against numpy and PyTorch on the CPU: the references of tests/test_gpu_half_io.py."""
import numpy as np
import torch

from tests import half_io_ref as R


def test_named_cases_are_what_the_definition_gives():
    got = R.round_bits(np.array([v for v, _ in R.NAMED], dtype=np.float32))
    for (v, want), g in zip(R.NAMED, got.tolist()):
        assert g == want, (float(v), hex(g), hex(want))
    assert len(R.TABLE32) == len(R.TABLE16) >= len(R.NAMED) + 10


def test_table_is_numpy_and_torch_rounding():
    with np.errstate(over="ignore"):
        by_numpy = R.TABLE32.astype(np.float16).view(np.uint16)
    by_torch = torch.from_numpy(R.TABLE32.copy()).half().view(torch.int16).numpy().view(np.uint16)
    assert R.same_half_bits(R.TABLE16, by_numpy) and R.same_half_bits(R.TABLE16, by_torch)
    # the signs of the zeros and of the infinities are bits, not NaNs: they are compared above


def test_definition_on_a_dense_sample():
    """Every float16 value, its neighbours' midpoints and a step to either side of each midpoint, against numpy and PyTorch."""
    h = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)               # every finite non-negative value
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)      # exact in fp32
    x = np.concatenate([h, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    x = np.concatenate([x, -x])
    want = R.round_bits(x)
    with np.errstate(over="ignore"):
        assert R.same_half_bits(want, x.astype(np.float16).view(np.uint16))
    assert R.same_half_bits(want, torch.from_numpy(x).half().view(torch.int16).numpy().view(np.uint16))


def test_widening_and_rounding_back_is_the_identity_on_every_pattern():
    bits = np.arange(65536, dtype=np.uint16)
    wide = bits.view(np.float16).astype(np.float32)
    assert R.same_half_bits(wide.astype(np.float16).view(np.uint16), bits) and R.same_half_bits(R.round_bits(wide), bits)
    t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16)
    back = t.float().half().view(torch.int16).numpy().view(np.uint16)
    assert R.same_half_bits(back, bits)
    assert np.array_equal(t.float().numpy().view(np.uint32)[~np.isnan(wide)], wide.view(np.uint32)[~np.isnan(wide)])
