"""The float16 rounding that the float16 entry points of the training operators (include/p2w.h: p2w_*_io, ops.half_io) are held to.

A float16 store of those kernels must be ONE rounding of the fp32 result: to nearest, ties to the even mantissa, overflow to +-inf
(from 65520 = 65504 + half a quantum on), gradual underflow (quantum 2^-24 below 2^-14; 2^-25 is a tie and goes to 0, anything above
it to 2^-24), the sign of a zero kept, a NaN kept a NaN - torch.Tensor.half().  round_bits() computes that from the definition on the
integer fields of the fp32 value; TABLE32 / TABLE16 is a table of the cases that matter, the named ones written out by hand in NAMED.
tests/test_half_io_ref_cpu.py pins both against numpy and PyTorch on the CPU; the GPU tests run the table through the kernels' store."""
import numpy as np

NAN16 = 0x7e00            # NaNs are compared as NaNs, never by payload


def round_bits(x):
    """uint16 bit patterns of float32 `x` (any shape) rounded to float16, from the definition, in Python integers."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.size, dtype=np.uint16)
    for i, u in enumerate(x.reshape(-1).view(np.uint32).tolist()):
        sign, exp, man = (u >> 31) << 15, (u >> 23) & 0xff, u & 0x7fffff
        if exp == 255:
            out[i] = NAN16 if man else sign | 0x7c00
            continue
        m, E = (man | 0x800000, exp - 150) if exp else (man, -149)          # |x| = m 2^E exactly
        if m == 0:
            out[i] = sign
            continue
        top = m.bit_length() - 1 + E                                          # 2^top <= |x| < 2^(top + 1)
        Q = max(top, -14) - 10                                                # the float16 quantum 2^Q at |x|
        if E >= Q:
            n = m << (E - Q)
        else:
            sh = Q - E
            n, rem, half = m >> sh, m & ((1 << sh) - 1), 1 << (sh - 1)
            if rem > half or (rem == half and (n & 1)):
                n += 1
        if Q == -24:                                                          # subnormal, or 1024 = the smallest normal: the same bits
            out[i] = sign | n
            continue
        e16 = Q + 10 + 15
        if n == 2048:
            n, e16 = 1024, e16 + 1
        out[i] = sign | (0x7c00 if e16 >= 31 else (e16 << 10) | (n - 1024))
    return out.reshape(x.shape)


def _f(v):
    return np.float32(v)


# value -> float16 bits, by hand
NAMED = [
    (_f(1.0), 0x3c00), (_f(0.5), 0x3800), (_f(1.5), 0x3e00), (_f(-2.75), 0xc180), (_f(1024.0), 0x6400), (_f(2.0 ** -14), 0x0400),
    (_f(1.0 + 2.0 ** -11), 0x3c00),                  # a tie above the even mantissa 0: down
    (_f(1.0 + 3 * 2.0 ** -11), 0x3c02),              # a tie below the even mantissa 2: up
    (_f(1.0 + 2.0 ** -11 + 2.0 ** -23), 0x3c01),     # just above the tie
    (_f(1.0 + 3 * 2.0 ** -11 - 2.0 ** -23), 0x3c01),   # just below the tie
    (_f(-(1.0 + 2.0 ** -11)), 0xbc00), (_f(-(1.0 + 3 * 2.0 ** -11)), 0xbc02),
    (_f(2.0 - 2.0 ** -12), 0x4000),                  # a tie that carries into the exponent
    (_f(65504.0), 0x7bff), (_f(65519.99), 0x7bff), (_f(65520.0), 0x7c00), (_f(-65519.99), 0xfbff), (_f(-65520.0), 0xfc00),
    (_f(1e9), 0x7c00), (_f(-3e38), 0xfc00),
    (_f(1023 * 2.0 ** -24), 0x03ff),                 # the largest subnormal
    (_f(2.0 ** -14 - 2.0 ** -25), 0x0400),           # a tie between it and the smallest normal: to the even one
    (_f(2.0 ** -24), 0x0001), (_f(2.0 ** -25), 0x0000), (_f(2.0 ** -25 * 1.0001), 0x0001), (_f(-(2.0 ** -25)), 0x8000),
    (_f(-(2.0 ** -25) * 1.0001), 0x8001), (_f(3 * 2.0 ** -25), 0x0002), (_f(2.5 * 2.0 ** -24), 0x0002), (_f(3.5 * 2.0 ** -24), 0x0004),
    (_f(1e-30), 0x0000), (_f(-1e-30), 0x8000), (_f(1e-45), 0x0000),
    (_f(0.0), 0x0000), (_f(-0.0), 0x8000), (_f(np.inf), 0x7c00), (_f(-np.inf), 0xfc00), (_f(np.nan), NAN16),
]
_rng = np.random.default_rng(11)
_extra = np.concatenate([
    (_rng.standard_normal(8) * 3).astype(np.float32),                                  # ordinary values
    (_rng.standard_normal(6) * 2.0 ** -18).astype(np.float32),                         # across the subnormal range
    np.array([0.1, -0.1, 1 / 3, 60000.3, -33.33], dtype=np.float32)])
TABLE32 = np.concatenate([np.array([v for v, _ in NAMED], dtype=np.float32), _extra])
TABLE16 = round_bits(TABLE32)


def same_half_bits(a, b):
    """uint16 arrays equal, every NaN pattern counting as the one NaN."""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    na, nb = (a & 0x7fff) > 0x7c00, (b & 0x7fff) > 0x7c00
    return a.shape == b.shape and bool((na == nb).all()) and bool((a[~na] == b[~nb]).all())
