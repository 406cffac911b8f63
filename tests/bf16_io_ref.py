"""The bfloat16 rounding that the bfloat16 entry points of the training operators (include/p2w.h: p2w_*_io with P2W_BF16, ops.half_io)
are held to.

A bfloat16 is the top 16 bits of an fp32: 1 sign bit, fp32's 8 exponent bits, 7 mantissa bits.  A bfloat16 store of those kernels must
be ONE rounding of the fp32 result: to nearest, ties to the even mantissa; a carry out of the largest finite value (the patterns
0x7F7F8000 and up) gives +-inf; fp32 subnormals round to bfloat16 subnormals and +-0 on the same grid (quantum 2^-133), nothing is
flushed; the sign of a zero is kept; a NaN stays a NaN, one whose payload lies only in the low 16 bits included - a truncation would
turn that one into an infinity.  That is torch.Tensor.bfloat16().  round_bits() computes it from the definition on the integer fields
of the fp32 value; TABLE32 / TABLE16 is a table of the cases that matter, the named ones written out by hand in NAMED as (fp32
pattern, bfloat16 pattern).  tests/test_bf16_io_ref_cpu.py pins both against PyTorch on the CPU; the GPU tests run the table through
the kernels' store."""
import numpy as np

NAN16 = 0x7fc0            # NaNs are compared as NaNs, never by payload


def round_bits(x):
    """uint16 bit patterns of float32 `x` (any shape) rounded to bfloat16, from the definition, in Python integers: the magnitude's
    31 bits are an integer count of steps on a grid on which the bfloat16 values are the multiples of 2^16 - inside a binade, across
    binades (a mantissa that carries raises the exponent field) and through the subnormals alike - so rounding to nearest even is
    rounding that integer to a multiple of 2^16, and the first multiple past the largest finite value is the infinity's pattern."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.size, dtype=np.uint16)
    for i, u in enumerate(x.reshape(-1).view(np.uint32).tolist()):
        sign, mag = (u >> 31) << 15, u & 0x7fffffff
        if mag > 0x7f800000:
            out[i] = NAN16
            continue
        n, rem = mag >> 16, mag & 0xffff
        if rem > 0x8000 or (rem == 0x8000 and (n & 1)):
            n += 1
        out[i] = sign | n                                  # n <= 0x7f80: a carry out of 0x7f7f is the infinity
    return out.reshape(x.shape)


# fp32 pattern -> bfloat16 pattern, by hand
NAMED = [
    (0x3F800000, 0x3F80), (0x3F000000, 0x3F00), (0x3FC00000, 0x3FC0), (0xC0300000, 0xC030), (0x44800000, 0x4480),   # 1, .5, 1.5, -2.75, 1024
    (0x3F808000, 0x3F80),      # a tie above the even mantissa 0: down
    (0x3F818000, 0x3F82),      # a tie below the even mantissa 2 (above the odd 1): up
    (0x3F808001, 0x3F81),      # just above the tie
    (0x3F817FFF, 0x3F81),      # just below the tie
    (0x3F807FFF, 0x3F80),
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82), (0xBF808001, 0xBF81),
    (0x3FFF8000, 0x4000),      # a tie that carries into the exponent
    (0x7F7F0000, 0x7F7F),      # the largest finite bfloat16
    (0x7F7F7FFF, 0x7F7F),      # the last pattern that stays finite
    (0x7F7F8000, 0x7F80),      # the tie above it: the carry gives +inf
    (0x7F7FFFFF, 0x7F80),      # FLT_MAX
    (0xFF7F7FFF, 0xFF7F), (0xFF7F8000, 0xFF80), (0xFF7FFFFF, 0xFF80),
    (0x00000001, 0x0000),      # the smallest fp32 subnormal
    (0x00008000, 0x0000),      # half the smallest bfloat16 subnormal: a tie, to the even 0
    (0x80008000, 0x8000),      # ... which keeps its sign
    (0x00008001, 0x0001),      # just above it
    (0x00018000, 0x0002),      # a tie between the subnormals 1 and 2: to the even one
    (0x00010000, 0x0001),      # the smallest bfloat16 subnormal
    (0x007F0000, 0x007F),      # the largest bfloat16 subnormal
    (0x007FFFFF, 0x0080),      # the largest fp32 subnormal: up to the smallest normal
    (0x007F8000, 0x0080),      # a tie between the largest subnormal and the smallest normal: to the even one
    (0x007F7FFF, 0x007F),
    (0x00800000, 0x0080),      # the smallest normal
    (0x80000001, 0x8000), (0x80018000, 0x8002),
    (0x00000000, 0x0000), (0x80000000, 0x8000), (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
    (0x7FC00000, NAN16),       # the quiet NaN
    (0x7F800001, NAN16),       # NaNs whose payload lies in the low 16 bits only: a truncation would give +-inf
    (0xFF800001, NAN16),
    (0x7F80FFFF, NAN16), (0x7FFFFFFF, NAN16),
]
_rng = np.random.default_rng(13)
_extra = np.concatenate([
    (_rng.standard_normal(8) * 3).astype(np.float32),                                  # ordinary values
    (_rng.standard_normal(6) * 2.0 ** -130).astype(np.float32),                        # across the subnormal range
    np.array([0.1, -0.1, 1 / 3, 60000.3, -33.33, 3e38, -1e-30], dtype=np.float32)])
TABLE32 = np.concatenate([np.array([u for u, _ in NAMED], dtype=np.uint32).view(np.float32), _extra])
TABLE16 = round_bits(TABLE32)


def same_bits(a, b):
    """uint16 arrays equal, every NaN pattern counting as the one NaN."""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    na, nb = (a & 0x7fff) > 0x7f80, (b & 0x7fff) > 0x7f80
    return a.shape == b.shape and bool((na == nb).all()) and bool((a[~na] == b[~nb]).all())
