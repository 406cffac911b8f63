"""The voxeliser's cap of include/p2w.h (p2w_cap_subset) restated in numpy over tests/feed_ref.philox4x32_10.

Weighted mode: key = float32(-log(u) / w) with u = (w0 + 0.5) 2^-32 and w0 = word 0 of Philox4x32-10 at counter (row_id, c1, c2, STREAM),
logarithm and division in float64 and ONE rounding to float32; 0xFFFFFFFF for a weight that is not finite and positive; a segment keeps
the k rows smallest in (key pattern, position), ascending by position, -1 behind a segment of fewer than k rows.  Replacement mode:
draw j of segment s is start + floor(w0 count / 2^32), w0 at counter (j, row_id[start], c2, STREAM ^ 1)."""
from __future__ import annotations

import numpy as np

from tests.feed_ref import philox4x32_10

STREAM = 0x50325743    # "P2WC"
N_MAX, S_MAX, OUT_MAX = 1 << 30, 1 << 20, 1 << 38   # P2W_CAP_N_MAX, P2W_CAP_S_MAX, P2W_CAP_OUT_MAX
INVALID = 0xFFFFFFFF


def word0(c0, c1, c2, c3, seed):
    """Word 0 at counter (c0, c1, c2, c3), every word broadcast against the others and taken modulo 2^32 -> uint32."""
    c = np.stack(np.broadcast_arrays(*(np.asarray(v, dtype=np.int64) & 0xffffffff for v in (c0, c1, c2, c3))), axis=-1)
    return philox4x32_10(c.astype(np.uint64), [seed & 0xffffffff, (seed >> 32) & 0xffffffff])[..., 0]


def race_keys(row_id, weight, seed, c1, c2):
    """uint32 patterns of the race's float32 keys; ``row_id``, ``weight`` (float32) and ``c2`` broadcast against each other."""
    w = np.asarray(weight, dtype=np.float32).astype(np.float64)
    u = (word0(row_id, c1, c2, STREAM, seed).astype(np.float64) + 0.5) * 2.0 ** -32
    valid = np.isfinite(w) & (w > 0)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        key = (-np.log(u) / np.where(valid, w, 1.0)).astype(np.float32)
    return np.where(valid, key.view(np.uint32), np.uint32(INVALID)).astype(np.uint32)


def ranges(n, seg_start, seg_count):
    """(start, count) per segment, clamped to the row space as the operator clamps them."""
    start = np.clip(np.asarray(seg_start, dtype=np.int64), 0, n)
    return start, np.clip(np.asarray(seg_count, dtype=np.int64), 0, n - start)


def select(n, seg_start, seg_count, k, keys):
    """[S, k] int64 from the key pattern of every row (any integer array of 32-bit patterns)."""
    key = np.asarray(keys).astype(np.int64) & 0xffffffff
    start, count = ranges(n, seg_start, seg_count)
    out = np.full((len(start), k), -1, dtype=np.int64)
    for s, (a, c) in enumerate(zip(start.tolist(), count.tolist())):
        pos = np.arange(a, a + c)
        keep = np.sort(pos[np.lexsort((pos, key[a:a + c]))[:k]])
        out[s, :len(keep)] = keep
    return out


def subset(n, seg_start, seg_count, k, weight, seed, c1, c2, row_id=None):
    """Weighted mode from the generator -> ([S, k] int64, key pattern of every row of the row space)."""
    key = race_keys(np.arange(n) if row_id is None else row_id, weight, seed, c1, c2)
    return select(n, seg_start, seg_count, k, key), key


def replace(n, seg_start, seg_count, k, seed, c2, row_id=None):
    """Replacement mode -> [S, k] int64 in draw order."""
    start, count = ranges(n, seg_start, seg_count)
    out = np.full((len(start), k), -1, dtype=np.int64)
    for s, (a, c) in enumerate(zip(start.tolist(), count.tolist())):
        if c > 0:
            w0 = word0(np.arange(k), a if row_id is None else int(row_id[a]), c2, STREAM ^ 1, seed).astype(np.uint64)
            out[s] = a + ((w0 * np.uint64(c)) >> np.uint64(32)).astype(np.int64)
    return out
