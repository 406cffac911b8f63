"""The random k-subset of include/p2w.h (p2w_random_subset) restated in numpy over tests/feed_ref.philox4x32_10: the k rows that are
smallest in the order of (key, row), ascending; key = word 0 of Philox4x32-10 at counter (row, c1, c2, STREAM) under the seed."""
from __future__ import annotations

import numpy as np

from tests.feed_ref import philox4x32_10

STREAM = 0x50325753    # "P2WS"
TILE = 1024            # P2W_SAMPLE_TILE
N_MAX = 1 << 24        # P2W_SAMPLE_N_MAX


def keys(n, seed, c1, c2):
    """[n] uint32: the key of every row."""
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(n), c1 & 0xffffffff, c2 & 0xffffffff, STREAM
    return philox4x32_10(ctr, [seed & 0xffffffff, (seed >> 32) & 0xffffffff])[:, 0]


def subset(n, k, seed, c1, c2, keys=None):
    """[k] int64, ascending.  ``keys`` (any integer array of 32-bit patterns) replaces the generator."""
    key = globals()["keys"](n, seed, c1, c2) if keys is None else np.asarray(keys).astype(np.int64) & 0xffffffff
    return np.sort(np.lexsort((np.arange(n), key))[:k]).astype(np.int64)
