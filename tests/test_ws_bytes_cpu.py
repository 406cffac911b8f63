"""Every ``p2w_*_ws_bytes`` function that is host arithmetic alone, against the sizes the library gave before its workspaces
were described by one carve function each (tests/golden/ws_bytes.json).  A workspace's size is part of the C ABI's behaviour:
callers allocate exactly this much, so a change here is a change of every offset behind it.

``p2w_gemm_h2_sk_ws_bytes`` is left out: it scales with the device's CU count.

Re-record (only when a size is meant to change):  python -m tests.test_ws_bytes_cpu <library to record from> <its commit>
"""
import ctypes
import json
import os
import sys

import pytest

from pointstowood_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ws_bytes.json")

SMALL = [0, 1, 255, 256, 257, 4097]
NEG = -1
SA_PACK8 = _lib.SA_PACK8


def _grid():
    """(function, argument tuple) of every case: the small sizes, a workload-sized one and the documented failures (-> 0)."""
    g = []

    def add(fn, *cases):
        g.extend((fn, tuple(c) if isinstance(c, (tuple, list)) else (c,)) for c in cases)

    for fn, big in [("p2w_voxel_sample_ws_bytes", 2_000_000), ("p2w_morton_order_ws_bytes", 2_000_000),
                    ("p2w_sort_pairs_u64_ws_bytes", 20_000_000), ("p2w_key_runs_ws_bytes", 20_000_000),
                    ("p2w_cell_starts_ws_bytes", 300_000_000), ("p2w_euclid_cluster_ws_bytes", 20_000_000),
                    ("p2w_pathlen_grow_ws_bytes", 5_000_000)]:
        add(fn, *SMALL, big, NEG)
    add("p2w_voxel_sample_table_ws_bytes", *[(n, t) for n in SMALL for t in (1, 257, 4097)], (400_000, 1 << 22), (400_000, 1 << 30),
        (NEG, 4096), (4096, 0), (4096, -1), (4096, (1 << 30) + 1))
    add("p2w_pathlen_sssp_ws_bytes", *[(n, m) for n in SMALL for m in (0, 1, 4097)], (5_000_000, 40_000_000), (NEG, 10), (10, NEG))
    add("p2w_confusion_ws_bytes", *[(n, s, c) for n in SMALL for s, c in ((1, 2), (3, 3), (7, 8))], (20_000_000, 64, 2), (1 << 40, 1, 2),
        (NEG, 1, 2), (10, 0, 2), (10, 1, 1), (10, 1, 9))
    add("p2w_poly1_focal_ws_bytes", *SMALL, 4096, 20_000_000, 1 << 40, NEG, (1 << 40) + 1)
    add("p2w_gemm_h2_rowdot_ws_bytes", *[(m, n) for m in SMALL for n in (1, 64, 65, 256)], (400_000, 128), (NEG, 64), (10, 0), (10, NEG))
    add("p2w_sa_conv_h_ws_bytes", *[(m, f) for m in (0, 1, 3, 4, 5, 1025, 400_000, NEG) for f in (0, SA_PACK8, SA_PACK8 | _lib.SA_ITEM_256)])
    add("p2w_interp_bwd_ws_bytes", *[(m, kw, nc) for m in SMALL for kw, nc in ((1, 1), (3, 257), (100, 0))], (400_000, 3, 100_000),
        (4097, 3, 2),                                      # long runs: the split partial sums
        (NEG, 3, 10), (10, 0, 10), (10, 101, 10), (10, 3, NEG), (1 << 30, 3, 10))
    add("p2w_edge_l1_bwd_ws_bytes", *[(e, ns, c1) for e in SMALL for ns, c1 in ((1, 1), (257, 32), (0, 67))], (6_000_000, 400_000, 64),
        (4097, 2, 32), (4097, 2, 33),                      # long runs: both panel widths of the partial sums
        (NEG, 10, 32), (10, NEG, 32), (10, 10, 0), (0x7fffffff, 10, 32))
    add("p2w_relu_bn_max_ws_bytes", *[(e, m, c2) for e in (2, 255, 256, 257, 4097) for m, c2 in ((1, 1), (17, 64), (257, 67))],
        (6_000_000, 400_000, 128), (0, 1, 64), (1, 1, 64), (NEG, 1, 64), (10, 0, 64), (10, 1, 0), (10, 1 << 30, 1 << 9))
    return g


def _key(fn, args):
    return f"{fn}({', '.join(str(a) for a in args)})"


def _sizes(h):
    out = {}
    for fn, args in _grid():
        f = getattr(h, fn)
        f.restype, f.argtypes = _lib.SIGNATURES[fn]
        out[_key(fn, args)] = int(f(*args))
    return out


def test_grid_covers_every_host_only_ws_bytes_function():
    names = {n for n in _lib.SIGNATURES if n.endswith("_ws_bytes")} - {"p2w_gemm_h2_sk_ws_bytes"}
    assert {fn for fn, _ in _grid()} == names


def test_ws_bytes_equal_the_recorded_sizes():
    golden = json.load(open(GOLDEN))["sizes"]
    got = _sizes(_lib.lib())
    assert set(got) == set(golden)
    wrong = {k: (got[k], golden[k]) for k in got if got[k] != golden[k]}
    assert not wrong, f"(now, recorded): {wrong}"


@pytest.mark.parametrize("key", ["p2w_voxel_sample_ws_bytes(-1)", "p2w_voxel_sample_table_ws_bytes(4096, 0)",
                                 "p2w_voxel_sample_table_ws_bytes(4096, 1073741825)", "p2w_relu_bn_max_ws_bytes(1, 1, 64)",
                                 "p2w_poly1_focal_ws_bytes(1099511627777)", "p2w_key_runs_ws_bytes(257)",
                                 "p2w_cell_starts_ws_bytes(4097)"])
def test_fixture_holds_the_documented_cases(key):
    """The fixture is a recording, not a tautology: the failure arguments are in it as 0 (a negative n of the sampler is the
    documented 256), and the two packed sizes are no multiples of 256."""
    v = json.load(open(GOLDEN))["sizes"][key]
    if key.startswith(("p2w_key_runs", "p2w_cell_starts")):
        assert v % 256 != 0
    elif key == "p2w_voxel_sample_ws_bytes(-1)":
        assert v == 256
    else:
        assert v == 0


if __name__ == "__main__":
    json.dump({"recorded_from": sys.argv[2] if len(sys.argv) > 2 else os.path.basename(sys.argv[1]),
               "sizes": _sizes(ctypes.CDLL(sys.argv[1]))}, open(GOLDEN, "w"), indent=0, sort_keys=True)
    print("wrote", GOLDEN)
