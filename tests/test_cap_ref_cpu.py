"""The voxeliser's cap without a GPU: tests/cap_ref.py against the definition in include/p2w.h (pinned draws, the law of successive
sampling and the replacement mode's uniformity on fixed inputs), the guards and the workspace arithmetic of p2w_cap_subset, the two
command-line flags and the arguments of voxelise."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pointstowood_amd import _lib
from tests import cap_ref as R
from tests import feed_ref as F
from tests import sample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 141190
LAW_W = np.array([1e-3, 0.5, 1, 1, 2, 3, 5, 8], dtype=np.float32)


def test_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "p2w.h")).read()
    assert int(re.search(r"#define P2W_CAP_STREAM (0x[0-9a-fA-F]+)u", hdr).group(1), 16) == _lib.CAP_STREAM == R.STREAM == 0x50325743
    assert R.STREAM.to_bytes(4, "big") == b"P2WC"
    assert len({R.STREAM, R.STREAM ^ 1, F.STREAM, sample_ref.STREAM}) == 4          # every user of the generator has its own word
    for name, lib_value, ref_value in (("N", _lib.CAP_N_MAX, R.N_MAX), ("S", _lib.CAP_S_MAX, R.S_MAX), ("OUT", _lib.CAP_OUT_MAX, R.OUT_MAX)):
        assert 1 << int(re.search(r"#define P2W_CAP_%s_MAX \(\(int64_t\)1 << (\d+)\)" % name, hdr).group(1)) == lib_value == ref_value
    assert R.N_MAX >= sample_ref.N_MAX


def test_reference_is_the_definition():
    """The key is float32(-log((w0 + 0.5) 2^-32) / w) from word 0 at counter (row_id, c1, c2, STREAM); the pinned draws fix the counter
    layout, the key's arithmetic and the order of the output."""
    idx, key = R.subset(8, [0], [8], 3, LAW_W, SEED, 0, 1)
    assert idx.tolist() == [[3, 6, 7]]
    assert [hex(v) for v in key] == ['0x42eaa897', '0x3f49b9fd', '0x3f3fa2b0', '0x3e43724c', '0x3fb9566f', '0x3f0a1dec', '0x3da6470a',
                                     '0x3cf2ae2e']
    assert R.subset(8, [0], [8], 3, LAW_W, SEED, 1, 1)[0].tolist() == [[4, 5, 7]]
    assert R.subset(8, [0], [8], 3, LAW_W, SEED, 0, 1, row_id=np.arange(8)[::-1].copy())[0].tolist() == [[4, 6, 7]]
    seed = (0x1234 << 32) | 0x9abcdef1
    w = np.array([0.25, 3.0, 1e-30, 7.5, 1e30], dtype=np.float32)
    ids = np.array([5, (1 << 32) + 6, 7, 1 << 40, 9])                         # only the low 32 bits of a row's identity count
    key = R.race_keys(ids, w, seed, 7, 9)
    assert key.dtype == np.uint32
    for i in range(5):
        w0 = int(F.philox4x32_10(np.array([ids[i] & 0xffffffff, 7, 9, R.STREAM], dtype=np.uint64), [0x9abcdef1, 0x1234])[0])
        with np.errstate(over="ignore"):
            want = np.float32(-np.log((w0 + 0.5) * 2.0 ** -32) / float(w[i]))
        assert key[i] == want.view(np.uint32)
    assert 0 < key[4] < key[0] < key[2] < 0x7f800000
    # a key beyond float32 rounds to +inf, still a valid key below the pattern of the invalid rows: -log(u) / 1.5e-38 overflows from
    # -log(u) = 5.1 on, which 0.6 % of the rows reach
    tiny = R.race_keys(np.arange(4000), np.full(4000, 1.5e-38, np.float32), seed, 0, 0)
    assert (tiny <= 0x7f800000).all() and 5 <= (tiny == 0x7f800000).sum() <= 60
    # weights that are not finite and positive: the pattern behind every valid key, +inf included
    bad = R.race_keys(np.arange(6), np.array([0.0, -1.0, np.inf, -np.inf, np.nan, -0.0], np.float32), seed, 0, 0)
    assert (bad == 0xFFFFFFFF).all()
    # rows of such a weight are taken only when valid rows run out, lowest positions first; -1 behind a short segment
    w = np.array([0.0, 2.0, np.nan, 1.0, -3.0, 4.0], dtype=np.float32)
    assert R.subset(6, [0], [6], 3, w, seed, 0, 0)[0].tolist() == [[1, 3, 5]]
    assert R.subset(6, [0], [6], 5, w, seed, 0, 0)[0].tolist() == [[0, 1, 2, 3, 5]]
    assert R.subset(6, [0, 4], [4, 2], 5, w, seed, 0, 0)[0].tolist() == [[0, 1, 2, 3, -1], [4, 5, -1, -1, -1]]
    # starts and counts are clamped to the row space
    assert R.select(6, [-3, 4, 9], [2, 10, 1], 2, np.zeros(6)).tolist() == [[0, 1], [4, 5], [-1, -1]]
    # planted keys: ties go to the lowest positions; patterns above 2^31 compare unsigned; the output is ascending by position
    assert R.select(6, [1], [5], 2, np.zeros(6, np.uint32)).tolist() == [[1, 2]]
    assert R.select(4, [0], [4], 2, np.array([-1, 5, -2, 7], np.int32)).tolist() == [[1, 3]]
    assert R.select(5, [0], [5], 3, np.array([9, 3, 9, 3, 9], np.uint32)).tolist() == [[0, 1, 3]]
    # a segment's sample is a function of its own (row_id, weight) pairs: alone, or behind another segment
    w = np.arange(1, 41, dtype=np.float32)
    alone = R.subset(40, [0], [40], 7, w, seed, 2, 3, row_id=np.arange(100, 140))[0]
    moved = R.subset(60, [0, 20], [20, 40], 7, np.concatenate([np.ones(20, np.float32), w]), seed, 2, 3,
                     row_id=np.concatenate([np.arange(20), np.arange(100, 140)]))[0]
    assert (moved[1] - 20).tolist() == alone[0].tolist()


def test_replacement_mode_is_the_integer_formula():
    assert R.replace(100, [10, 50], [7, 30], 6, SEED, 4).tolist() == [[11, 14, 14, 16, 13, 10], [51, 67, 53, 79, 52, 66]]
    assert R.replace(100, [10, 50], [7, 30], 6, SEED, 4, row_id=np.arange(100) + 5).tolist() == [[10, 10, 13, 13, 15, 14],
                                                                                                 [59, 61, 66, 55, 78, 63]]
    seed = (0x1234 << 32) | 0x9abcdef1
    got = R.replace(40, [3, 40], [29, 5], 4, seed, 9)
    for j in range(4):
        w0 = int(F.philox4x32_10(np.array([j, 3, 9, R.STREAM ^ 1], dtype=np.uint64), [0x9abcdef1, 0x1234])[0])
        assert got[0, j] == 3 + (w0 * 29 >> 32)
    assert got[1].tolist() == [-1] * 4                                          # an empty segment (clamped)


def test_the_law_of_successive_sampling_on_fixed_inputs():
    """Weights (1e-3, 0.5, 1, 1, 2, 3, 5, 8), k = 3, the 20 000 draws c2 = 0 .. 19999 at c1 = 0, seeds 1, 2 and 141190, against the
    exact probabilities of torch.multinomial's law (draw after draw proportional to the weights still there), enumerated over the 336
    ordered triples: every inclusion count and every pair count whose expected value is at least 100 lies within 4.5 standard
    deviations (the restatement stays at 2.68 over all such cells and seeds).  The row of weight 1e-3 is expected 4.3 times: it is held
    to at most 20 (a Poisson tail below 1e-7).  Conditions on fixed inputs, not measurements."""
    W = LAW_W.astype(np.float64)
    p1, p2 = np.zeros(8), np.zeros((8, 8))
    for t in itertools.permutations(range(8), 3):
        p = W[t[0]] / W.sum() * W[t[1]] / (W.sum() - W[t[0]]) * W[t[2]] / (W.sum() - W[t[0]] - W[t[1]])
        p1[list(t)] += p
        for a, b in itertools.combinations(sorted(t), 2):
            p2[a, b] += p
    assert abs(p1.sum() - 3) < 1e-12 and abs(p2.sum() - 3) < 1e-12
    draws = 20000
    small = draws * p1 < 100
    assert small.tolist() == [True] + [False] * 7 and 4.0 < draws * p1[0] < 4.5
    for seed in (1, 2, SEED):
        keys = R.race_keys(np.arange(8)[None, :], LAW_W[None, :], seed, 0, np.arange(draws)[:, None]).astype(np.int64)
        kept = np.lexsort((np.broadcast_to(np.arange(8), keys.shape), keys), axis=1)[:, :3]
        member = np.zeros((draws, 8))
        np.put_along_axis(member, kept, 1.0, axis=1)
        assert (member.sum(1) == 3).all()
        count, joint = member.sum(0), member.T @ member
        dev1 = np.abs(count - draws * p1) / np.sqrt(draws * p1 * (1 - p1))
        iu = np.triu_indices(8, 1)
        e2 = draws * p2[iu]
        dev2 = (np.abs(joint[iu] - e2) / np.sqrt(e2 * (1 - p2[iu])))[e2 >= 100]
        assert (e2 >= 100).sum() >= 21
        print(f"seed {seed}: rows {dev1[~small].max():.2f} sd, pairs {dev2.max():.2f} sd, row 0 taken {int(count[0])} times")
        assert dev1[~small].max() <= 4.5 and dev2.max() <= 4.5
        assert count[0] <= 20


def test_replacement_uniformity_on_fixed_inputs():
    """One segment of 7 rows, 20 000 draws: every position's count within 4.5 standard deviations of 20 000 / 7 (the restatement stays
    at 1.56)."""
    draws = 20000
    got = R.replace(50, [20], [7], draws, SEED, 0)[0]
    assert got.min() >= 20 and got.max() < 27
    count = np.bincount(got - 20, minlength=7)
    worst = np.abs(count - draws / 7).max() / np.sqrt(draws / 7 * 6 / 7)
    print(f"positions {worst:.2f} sd")
    assert worst <= 4.5


def test_ws_size_host_arithmetic_and_refusals():
    """4 bytes per row; per segment 4 x 256 histogram bins and a control record of two words; S + 1 tile offsets and their scan's tile
    sums; two counters per tile, n / 1024 + S + 1 tiles, and their scan's tile sums (one int per 4096 entries and 256 bytes of slack);
    every region rounded up to the arena's 256 bytes; 0 for the sizes the call refuses."""
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    scan = lambda m: 4 * ((max(m, 1) + 4095) // 4096) + 256
    for n, S in [(0, 0), (0, 3), (1, 1), (1023, 1), (1024, 2), (1025, 300), (131072, 4095), (131072, 4096), ((1 << 21) + 1025, 7),
                 (1 << 24, 1000), (1 << 30, 1 << 20)]:
        tiles = n // 1024 + S + 1
        want = up(4 * n) + up(4096 * S) + up(8 * S) + up(4 * (S + 1)) + up(scan(S + 1)) + up(8 * tiles) + up(scan(2 * tiles))
        assert L.p2w_cap_subset_ws_size(n, S) == want, (n, S)
    for n, S in [(-1, 1), ((1 << 30) + 1, 1), (1 << 40, 1), (10, -1), (10, (1 << 20) + 1)]:
        assert L.p2w_cap_subset_ws_size(n, S) == 0, (n, S)


def test_argument_refusals_come_back_before_any_launch():
    """Fake addresses that are never dereferenced: every status below is returned before a launch (no GPU is needed)."""
    L = _lib.lib()
    A, U4, U2 = 4096, 4100, 4098
    need = L.p2w_cap_subset_ws_size(100, 3)

    def call(n=100, start=A, count=A, S=3, k=5, weight=A, row_id=None, keys=None, idx=A, keys_out=None, ws=A, ws_size=1 << 20):
        return L.p2w_cap_subset(n, start, count, S, k, weight, row_id, SEED, 0, 0, keys, idx, keys_out, ws, ws_size, None)
    # sizes
    assert call(n=-1) == -1 and call(n=(1 << 30) + 1) == -1 and call(S=-1) == -1 and call(S=(1 << 20) + 1) == -1
    assert call(k=0) == -1 and call(k=-1) == -1 and call(k=(1 << 30) + 1) == -1 and call(S=1 << 20, k=(1 << 18) + 1) == -1
    assert call(S=0) == 0 and call(S=0, start=None, count=None, idx=None, ws=None, ws_size=0) == 0   # nothing to do, nothing launched
    # null
    assert call(start=None) == -2 and call(count=None) == -2 and call(idx=None) == -2 and call(ws=None) == -2
    assert call(weight=None, keys=A, ws=None) == -2
    # alignment: the workspace 16 bytes, the int64 arrays 8, the 32-bit arrays 4
    assert call(ws=U4) == -3 and call(start=U4) == -3 and call(count=U4) == -3 and call(idx=U4) == -3 and call(row_id=U4) == -3
    assert call(weight=U2) == -3 and call(keys=U2) == -3 and call(keys_out=U2) == -3
    assert call(weight=None, start=U4) == -3                                     # replacement mode keeps the guards of what it reads
    # workspace (4-byte aligned 32-bit arrays pass the alignment guard and reach the size guard)
    assert call(weight=U4, keys=U4, keys_out=U4, ws_size=need - 1) == -4 and call(ws_size=need - 1) == -4 and call(ws_size=0) == -4
    assert call(weight=None, keys=A, ws_size=need - 1) == -4
    assert call(n=1 << 24, S=1 << 10, ws_size=L.p2w_cap_subset_ws_size(1 << 24, 1 << 10) - 1) == -4


def test_operator_refuses_what_the_c_abi_refuses():
    """ops.cap_subset checks its arguments before it touches the library or a device."""
    import torch
    from pointstowood_amd import ops
    seg = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cap_subset(10, seg, seg, 3, SEED)


def test_command_line_flags():
    for script, flag in (("predict.py", "--cap_seed"), ("train.py", "--device_cap")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert flag in r.stdout
    sys.path.insert(0, ROOT)
    import predict as predict_cli
    import train as train_cli
    assert predict_cli.build_parser().parse_args([]).cap_seed is None
    assert predict_cli.build_parser().parse_args(["--cap_seed", "7"]).cap_seed == 7
    assert train_cli.build_parser().parse_args([]).device_cap is False
    assert train_cli.build_parser().parse_args(["--device_cap"]).device_cap is True


def test_voxelise_takes_a_cap_or_a_generator():
    import torch
    from pointstowood_amd import preprocessing as P
    cap = P.DeviceCap(SEED)
    assert (cap.seed, cap.counter) == (SEED, 0) and P.DeviceCap(3, counter=4).counter == 4
    with pytest.raises(ValueError, match="cap or generator"):
        P.voxelise(torch.zeros(4, 4), cap=cap, generator=torch.Generator())
    import inspect
    from pointstowood_amd import pipeline
    assert inspect.signature(P.voxelise).parameters["cap"].default is None
    assert inspect.signature(pipeline.segment_plot).parameters["cap"].default is None


def test_device_cap_makes_one_operator_call_per_grid_size(monkeypatch, tensor_backend):
    """The host-side logic of voxelise(cap=) on the tensor backend, with the operator replaced by a recorder that takes the first
    max_pts rows: one call per grid size over all oversized runs, row space = the cell-sorted order, row_id = the original point index,
    c1 = the grid's index, c2 = the cap's counter, weights only with reflectance; voxels under the cap are those of the host route."""
    import torch
    from pointstowood_amd import ops
    from pointstowood_amd import preprocessing as P
    from tests.test_host_cpu import _plot
    calls = []

    def recorder(n, seg_start, seg_count, k, seed, counter=(0, 0), weight=None, row_id=None, keys=None, return_keys=False):
        calls.append(dict(n=n, start=seg_start.tolist(), count=seg_count.tolist(), k=k, seed=seed, counter=tuple(counter),
                          weight=weight, row_id=row_id))
        return seg_start[:, None] + torch.arange(k)[None, :]
    monkeypatch.setattr(ops, "cap_subset", recorder)
    n = 20000
    for refl in (True, False):
        cloud = _plot(n=n, seed=2, refl=refl)
        calls.clear()
        full, _ = P.voxelise(cloud, (2.0, 4.0), 64, 100000, mode="xyz")
        host, nz_host = P.voxelise(cloud, (2.0, 4.0), 64, 300, mode="xyz", generator=torch.Generator().manual_seed(1))
        got, nz = P.voxelise(cloud, (2.0, 4.0), 64, 300, mode="xyz", cap=P.DeviceCap(9, counter=5))
        assert len(got) == len(host) == len(full) and torch.equal(nz, nz_host)
        over = [i for i, v in enumerate(full) if v.shape[0] > 300]
        assert len(over) >= 4 and len(over) < len(full)
        # a grid size without an oversized voxel makes no call; the others one each, with the grid's index as c1
        assert 1 <= len(calls) <= 2 and [c["counter"][1] for c in calls] == [5] * len(calls) and calls[-1]["counter"][0] == 1
        assert all(c["seed"] == 9 and c["k"] == 300 and c["n"] == n and (c["weight"] is not None) == refl for c in calls)
        assert sum((c["count"] for c in calls), []) == [full[i].shape[0] for i in over]
        assert all(sorted(c["row_id"].tolist()) == list(range(n)) for c in calls)
        for i, (a, b, f) in enumerate(zip(got, host, full)):
            if i in over:
                assert torch.equal(a, f[:300])                                  # the recorder's rows, gathered from the sorted order
            else:
                assert torch.equal(a, b) and torch.equal(a, f)
