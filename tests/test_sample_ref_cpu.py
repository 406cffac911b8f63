"""The random k-subset without a GPU: tests/sample_ref.py against the definition in include/p2w.h (pinned draws, uniformity on fixed
inputs), the guards and the workspace arithmetic of p2w_random_subset, the command-line flag and train.DeviceSampler's counters."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pointstowood_amd import _lib
from tests import feed_ref as F
from tests import sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 141190


def test_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "p2w.h")).read()
    assert int(re.search(r"#define P2W_SAMPLE_STREAM (0x[0-9a-fA-F]+)u", hdr).group(1), 16) == _lib.SAMPLE_STREAM == R.STREAM == 0x50325753
    assert R.STREAM.to_bytes(4, "big") == b"P2WS" and R.STREAM != F.STREAM
    assert int(re.search(r"#define P2W_SAMPLE_TILE (\d+)", hdr).group(1)) == _lib.SAMPLE_TILE == R.TILE
    assert 1 << int(re.search(r"#define P2W_SAMPLE_N_MAX \(\(int64_t\)1 << (\d+)\)", hdr).group(1)) == _lib.SAMPLE_N_MAX == R.N_MAX >= 1 << 24


def test_reference_is_the_definition():
    """Ascending, distinct, k long; the key is word 0 at counter (row, c1, c2, STREAM); the two pinned draws fix the counter layout."""
    assert R.subset(7, 3, SEED, 0, 1).tolist() == [1, 4, 6]
    assert R.subset(7, 3, SEED, 1, 1).tolist() == [0, 3, 6]
    seed = (0x1234 << 32) | 0x9abcdef1
    key = R.keys(5, seed, 7, 9)
    assert key.dtype == np.uint32
    for i in range(5):
        assert key[i] == F.philox4x32_10(np.array([i, 7, 9, R.STREAM], dtype=np.uint64), [0x9abcdef1, 0x1234])[0]
    for n, k in [(1, 0), (1, 1), (2, 1), (65, 13), (1000, 500), (1000, 999), (1000, 1000)]:
        s = R.subset(n, k, seed, 2, 3)
        assert s.dtype == np.int64 and s.shape == (k,) and (np.diff(s) > 0).all() and (k == 0 or (0 <= s[0] and s[-1] < n))
        key = R.keys(n, seed, 2, 3).astype(np.int64)
        out = np.setdiff1d(np.arange(n), s)
        if 0 < k < n:                                             # every kept (key, row) is below every dropped one
            assert max((key[i], i) for i in s) < min((key[i], i) for i in out)
    assert R.subset(1000, 1000, seed, 2, 3).tolist() == list(range(1000))
    # planted keys: ties go to the lowest rows; patterns above 2^31 compare unsigned, whatever integer type carries them
    assert R.subset(6, 2, 0, 0, 0, keys=np.zeros(6, np.uint32)).tolist() == [0, 1]
    assert R.subset(4, 2, 0, 0, 0, keys=np.array([-1, 5, -2, 7], np.int32)).tolist() == [1, 3]
    assert R.subset(5, 3, 0, 0, 0, keys=np.array([9, 3, 9, 3, 9], np.uint32)).tolist() == [0, 1, 3]


def test_uniformity_on_fixed_inputs():
    """n = 64, k = 32, the 2 000 draws c1 = 0 .. 1999 at c2 = 1: every row's inclusion count within 4 standard deviations of 1 000 and
    every pair's joint count within 5 of 2000 k (k - 1) / (n (n - 1)).  Conditions on fixed inputs (the reference stays at 2.42 and
    3.48), not measurements."""
    n, k, draws = 64, 32, 2000
    member = np.zeros((draws, n))
    for c1 in range(draws):
        member[c1, R.subset(n, k, SEED, c1, 1)] = 1.0
    count = member.sum(0)
    sd = np.sqrt(draws / 4)
    worst = np.abs(count - draws / 2).max() / sd
    joint = (member.T @ member)[np.triu_indices(n, 1)]
    p = k * (k - 1) / (n * (n - 1))
    worst_pair = np.abs(joint - draws * p).max() / np.sqrt(draws * p * (1 - p))
    print(f"rows {worst:.2f} sd, pairs {worst_pair:.2f} sd")
    assert worst <= 4.0 and worst_pair <= 5.0


def test_ws_size_host_arithmetic_and_refusals():
    """4 bytes per row, 4 x 256 histogram bins, a control record, two counters per tile of 1024 rows and the scan's tile sums (one int per
    4096 counters and 256 bytes of slack), every region rounded up to the arena's 256 bytes; 0 for the sizes the call refuses."""
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for n in [0, 1, 2, 1023, 1024, 1025, 131072, (1 << 21) + 1025, 1 << 24]:
        tiles = (n + 1023) // 1024
        scan = 4 * ((max(2 * tiles, 1) + 4095) // 4096) + 256
        assert L.p2w_random_subset_ws_size(n) == up(4 * n) + up(4096) + up(16) + up(8 * tiles) + up(scan), n
    for n in [-1, (1 << 24) + 1, 1 << 40]:
        assert L.p2w_random_subset_ws_size(n) == 0, n


def test_argument_refusals_come_back_before_any_launch():
    """Fake addresses that are never dereferenced: every status below is returned before a launch (no GPU is needed)."""
    L = _lib.lib()
    A, U = 4096, 4100

    def call(n=10, k=5, keys=None, idx=A, keys_out=None, ws=A, ws_size=1 << 20):
        return L.p2w_random_subset(n, k, SEED, 0, 0, keys, idx, keys_out, ws, ws_size, None)
    assert call(n=-1, k=0) == -1 and call(k=-1) == -1 and call(k=11) == -1 and call(n=(1 << 24) + 1) == -1
    assert call(n=0, k=0) == 0 and call(k=0) == 0               # nothing to do: OK, nothing launched, nothing written
    assert call(n=0, k=0, idx=None, ws=None, ws_size=0) == 0
    assert call(idx=None) == -2 and call(ws=None) == -2
    assert call(ws=U) == -3 and call(idx=U) == -3 and call(keys=A + 2) == -3 and call(keys_out=A + 1) == -3
    # (4-byte aligned keys pass the alignment guard and reach the size guard)
    assert call(keys=U, keys_out=U, ws_size=L.p2w_random_subset_ws_size(10) - 1) == -4
    assert call(ws_size=L.p2w_random_subset_ws_size(10) - 1) == -4
    assert call(n=1 << 24, k=1, ws_size=L.p2w_random_subset_ws_size(1 << 24) - 1) == -4


def test_command_line_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--device_sample" in r.stdout
    sys.path.insert(0, ROOT)
    import train as cli
    assert cli.build_parser().parse_args([]).device_sample is False
    assert cli.build_parser().parse_args(["--device_sample"]).device_sample is True


def test_device_sampler_counters(monkeypatch):
    from pointstowood_amd import ops
    from pointstowood_amd import train as T
    calls = []

    def recorder(n, k, seed, counter=(0, 0), device="cuda", keys=None, return_keys=False):
        calls.append((n, k, seed, tuple(counter), device))
        return "drawn"
    monkeypatch.setattr(ops, "random_subset", recorder)
    s = T.DeviceSampler(SEED)
    assert (s.seed, s.epoch, s.step) == (SEED, 0, 0)
    assert s.draw(0, 801, "dev") == "drawn" and calls[-1] == (801, 400, SEED, (0, 0), "dev")
    s.step = 6
    s.set_epoch(3)
    assert (s.epoch, s.step) == (3, 0)
    s.step = 5                                                    # assignable: a resumed run continues
    for level in (0, 1, 2):
        s.draw(level, 100 >> level, "dev")
        assert calls[-1] == (100 >> level, (100 >> level) // 2, SEED, (4 * 5 + level, 3), "dev")
    assert s.step == 5                                            # drawing does not advance the step: Net.forward does


def test_net_hands_the_sampler_to_its_levels():
    from pointstowood_amd import train as T
    assert T.Net.sampler is None and T.SAModule.sampler is None
    net = T.Net(1, 4)
    levels = [net.sa1_module, net.sa2_module, net.sa3_module]
    assert [m.level for m in levels] == [0, 1, 2] and all(m.sampler is None for m in levels)
    s = T.DeviceSampler(1)
    net.sampler = s
    assert all(m.sampler is s for m in levels) and net.sampler is s
    net.sampler = None
    assert all(m.sampler is None for m in levels)
    assert len(net.state_dict()) == 257                           # neither attribute is state
