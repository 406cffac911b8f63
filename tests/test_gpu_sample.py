"""The random k-subset on the GPU: p2w_random_subset through the C ABI, bit for bit against tests/sample_ref.py, with a caller-owned
workspace filled with 0xFF bytes beforehand; then ``ops.random_subset``, ``train.DeviceSampler`` inside ``train.Net`` and
``trainer.SemanticTraining`` with ``device_sample``.  T = P2W_SAMPLE_TILE = 1024 rows per workgroup, 256 per wave, 64 per step; the scan of
the per-tile counters takes a second level above 2^21 rows."""
import argparse
import os

import numpy as np
import pytest
import torch

from pointstowood_amd import _lib
from tests import net_train_ref as NR
from tests import sample_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = (0x1234 << 32) | 0x9abcdef1
T = R.TILE
TWO_LEVEL = (1 << 21) + T + 1                       # 2 x 2050 tile counters: more than one 4096-entry tile of the scan


def _call(n, k, seed=SEED, c1=3, c2=5, keys=None, want_keys=False, fill=0xFF):
    """-> (idx [k] int64, keys_out [n] uint32 or None) as numpy arrays; every output is pre-filled with a value no draw can give."""
    L = _lib.lib()
    ws = torch.full((max(int(L.p2w_random_subset_ws_size(n)), 1),), fill, dtype=torch.uint8, device=DEV)
    idx = torch.full((k,), -7, dtype=torch.int64, device=DEV)
    kout = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device=DEV) if want_keys else None
    kin = None if keys is None else torch.from_numpy(np.asarray(keys, dtype=np.uint32).view(np.int32)).to(DEV)
    _lib.check(L.p2w_random_subset(n, k, seed, c1, c2, _lib.ptr(kin), _lib.ptr(idx) if k else None, _lib.ptr(kout), _lib.ptr(ws),
                                   ws.numel(), _lib.stream()), "p2w_random_subset")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), None if kout is None else kout.cpu().numpy().view(np.uint32)


SHAPES = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 1), (63, 31), (64, 32), (65, 32), (255, 127), (256, 128), (257, 128),
          (T - 1, (T - 1) // 2), (T, T // 2), (T + 1, (T + 1) // 2), (T + 1, 1), (T + 1, T), (T + 1, T + 1), (5 * T + 77, 1),
          (5 * T + 77, 5 * T + 76), (5 * T + 77, 5 * T + 77), (131072, 65536), (131072, 1), (131072, 131071), (TWO_LEVEL, TWO_LEVEL // 2)]


@pytest.mark.parametrize("n,k", SHAPES)
def test_bit_for_bit_against_the_reference(n, k):
    got, key = _call(n, k, want_keys=True)
    if k == 0:                                                    # nothing launched, nothing written - keys_out included
        assert got.shape == (0,) and (key == 0x5a5a5a5a).all()
        return
    assert np.array_equal(key, R.keys(n, SEED, 3, 5))
    assert np.array_equal(got, R.subset(n, k, SEED, 3, 5, keys=key))
    if k == n:
        assert np.array_equal(got, np.arange(n))


def test_counters_and_seed_reach_the_generator():
    n, k = 3000, 1500
    draws = {}
    for seed, c1, c2 in [(SEED, 0, 0), (SEED, 1, 0), (SEED, 0, 1), (SEED ^ 1, 0, 0), (SEED ^ (1 << 40), 0, 0), (141190, 0xffffffff, 0xfffffffe)]:
        got, _ = _call(n, k, seed=seed, c1=c1, c2=c2)
        assert np.array_equal(got, R.subset(n, k, seed, c1, c2)), (seed, c1, c2)
        draws[(seed, c1, c2)] = got.tobytes()
    assert len(set(draws.values())) == len(draws)


def _planted():
    n = 4 * T + 100
    i = np.arange(n, dtype=np.uint64)
    cases = {"all_equal": (np.full(n, 0x12345678), n // 2), "all_zero": (np.zeros(n), n // 3), "all_ones": (np.full(n, 0xffffffff), n - 1),
             "descending": ((n - 1 - i) * 70001, 1234)}
    # the threshold value 0x80000001 on rows 900 .. 1200 (across the tile boundary at 1024 and the wave boundary inside it), 100 rows
    # below it in two other tiles, everything else above: k = 300 takes the 100 and the lowest r = 200 of the 301 equal rows
    two = np.full(n, 0xf0000000)
    two[900:1201] = 0x80000001
    two[0:50] = 0x80000000
    two[2 * T + 500:2 * T + 550] = 0x7fffffff
    cases["threshold_straddles"] = (two, 300)
    # r rows of the threshold value in each of two tiles: the tie ranks carry over the scan
    cases["threshold_two_tiles"] = (np.where((i % 3) == 0, 7, 9), n // 3 - 400)
    for d in range(4):                                            # keys that differ in ONE digit only: that select pass decides alone
        digit = (i * 37 + 11) % 256
        base = 0xa5c3e17b & ~(0xff << (8 * d)) & 0xffffffff
        cases[f"digit{d}_only"] = (base | (digit << np.uint64(8 * d)), n // 2 + 3)
    return n, {name: (np.asarray(v, dtype=np.uint64).astype(np.uint32), k) for name, (v, k) in cases.items()}


PLANTED_N, PLANTED = _planted()


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_keys(name):
    keys, k = PLANTED[name]
    n = PLANTED_N
    got, key = _call(n, k, keys=keys, want_keys=True)
    assert np.array_equal(key, keys)
    assert np.array_equal(got, R.subset(n, k, 0, 0, 0, keys=keys))
    if name.startswith("all_"):
        assert np.array_equal(got, np.arange(k))
    if name == "descending":
        assert np.array_equal(got, np.arange(n - k, n))
    if name == "threshold_straddles":
        assert np.array_equal(got, np.concatenate([np.arange(0, 50), np.arange(900, 1100), np.arange(2 * T + 500, 2 * T + 550)]))


def test_same_bits_on_every_run_whatever_the_workspace_held():
    for n, k in [(5 * T + 77, 2 * T + 9), (131072, 65536)]:
        first, _ = _call(n, k)
        again, _ = _call(n, k)
        zeroed, _ = _call(n, k, fill=0x00)
        assert first.tobytes() == again.tobytes() == zeroed.tobytes()
    keys, k = PLANTED["threshold_straddles"]
    assert _call(PLANTED_N, k, keys=keys)[0].tobytes() == _call(PLANTED_N, k, keys=keys, fill=0x00)[0].tobytes()


def test_refused_calls_write_nothing():
    L = _lib.lib()
    idx = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(L.p2w_random_subset_ws_size(16)), dtype=torch.uint8, device=DEV)
    assert L.p2w_random_subset(16, 17, SEED, 0, 0, None, idx.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream()) == -1
    assert L.p2w_random_subset(16, 8, SEED, 0, 0, None, idx.data_ptr(), None, ws.data_ptr(), ws.numel() - 1, _lib.stream()) == -4
    assert L.p2w_random_subset(16, 0, SEED, 0, 0, None, idx.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert (idx == -7).all()


# ---- the operator ------------------------------------------------------------------------------------------------------------------

def test_operator_is_the_c_abi():
    from pointstowood_amd import ops
    for n, k in [(1, 0), (1, 1), (T + 1, T // 2), (131072, 65536)]:
        want, want_keys = _call(n, k, c1=9, c2=2)[0], R.keys(n, SEED, 9, 2)
        got = ops.random_subset(n, k, SEED, counter=(9, 2))
        assert got.dtype == torch.int64 and got.shape == (k,) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
        got, key = ops.random_subset(n, k, SEED, counter=(9, 2), return_keys=True)
        assert key.dtype == torch.int32 and np.array_equal(key.cpu().numpy().view(np.uint32), want_keys)
        assert np.array_equal(got.cpu().numpy(), want)
    keys, k = PLANTED["threshold_straddles"]
    planted = torch.from_numpy(keys.view(np.int32)).to(DEV)
    assert np.array_equal(ops.random_subset(PLANTED_N, k, 0, keys=planted).cpu().numpy(), R.subset(PLANTED_N, k, 0, 0, 0, keys=keys))
    assert ops.random_subset(0, 0, SEED).shape == (0,)
    with pytest.raises(ValueError):
        ops.random_subset(4, 5, SEED)
    with pytest.raises(RuntimeError):
        ops.random_subset(4, 2, SEED, device="cpu")


def test_operator_makes_no_host_wait():
    """Under torch's synchronisation watch in its raising mode the call completes: nothing in it waits for the device."""
    from pointstowood_amd import ops
    n = 65536
    ops.random_subset(n, n // 2, SEED, counter=(1, 1))           # (the library and the allocator's blocks are there before the watch)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ops.random_subset(n, n // 2, SEED, counter=(1, 1), device=torch.device(DEV))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert np.array_equal(got.cpu().numpy(), R.subset(n, n // 2, SEED, 1, 1))


# ---- the network -------------------------------------------------------------------------------------------------------------------

NET_SEED = 4


class _D:
    pass


def _data():
    inp = NR.inputs(NET_SEED)
    d = _D()
    d.pos, d.batch, d.reflectance, d.sf = (inp[k].cuda() for k in ("pos", "batch", "reflectance", "sf"))
    return d, inp["g"].cuda()


def _raise(num_points):
    raise AssertionError("random_sample was called")


def _net(sampler, train=True):
    """A seeded train.Net(1, 8) whose random_sample raises; what the sampler draws is recorded on it as `drawn` [(level, n, keep)]."""
    from pointstowood_amd import train as TR
    torch.manual_seed(NET_SEED)
    net = TR.Net(1, NR.C).cuda().train(train)
    for m in (net.sa1_module, net.sa2_module, net.sa3_module):
        m.random_sample = _raise
    if sampler is not None:
        sampler.drawn = []
        inner = sampler.draw

        def draw(level, n, device):
            keep = inner(level, n, device)
            sampler.drawn.append((level, n, keep))
            return keep
        sampler.draw = draw
        net.sampler = sampler
    return net


def _step(net, d, g):
    """forward under autocast and a backward: the logits' and every gradient's bits"""
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        out = net(d)
    (out.float() * g).sum().backward()
    torch.cuda.synchronize()
    return [out.detach().clone()] + [p.grad.detach().clone() for p in net.parameters() if p.grad is not None]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _expect(drawn, seed, step, epoch):
    assert [(level, n) for level, n, _ in drawn] == [(0, 800), (1, 400), (2, 200)]
    for level, n, keep in drawn:
        assert keep.dtype == torch.int64 and keep.is_cuda
        assert np.array_equal(keep.cpu().numpy(), R.subset(n, n // 2, seed, 4 * step + level, epoch)), (level, step, epoch)


def test_net_draws_its_samples_on_the_device():
    from pointstowood_amd import train as TR
    d, g = _data()
    a, b = TR.DeviceSampler(SEED), TR.DeviceSampler(SEED)
    a.set_epoch(2)
    b.set_epoch(2)
    net_a, net_b = _net(a), _net(b)
    first = _step(net_a, d, g)
    assert a.step == 1 and len(a.drawn) == 3
    _expect(a.drawn, SEED, 0, 2)
    assert len(first) > 50 and all(torch.isfinite(t.float()).all() for t in first)
    # an equal (seed, epoch, step) in another net: equal logits and gradients, bit for bit
    assert _same(first, _step(net_b, d, g))
    # the second forward draws other samples
    second = _step(net_a, d, g)
    assert a.step == 2 and len(a.drawn) == 6
    _expect(a.drawn[3:], SEED, 1, 2)
    assert not any(torch.equal(x[2], y[2]) for x, y in zip(a.drawn[:3], a.drawn[3:])) and not torch.equal(first[0], second[0])
    # set_epoch replays the epoch from its step 0; an assigned step continues from there
    a.set_epoch(2)
    assert a.step == 0
    assert _same(first, _step(net_a, d, g))
    b.set_epoch(2)
    b.step = 1
    assert _same(second, _step(net_b, d, g))
    a.set_epoch(3)
    _step(net_a, d, g)
    _expect(a.drawn[-3:], SEED, 0, 3)


def test_net_without_a_sampler_takes_the_host_draw():
    from pointstowood_amd import train as TR
    d, g = _data()
    net = _net(None)
    calls = []
    for m in (net.sa1_module, net.sa2_module, net.sa3_module):
        def sample(n, m=m):
            calls.append(n)
            return TR.SAModule.random_sample(m, n)
        m.random_sample = sample
    assert net.sampler is None
    torch.manual_seed(11)
    first = _step(net, d, g)
    assert calls == [800, 400, 200]
    torch.manual_seed(11)
    assert _same(first, _step(net, d, g)) and len(calls) == 6


def test_eval_mode_never_looks_at_the_sampler():
    from pointstowood_amd import train as TR
    d, _ = _data()
    s = TR.DeviceSampler(SEED)
    net = _net(s, train=False)
    with torch.no_grad():
        with_sampler = net(d).clone()
        net.sampler = None
        without = net(d).clone()
    assert torch.equal(with_sampler, without) and s.drawn == [] and s.step == 0


# ---- the trainer -------------------------------------------------------------------------------------------------------------------

def _training_run(wdir, vox):
    from pointstowood_amd.trainer import SemanticTraining
    for part, which in (("train", range(8)), ("test", range(4, 8))):
        folder = os.path.join(wdir, "data", part, "voxels")
        os.makedirs(folder)
        for j, i in enumerate(which):
            torch.save(vox[i].clone(), os.path.join(folder, f"voxel_{j}.pt"))
    args = argparse.Namespace(wdir=str(wdir), model="model.pth", trfile=os.path.join(wdir, "data", "train", "voxels"),
                              tefile=os.path.join(wdir, "data", "test", "voxels"), batch_size=4, num_epochs=2,
                              checkpoints=np.arange(0, 3, 2), augmentation=True, test=True, tune=False, stop_early=False, wandb=False,
                              seed=5, C=8, max_pts=16384, device_sample=True)
    SemanticTraining(args)
    return open(os.path.join(wdir, "model", "model_history.csv"), "rb").read()


def test_semantic_training_with_the_device_sample(tmp_path, monkeypatch):
    """8 synthetic labelled voxels of 200 - 487 points, C = 8, 2 epochs with device_sample and a random_sample that raises: it completes,
    the checkpoint loads into route A with strict=True, and a second run writes the same history bits."""
    import pointstowood_amd
    from pointstowood_amd import synthetic_voxels as synth
    from pointstowood_amd import train as TR
    monkeypatch.setattr(TR.SAModule, "random_sample", lambda self, num_points: _raise(num_points))
    seen = []
    epoch_of = TR.DeviceSampler.set_epoch
    monkeypatch.setattr(TR.DeviceSampler, "set_epoch", lambda self, e: (seen.append(e), epoch_of(self, e))[1])
    vox = []
    for i in range(8):
        n = 200 + 41 * i
        p, refl = synth.uniform_points(2.0, n, 50 + i, reflectance=True)
        label = (torch.rand(n, generator=torch.Generator().manual_seed(i)) < 0.3).float()
        vox.append(torch.cat([p, refl[:, None], label[:, None]], 1))
    first = _training_run(str(tmp_path / "a"), vox)
    assert seen == [1, 2]
    h = np.loadtxt(tmp_path / "a" / "model" / "model_history.csv")
    assert h.shape == (2, 11) and np.isfinite(h).all() and h[:, 0].tolist() == [1.0, 2.0]
    ck = torch.load(tmp_path / "a" / "model" / "model.pth", map_location="cpu")
    missing, unexpected = pointstowood_amd.Net(1, C=8).load_state_dict(ck["model_state_dict"], strict=True)
    assert not missing and not unexpected
    assert _training_run(str(tmp_path / "b"), vox) == first
