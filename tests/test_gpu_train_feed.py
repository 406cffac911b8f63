"""The training feed on the GPU: p2w_train_feed through the C ABI against float64 (tests/feed_ref.py) and against the fixtures recorded
from the reference (tests/golden/train_feed/), its generator against the pure-numpy Philox, its guards, then ``feed.TrainingFeed`` and
``trainer.SemanticTraining`` end to end.  References are computed once per module and not written to."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import feed_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 255, 256, 257, 600]                     # the chunk boundary from both sides, a one-point voxel, several chunks
OFFSETS = [(0.0, 0.0, 0.0), (3.0, -2.0, 1.0), (0.0, 0.0, 0.0), (-4.0, 5.0, 2.0), (300.0, 310.0, 20.0)]
MODES = [0, 1, 2, 2, 0]                             # keep, zero, perturb, perturb, keep
ROTATE = [False, True, True, False, True]
BATCHES = [(4, 0, 2), (3, 1, 4)]                    # permuted subsets of 3 of the V = 5 voxels
SEED, EPOCH = (0x1234 << 32) | 0x9abcdef1, 3


def _voxels(refl_zero=False):
    out = []
    for i, (n, off) in enumerate(zip(SIZES, OFFSETS)):
        g = torch.Generator().manual_seed(100 + i)
        xyz = torch.rand(n, 3, generator=g) * 2.0 + torch.tensor(off)
        refl = torch.zeros(n) if refl_zero else torch.rand(n, generator=g) * 2 - 1
        label = (torch.rand(n, generator=g) < 0.3).float()
        out.append(torch.cat([xyz, refl[:, None], label[:, None]], 1))
    return out


_cache = {}


def _setup():
    """The set, its plan and per voxel the float64 reference (pos, refl) with the per-element cap - once."""
    if _cache:
        return _cache
    from pointstowood_amd import feed as F
    vox = _voxels()
    g = torch.Generator().manual_seed(9)
    u_angles = torch.rand(5, 3, generator=g)
    u_refl = torch.tensor([0.9, 0.1, 0.3, 0.3, 0.9])
    u_pos = torch.tensor([0.9 if not r else 0.1 for r in ROTATE])
    plan = F.plan_from_draws(u_refl, u_pos, u_angles, "train")
    assert plan["refl_mode"].tolist() == MODES and plan["rotate"].astype(bool).tolist() == ROTATE
    noise = [(torch.randn(n, generator=g) * 0.1).numpy() for n in SIZES]
    ref = []
    for v in range(5):
        pc = vox[v].numpy()
        roll, pitch, yaw = R.rotation_matrices(u_angles[v].numpy())
        R64 = roll @ pitch @ yaw
        x = pc[:, :3].astype(np.float64)
        d = x - x.mean(axis=0)
        pos = d @ R64 if ROTATE[v] else d
        r = pc[:, 3].astype(np.float64)
        refl = r if MODES[v] == 0 else np.zeros_like(r) if MODES[v] == 1 else r + noise[v].astype(np.float64)
        ref.append(dict(pos=pos, refl=refl, y=pc[:, 4], cap=R.kernel_pos_cap(pc[:, :3], ROTATE[v], R64)))
    _cache.update(F=F, vox=vox, plan=plan, noise=noise, ref=ref, tset=F.TrainingSet(vox, DEV))
    return _cache


def _run(tset, plan, ids, noise=None, seed=SEED, epoch=EPOCH, words=False):
    """One call through the C ABI wrapper; everything back on the host as numpy."""
    from pointstowood_amd import feed as F
    lengths = tset.lengths[list(ids)]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out = F.train_feed(tset, torch.tensor(list(ids), dtype=torch.int32, device=DEV), torch.from_numpy(ptr).to(DEV), int(ptr[-1]),
                       F.plan_to_device(plan, DEV), seed, epoch, None if noise is None else torch.from_numpy(noise).to(DEV), words)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], ptr


def _slot_noise(S, ids):
    return np.concatenate([S["noise"][v] for v in ids]).astype(np.float32)


@pytest.mark.parametrize("ids", BATCHES)
def test_kernel_against_float64(ids):
    """pos within the per-element cap of feed_ref.kernel_pos_cap (one rounding of d, the rounding of R, three roundings of the
    product); reflectance and y bit for bit where kept or zeroed and within half an ulp of the sum where perturbed; sf bit for bit the
    float32 maximum recomputed from the written pos in the header's order; batch exact.  Measured worst error / cap: see the README."""
    S = _setup()
    (pos, refl, y, batch, sf, nonfinite), ptr = _run(S["tset"], S["plan"], ids, _slot_noise(S, ids))
    worst = 0.0
    for b, v in enumerate(ids):
        a, e = ptr[b], ptr[b + 1]
        ref = S["ref"][v]
        err = np.abs(pos[a:e].astype(np.float64) - ref["pos"])
        worst = max(worst, float((err / np.maximum(ref["cap"], 1e-300)).max()) if SIZES[v] > 1 else 0.0)
        assert (err <= ref["cap"]).all(), (v, float((err / ref["cap"]).max()))
        if MODES[v] == 2:
            assert (np.abs(refl[a:e].astype(np.float64) - ref["refl"]) <= 0.5 * np.spacing(np.abs(refl[a:e]))).all(), v
        else:
            assert np.array_equal(refl[a:e].astype(np.float64), ref["refl"]), v
            assert not np.signbit(refl[a:e]).any() or MODES[v] == 0
        assert np.array_equal(y[a:e], ref["y"]), v
        assert (batch[a:e] == b).all() and batch.dtype == np.int64
        assert sf[b].tobytes() == np.float32(R.sf_f32(pos[a:e])).tobytes(), (v, sf[b], R.sf_f32(pos[a:e]))
        if SIZES[v] == 1:
            assert (pos[a:e] == 0).all() and sf[b] == 0
    print(f"ids {ids}: worst pos error / cap = {worst:.3f}")
    assert (nonfinite == 0).all()


_fixture_runs = {}


def _fixture_run(name):
    """Our output for one recorded case (its draws through plan_from_draws, its noise by row) beside the float64 restatement."""
    if name not in _fixture_runs:
        from pointstowood_amd import feed as F
        c = R.load_cases()[name]
        pc = c["pc"]
        tset = F.TrainingSet([torch.from_numpy(pc)], DEV)
        plan = F.plan_from_draws(c["u_refl"], c["u_pos"], c["u_angles"][None], c["mode"])
        assert int(plan["refl_mode"][0]) == c["refl_mode"] and bool(plan["rotate"][0]) == c["rotate"]
        (pos, refl, y, batch, sf, nonfinite), _ = _run(tset, plan, (0,), c["noise"].astype(np.float32))
        p64, r64, sf64 = R.item_f64(pc[:, :3], pc[:, 3], c["refl_mode"], c["rotate"], c["u_angles"], c["noise"])
        roll, pitch, yaw = R.rotation_matrices(c["u_angles"])
        cap = R.kernel_pos_cap(pc[:, :3], c["rotate"], roll @ pitch @ yaw).max()
        _fixture_runs[name] = dict(c=c, pos=pos, refl=refl, y=y, sf=sf, p64=p64, r64=r64, sf64=sf64, cap=cap)
    return _fixture_runs[name]


@pytest.mark.parametrize("name", sorted(R.load_cases()))
def test_against_the_reference_fixtures(name):
    """On every tensor our error against float64 is at most the reference's own error against float64 plus our derived cap."""
    f = _fixture_run(name)
    c = f["c"]
    ours = np.abs(f["pos"].astype(np.float64) - f["p64"]).max()
    theirs = np.abs(c["pos"].astype(np.float64) - f["p64"]).max()
    print(f"{name}: pos ours {ours:.3e} reference {theirs:.3e} cap {f['cap']:.3e}")
    assert ours <= theirs + f["cap"]
    ours_r = np.abs(f["refl"].astype(np.float64) - f["r64"]).max()
    theirs_r = np.abs(c["reflectance"].astype(np.float64) - f["r64"]).max()
    assert ours_r <= theirs_r + (0.5 * np.spacing(np.abs(f["refl"])).max() if c["refl_mode"] == 2 else 0.0)
    assert np.array_equal(f["y"], c["y"])
    sf_cap = np.sqrt(3.0) * f["cap"] + 3 * R.U32 * f["sf64"] * 1.01          # feed_ref.reference_sf_cap's form on our pos cap
    assert abs(float(f["sf"][0]) - f["sf64"]) <= abs(float(c["sf"]) - f["sf64"]) + sf_cap


def test_more_accurate_than_the_reference_at_plot_coordinates():
    f = _fixture_run("plot300")
    ours = np.abs(f["pos"].astype(np.float64) - f["p64"]).max()
    theirs = np.abs(f["c"]["pos"].astype(np.float64) - f["p64"]).max()
    print(f"plot300: ours {ours:.3e} reference {theirs:.3e}")
    assert ours < theirs


def _generator_set():
    if "gen" not in _cache:
        S = _setup()
        plan = S["plan"].copy()
        plan["refl_mode"] = 2
        _cache["gen"] = (S["F"].TrainingSet(_voxels(refl_zero=True), DEV), plan)
    return _cache["gen"]


def test_generator_words_and_normal():
    """noise = NULL, reflectance 0 in: the output IS fl32(0.1f * z).  The words equal feed_ref's Philox bit for bit; z is held to
    feed_ref.z_cap, derived from the ulp bounds of the device logf / cosf and the correctly rounded sqrtf."""
    tset, plan = _generator_set()
    ids = (4, 1, 3)
    (pos, refl, y, batch, sf, nonfinite, words), ptr = _run(tset, plan, ids, words=True)
    point1 = float(np.float32(0.1))
    for b, v in enumerate(ids):
        a, e = ptr[b], ptr[b + 1]
        want = R.feed_words(SIZES[v], v, EPOCH, SEED)
        assert np.array_equal(words[a:e].view(np.uint32), want), v
        z = R.box_muller_f64(want)
        err = np.abs(refl[a:e].astype(np.float64) - point1 * z)
        cap = point1 * R.z_cap(want) + R.U32 * np.abs(point1 * z) * 1.001
        print(f"voxel {v}: worst noise error / cap = {float((err / cap).max()):.3f}")
        assert (err <= cap).all(), (v, float((err / cap).max()))
    # with a reflectance, the row is fl32(r + e) of the same e
    S = _setup()
    (_, refl2, *_), _ = _run(S["tset"], plan, ids)
    r = np.concatenate([S["vox"][v][:, 3].numpy() for v in ids])
    assert np.array_equal(refl2, r + refl)


def test_noise_depends_on_voxel_epoch_and_seed_only():
    tset, plan = _generator_set()
    (_, a, *_), pa = _run(tset, plan, (4, 1, 3))
    (_, b, *_), pb = _run(tset, plan, (1, 0, 2, 4))                         # another batch, slot and composition
    assert np.array_equal(a[pa[0]:pa[1]], b[pb[3]:pb[4]]) and np.array_equal(a[pa[1]:pa[2]], b[pb[0]:pb[1]])
    (_, c, *_), _ = _run(tset, plan, (4, 1, 3), epoch=EPOCH + 1)
    (_, d, *_), _ = _run(tset, plan, (4, 1, 3), seed=SEED + 1)
    (_, e, *_), _ = _run(tset, plan, (4, 1, 3))
    assert not np.array_equal(a, c) and not np.array_equal(a, d) and not np.array_equal(c, d) and np.array_equal(a, e)
    assert (a[pa[0]:pa[1]][:255] != a[pa[1]:pa[2]]).any()                  # and on the voxel


def test_nonfinite_row_is_counted_and_poisons_its_voxel_only():
    S = _setup()
    F = S["F"]
    vox = _voxels()
    vox[2][7, 1] = float("nan")
    ids = (4, 2, 3)
    (pos, refl, y, batch, sf, nonfinite), ptr = _run(F.TrainingSet(vox, DEV), S["plan"], ids, _slot_noise(S, ids))
    (pos0, refl0, y0, _, sf0, _), _ = _run(S["tset"], S["plan"], ids, _slot_noise(S, ids))
    assert nonfinite.tolist() == [0, 1, 0]
    assert np.isnan(sf[1]) and sf[0].tobytes() == sf0[0].tobytes() and sf[2].tobytes() == sf0[2].tobytes()
    keep = np.r_[ptr[0]:ptr[1], ptr[2]:ptr[3]]
    assert np.array_equal(pos[keep], pos0[keep]) and np.array_equal(refl, refl0) and np.array_equal(y, y0)
    assert np.isnan(pos[ptr[1]:ptr[2]]).any(axis=1).all()               # the voxel's centroid is NaN, as the reference's is


def test_refused_calls_launch_nothing():
    from pointstowood_amd import _lib
    S = _setup()
    tset, F = S["tset"], S["F"]
    L = _lib.lib()
    ids = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV)
    ptr = torch.tensor([0, 600, 601, 857], dtype=torch.int64, device=DEV)
    n, B = 857, 3
    plan = F.plan_to_device(S["plan"], DEV)
    outs = [torch.full((k,), -7.0, device=DEV) for k in (3 * n, n, n)] + [torch.full((n,), -7, dtype=torch.int64, device=DEV),
                                                                          torch.full((B,), -7.0, device=DEV),
                                                                          torch.full((B,), -7, dtype=torch.int32, device=DEV)]
    need = int(L.p2w_train_feed_ws_size(n, B))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    p = _lib.ptr

    def call(B=B, n=n, ws_ptr=p(ws), ws_size=need, xyzr=p(tset.xyzr)):
        return L.p2w_train_feed(xyzr, p(tset.y), p(tset.set_ptr), tset.num_points, 5, p(ids), p(ptr), B, n, p(plan), 1, 0, None,
                                *[p(o) for o in outs], None, ws_ptr, ws_size, _lib.stream())
    assert call(B=-1) == -1 and call(n=-1) == -1
    assert call(ws_size=need - 1) == -4
    assert call(ws_ptr=p(ws) + 4) == -3 and call(xyzr=p(tset.xyzr) + 4) == -3
    assert call(B=0) == 0 and call(n=0) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((outs[0] == -7).any()) and bool((outs[5] == 0).all())


# ---- TrainingFeed ------------------------------------------------------------------------------------------------------------------

def _ten():
    if "ten" not in _cache:
        from pointstowood_amd import feed as F
        from pointstowood_amd import synthetic_voxels as synth
        vox = []
        for i in range(10):
            n = 200 + 41 * i
            p, refl = synth.uniform_points(2.0, n, 50 + i, reflectance=True)
            label = (torch.rand(n, generator=torch.Generator().manual_seed(i)) < 0.3).float()
            vox.append(torch.cat([p, refl[:, None], label[:, None]], 1))
        _cache["ten"] = (vox, F.TrainingSet(vox, DEV))
    return _cache["ten"]


def _host(batch):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in batch.tensors().items()}


def test_feed_batches_contract_and_determinism():
    from pointstowood_amd import feed as F
    vox, tset = _ten()
    feed = F.TrainingFeed(tset, batch_size=4, shuffle=True, drop_last=True, augmentation=True, mode="train", seed=11)
    assert len(feed) == 2 and len(F.TrainingFeed(tset, 4, drop_last=False)) == 3
    feed.set_epoch(1)
    first = [_host(b) for b in feed]
    assert len(first) == 2
    order = feed.order()
    assert sorted(order.tolist()) == list(range(10))
    seen = []
    for i, b in enumerate(first):
        ids = order[4 * i:4 * i + 4]
        seen += ids.tolist()
        n = int(tset.lengths[ids].sum())
        assert b["pos"].shape == (n, 3) and b["pos"].dtype == torch.float32
        assert b["reflectance"].shape == (n,) and b["y"].shape == (n,) and b["sf"].shape == (4,)
        assert b["batch"].dtype == torch.int64 and b["ptr"].dtype == torch.int64 and b["batch"].shape == (n,)
        assert b["ptr"].tolist() == np.concatenate([[0], np.cumsum(tset.lengths[ids])]).tolist()
        assert torch.equal(b["batch"], torch.repeat_interleave(torch.arange(4), torch.from_numpy(tset.lengths[ids])))
        assert torch.equal(b["y"], torch.cat([vox[v][:, 4] for v in ids]))
    assert len(set(seen)) == 8                                             # no voxel twice
    again = F.TrainingFeed(tset, 4, augmentation=True, seed=11)
    again.set_epoch(1)
    for a, b in zip(first, again):
        assert b.num_graphs == 4
        b = _host(b)
        assert all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a)
    again.set_epoch(2)
    assert again.order().tolist() != order.tolist()
    assert again.plan().tobytes() != feed.plan().tobytes()


def test_feed_without_augmentation_is_collate_device():
    """collate_device takes the centroid by a float32 sum (error at most n u m per coordinate, m = the largest |coordinate|) and
    subtracts in float32 (one rounding, u |p|); ours errs by u |p| (+ the float64 sum, far below): the positions agree within
    (n + 2) u m, sf within sqrt(3) times that plus three float32 roundings of the norm.  y, reflectance, batch and ptr are exact."""
    from pointstowood_amd import feed as F
    from pointstowood_amd.predicter import collate_device
    vox, tset = _ten()
    feed = F.TrainingFeed(tset, 4, shuffle=False, drop_last=True, augmentation=False)
    for i, b in enumerate(feed):
        ids = list(range(4 * i, 4 * i + 4))
        want = _host(collate_device([vox[v].to(DEV) for v in ids]))
        got = _host(b)
        for k, v in enumerate(ids):
            a, e = int(got["ptr"][k]), int(got["ptr"][k + 1])
            n, m = e - a, float(vox[v][:, :3].abs().max())
            cap = (n + 2) * R.U32 * m
            assert float((got["pos"][a:e].double() - want["pos"][a:e].double()).abs().max()) <= cap
            assert abs(float(got["sf"][k]) - float(want["sf"][k])) <= np.sqrt(3.0) * cap + 3 * R.U32 * float(want["sf"][k])
        assert torch.equal(got["reflectance"], want["reflectance"]) and torch.equal(got["batch"], want["batch"])
        assert torch.equal(got["ptr"], want["ptr"]) and torch.equal(got["y"], torch.cat([vox[v][:, 4] for v in ids]))


def test_one_training_step_on_a_yielded_batch():
    from pointstowood_amd import feed as F
    from pointstowood_amd import train as T
    from pointstowood_amd.loss import Poly1FocalLoss
    _, tset = _ten()
    torch.manual_seed(0)
    net = T.Net(1, C=8).to(DEV).train()
    batch = next(iter(F.TrainingFeed(tset, 4, augmentation=True, seed=2)))
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    with torch.autocast("cuda", dtype=torch.float16):
        out = net(batch)
        loss, _ = criterion(out, batch.y)
    loss.backward()
    assert out.shape == batch.y.shape and bool(torch.isfinite(loss))
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)


# ---- SemanticTraining --------------------------------------------------------------------------------------------------------------

def _training_run(wdir, vox):
    from pointstowood_amd.trainer import SemanticTraining
    for part, which in (("train", range(8)), ("test", range(4, 8))):
        d = os.path.join(wdir, "data", part, "voxels")
        os.makedirs(d)
        for k, i in enumerate(which):
            torch.save(vox[i].clone(), os.path.join(d, f"voxel_{k}.pt"))
    args = argparse.Namespace(wdir=str(wdir), model="model.pth", trfile=os.path.join(wdir, "data", "train", "voxels"),
                              tefile=os.path.join(wdir, "data", "test", "voxels"), batch_size=4, num_epochs=2,
                              checkpoints=np.arange(0, 3, 2), augmentation=True, test=True, tune=False, stop_early=False, wandb=False,
                              seed=5, C=8, max_pts=16384)
    SemanticTraining(args)
    return open(os.path.join(wdir, "model", "model_history.csv"), "rb").read()


def test_semantic_training_end_to_end(tmp_path):
    """8 synthetic labelled voxels of 200 - 600 points, C = 8, batch_size 4, 2 epochs, --test --augmentation: a 2 x 11 history of finite
    values, a checkpoint that loads into route A with strict=True, and the same history bits from a second run with the same seed."""
    import pointstowood_amd
    vox, _ = _ten()
    first = _training_run(str(tmp_path / "a"), vox)
    h = np.loadtxt(tmp_path / "a" / "model" / "model_history.csv")
    assert h.shape == (2, 11) and np.isfinite(h).all() and h[:, 0].tolist() == [1.0, 2.0]
    assert (h[:, 1] > 0).all() and (h[:, 2] > 0).all() and ((h[:, 3:] >= 0) & (h[:, 3:] <= 1)).all()
    for path in (tmp_path / "a" / "checkpoints" / "epoch_2.pth", tmp_path / "a" / "model" / "model.pth"):
        ck = torch.load(path, map_location="cpu")
        assert list(ck) == ["model_state_dict"]
        missing, unexpected = pointstowood_amd.Net(1, C=8).load_state_dict(ck["model_state_dict"], strict=True)
        assert not missing and not unexpected
    assert os.path.exists(tmp_path / "a" / "model" / "ba-model.pth") or h[1, 7] == 0
    assert _training_run(str(tmp_path / "b"), vox) == first
