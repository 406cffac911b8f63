"""Stopping a training run after any step and continuing it in freshly built objects: ``trainer.save_state`` / ``load_state`` /
``restore_state``, ``--state_every``, ``--stop_at``, ``--resume`` and the stop request of ``trainer.SemanticTraining``.

Every comparison is bit for bit: whole runs (8 synthetic labelled voxels of 200 - 599 points, C = 8, batch_size 2 = 4 steps per epoch,
3 epochs, --test --augmentation, a checkpoint at every epoch) are compared file by file - the bytes of the history, every tensor of
every model file by its raw bits, which files exist, and the final state in full - between a run that was cut and continued and the
run that never stopped, in the default route (host draw, GradScaler, torch's AdamW, fp16) and with every opt-in flag on.  The
uninterrupted run of a route is made once per module and not written to."""
import argparse
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTES = {"default": {}, "all_flags": dict(device_sample=True, fused_step=True, fused_bn_max=True, amp="bf16")}
EPOCHS, STEPS = 3, 4
_cache = {}


@pytest.fixture(autouse=True)
def _no_stale_stop_request():
    from pointstowood_amd import trainer as TR
    TR.clear_stop()
    yield
    TR.clear_stop()


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """A directory with the voxel files (data/train: 8 voxels, data/test: the last 4 of them), written once."""
    from pointstowood_amd import synthetic_voxels as synth
    root = str(tmp_path_factory.mktemp("resume"))
    vox = []
    for i in range(8):
        n = 200 + 57 * i
        p, refl = synth.uniform_points(2.0, n, 50 + i, reflectance=True)
        label = (torch.rand(n, generator=torch.Generator().manual_seed(i)) < 0.3).float()
        vox.append(torch.cat([p, refl[:, None], label[:, None]], 1))
    for part, which in (("train", range(8)), ("test", range(4, 8))):
        d = os.path.join(root, "data", part, "voxels")
        os.makedirs(d)
        for k, i in enumerate(which):
            torch.save(vox[i].clone(), os.path.join(d, f"voxel_{k}.pt"))
    return root


def _run(base, name, route, **extra):
    """One ``SemanticTraining`` call in the working directory ``base/name`` (kept between calls: that is how a run is resumed)."""
    from pointstowood_amd.trainer import SemanticTraining
    wdir = os.path.join(base, name)
    os.makedirs(wdir, exist_ok=True)
    args = dict(wdir=wdir, model="model.pth", trfile=os.path.join(base, "data", "train", "voxels"),
                tefile=os.path.join(base, "data", "test", "voxels"), batch_size=2, num_epochs=EPOCHS,
                checkpoints=np.arange(0, EPOCHS + 1), augmentation=True, test=True, tune=False, stop_early=False, wandb=False, seed=5,
                C=8, max_pts=16384)
    args.update(ROUTES[route])
    args.update(extra)
    return wdir, SemanticTraining(argparse.Namespace(**args))


def _bits(t):
    """A tensor as integers of its element size: NaNs cannot hide, -0.0 is not 0.0."""
    t = t.detach().cpu().contiguous()
    if t.is_floating_point():
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _leaves(obj, prefix=""):
    """Every tensor and number of a nested dict / list / tuple as {path: comparable}."""
    out = {}
    if isinstance(obj, dict):
        for k, v in obj.items():
            out.update(_leaves(v, f"{prefix}/{k!r}"))
    elif isinstance(obj, (list, tuple)):
        out[prefix + "/#"] = (type(obj).__name__, len(obj))
        for k, v in enumerate(obj):
            out.update(_leaves(v, f"{prefix}/{k}"))
    elif torch.is_tensor(obj):
        out[prefix] = (str(obj.dtype), tuple(obj.shape), _bits(obj))
    else:
        out[prefix] = (type(obj).__name__, repr(obj))           # repr of a float is exact, and tells nan and -0.0 apart
    return out


def _same(a, b):
    if isinstance(a, tuple) and len(a) == 3 and torch.is_tensor(a[2]):
        return isinstance(b, tuple) and len(b) == 3 and a[:2] == b[:2] and torch.equal(a[2], b[2])
    return a == b


def _assert_same_leaves(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    different = [k for k in a if not _same(a[k], b[k])]
    assert not different, (what, different[:8])


def _snapshot(wdir):
    """{relative path: content} of everything the run left under model/ and checkpoints/: bytes of the history, leaves of the rest."""
    out = {}
    for folder in ("model", "checkpoints"):
        for f in sorted(os.listdir(os.path.join(wdir, folder))) if os.path.isdir(os.path.join(wdir, folder)) else []:
            path, rel = os.path.join(wdir, folder, f), folder + "/" + f
            if f.endswith(".csv"):
                out[rel] = open(path, "rb").read()
            elif f.endswith(".pth"):
                out[rel] = _leaves(torch.load(path, map_location="cpu", weights_only=True))
            else:
                out[rel] = None                                  # (a .tmp: only its presence)
    return out


STATE = "model/model_state.pth"
ALL_FILES = sorted(["model/model.pth", "model/model_history.csv", STATE, "model/ba-model.pth", "model/f1-model.pth",
                    "model/precision-model.pth"] + [f"checkpoints/epoch_{e}.pth" for e in range(1, EPOCHS + 1)])


def _assert_equal_runs(a, b, state=True):
    """Two snapshots are the same run: the same files (``state=False``: the state file left aside), the same bytes and bits."""
    a, b = ({k: v for k, v in s.items() if state or k != STATE} for s in (a, b))
    assert sorted(a) == sorted(b)
    for rel in a:
        if isinstance(a[rel], dict):
            _assert_same_leaves(a[rel], b[rel], rel)
        else:
            assert a[rel] == b[rel], rel


def _reference(base, route):
    """The uninterrupted run of ``route`` with state_every = 0, once."""
    if route not in _cache:
        wdir, history = _run(base, f"ref_{route}", route, state_every=0)
        snap = _snapshot(wdir)
        assert history.shape == (EPOCHS, 11) and np.isfinite(history).all()
        # the best models are written from epoch 2 on (epoch > 0.5 * 3) where a figure is above 0: told apart here, equal below
        assert set(snap) <= set(ALL_FILES) and set(ALL_FILES) - set(snap) <= {"model/ba-model.pth", "model/f1-model.pth",
                                                                               "model/precision-model.pth"}
        state = torch.load(os.path.join(wdir, "model", "model_state.pth"), map_location="cpu", weights_only=True)
        assert (state["format"], state["epoch"], state["step"]) == (1, EPOCHS + 1, 0) and state["history"].dtype == torch.float64
        assert np.array_equal(state["history"].numpy().view(np.int64), history.view(np.int64)) and state["scores"]["batches"] == 0
        _cache[route] = snap
    return _cache[route]


@pytest.mark.parametrize("route", list(ROUTES))
def test_control_two_uninterrupted_runs_are_equal(base, route):
    """What makes a failure below a finding about the resume and not about the stack's determinism."""
    ref = _reference(base, route)
    wdir, _ = _run(base, f"control_{route}", route, state_every=0)
    _assert_equal_runs(_snapshot(wdir), ref)


@pytest.mark.parametrize("route", list(ROUTES))
def test_stop_and_resume_at_an_epoch_boundary(base, route):
    ref = _reference(base, route)
    wdir, history = _run(base, f"boundary_{route}", route, stop_at=(2, 0))
    state = torch.load(os.path.join(wdir, "model", "model_state.pth"), map_location="cpu", weights_only=True)
    assert (state["epoch"], state["step"]) == (2, 0) and history.shape == (1, 11)
    assert not os.path.exists(os.path.join(wdir, "checkpoints", "epoch_2.pth"))
    wdir, history = _run(base, f"boundary_{route}", route, resume=True)
    assert history.shape == (EPOCHS, 11)
    _assert_equal_runs(_snapshot(wdir), ref)


@pytest.mark.parametrize("route", list(ROUTES))
def test_stop_and_resume_in_the_middle_of_an_epoch(base, route):
    """The cut that needs the open epoch's scores, the sampler's step, the CPU generator and the feed's start position."""
    ref = _reference(base, route)
    wdir, history = _run(base, f"middle_{route}", route, stop_at=(2, 2))
    state = torch.load(os.path.join(wdir, "model", "model_state.pth"), map_location="cpu", weights_only=True)
    assert (state["epoch"], state["step"], state["scores"]["batches"]) == (2, 2, 2) and history.shape == (1, 11)
    assert tuple(state["scores"]["counts"].shape) == (2, 5) and bool(torch.isfinite(state["scores"]["losses"]).all())
    if route == "all_flags":
        assert state["sampler"] == {"seed": 5, "epoch": 2, "step": 2} and "record" in state["optimizer"] and not state["scaler"]
    else:
        assert state["sampler"] is None and state["scaler"]["scale"] > 0
    first_leg = open(os.path.join(wdir, "model", "model_history.csv"), "rb").read()
    wdir, history = _run(base, f"middle_{route}", route, resume=True)
    got = _snapshot(wdir)
    # the resumed epoch's row is a function of its four per-batch matrices and losses, two of them from the state: its bits
    rows, ref_rows = got["model/model_history.csv"].splitlines(), ref["model/model_history.csv"].splitlines()
    assert len(rows) == EPOCHS and rows[1] == ref_rows[1] and rows[0] + b"\n" == first_leg
    _assert_equal_runs(got, ref)


@pytest.mark.parametrize("route", list(ROUTES))
def test_two_cuts(base, route):
    ref = _reference(base, route)
    name = f"cuts_{route}"
    wdir, history = _run(base, name, route, stop_at=(1, 3))
    assert history is None
    wdir, history = _run(base, name, route, resume=True, stop_at=(3, 1))
    state = torch.load(os.path.join(wdir, "model", "model_state.pth"), map_location="cpu", weights_only=True)
    assert (state["epoch"], state["step"]) == (3, 1) and history.shape == (2, 11)
    wdir, history = _run(base, name, route, resume=True)
    _assert_equal_runs(_snapshot(wdir), ref)


@pytest.mark.parametrize("route", list(ROUTES))
def test_saving_does_not_perturb_the_run(base, route, monkeypatch):
    """state_every = 3 without any stop: states at step 3 of every epoch and at every epoch's end, and every file but the state
    itself as in a run without the flag (and as in the reference, whose state_every is 0)."""
    from pointstowood_amd import trainer as TR
    ref = _reference(base, route)
    positions, inner = [], TR.save_state

    def watched(path, **k):
        positions.append((k["epoch"], k["step"]))
        return inner(path, **k)
    monkeypatch.setattr(TR, "save_state", watched)
    with_flag, _ = _run(base, f"every3_{route}", route, state_every=3)
    assert positions == [(1, 3), (2, 0), (2, 3), (3, 0), (3, 3), (4, 0)]
    without, _ = _run(base, f"plain_{route}", route)
    assert len(positions) == 6
    a, b = _snapshot(with_flag), _snapshot(without)
    assert STATE in a and STATE not in b
    _assert_equal_runs(a, b, state=False)
    _assert_equal_runs(a, ref)                                   # the final state too: (4, 0) in both


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_stop_request_before_the_first_step(base, route):
    from pointstowood_amd import trainer as TR
    ref = _reference(base, route)
    TR.request_stop()
    wdir, history = _run(base, f"request_{route}", route, resume=True)
    assert history is None and not TR.stop_requested()
    state = torch.load(os.path.join(wdir, "model", "model_state.pth"), map_location="cpu", weights_only=True)
    assert (state["epoch"], state["step"]) == (1, 0) and tuple(state["history"].shape) == (0, 11)
    assert sorted(os.listdir(os.path.join(wdir, "model"))) == ["model.pth", "model_state.pth"]
    wdir, history = _run(base, f"request_{route}", route, resume=True)
    assert history.shape == (EPOCHS, 11)
    _assert_equal_runs(_snapshot(wdir), ref)


def test_a_resume_that_cannot_be_exact_is_refused(base):
    """Another batch_size, seed, amp or fused_step, or a voxel fewer: ValueError naming the field, the state file's bytes as they
    were, no history written.  A leftover .tmp of garbage beside the valid state disturbs nothing."""
    ref = _reference(base, "default")
    name = "refused"
    wdir, _ = _run(base, name, "default", stop_at=(1, 2))
    state_path = os.path.join(wdir, "model", "model_state.pth")
    before, files = open(state_path, "rb").read(), sorted(os.listdir(os.path.join(wdir, "model")))
    assert "model_history.csv" not in files
    fewer = os.path.join(base, "data", "train_fewer")
    shutil.copytree(os.path.join(base, "data", "train", "voxels"), fewer)
    os.remove(os.path.join(fewer, "voxel_7.pt"))
    for change, fields in ((dict(batch_size=4), ["batch_size"]), (dict(seed=6), ["seed"]), (dict(amp="bf16"), ["amp"]),
                           (dict(fused_step=True), ["fused_step"]), (dict(trfile=fewer), ["train_voxels", "train_lengths_sha256"]),
                           (dict(seed=6, num_epochs=4, checkpoints=np.arange(0, 5)), ["seed", "num_epochs"])):
        with pytest.raises(ValueError) as e:
            _run(base, name, "default", resume=True, **change)
        message = str(e.value)
        assert all(f in message for f in fields), (change, message)
        if "seed" in change:
            assert "seed: 5, 6" in message                       # both values, the saved one first
        assert open(state_path, "rb").read() == before and sorted(os.listdir(os.path.join(wdir, "model"))) == files
        assert not os.path.exists(os.path.join(wdir, "checkpoints"))
    with open(state_path + ".tmp", "wb") as f:
        f.write(b"\x00garbage, as a kill during a write leaves it" * 7)
    wdir, history = _run(base, name, "default", resume=True)
    assert not os.path.exists(state_path + ".tmp")               # overwritten by the next save and moved into place
    _assert_equal_runs(_snapshot(wdir), ref)


# ---- the state functions alone ---------------------------------------------------------------------------------------------------

def _two_voxel_feed():
    """Two voxels of 600 and 200 points (what BatchNorm at the coarse levels needs), one batch per epoch."""
    if "feed" not in _cache:
        from pointstowood_amd import feed as F
        from pointstowood_amd import synthetic_voxels as synth
        vox = []
        for i, (side, n) in enumerate(((0.5, 600), (0.35, 200))):
            p, refl = synth.uniform_points(side, n, 400 + i, reflectance=True)
            label = (torch.rand(n, generator=torch.Generator().manual_seed(40 + i)) < 0.3).float()
            vox.append(torch.cat([p, refl[:, None], label[:, None]], 1))
        _cache["feed"] = F.TrainingFeed(F.TrainingSet(vox, DEV), 2, augmentation=True, seed=3)
    return _cache["feed"]


def _objects(kind, seed):
    from pointstowood_amd import train as T
    from pointstowood_amd import trainer as TR
    from pointstowood_amd.optim import ClipAdamW
    torch.manual_seed(seed)
    net = T.Net(1, C=8).to(DEV).train()
    net.sampler = T.DeviceSampler(seed)
    params = [p for p in net.parameters() if p.requires_grad]
    if kind == "clip":
        opt, scaler = ClipAdamW(params, lr=1e-4, weight_decay=1e-2, max_norm=1.0, loss_scale=512.0), None
    else:
        opt, scaler = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-2), torch.amp.GradScaler("cuda", init_scale=512)
    sched = TR.CosineAnnealingWarmupRestarts(opt, first_cycle_steps=4, cycle_mult=1.0, max_lr=1e-3, min_lr=1e-5, warmup_steps=1,
                                             gamma=0.5)
    return net, opt, scaler, sched


def _step(net, opt, scaler, epoch, plant_inf=False):
    """One training step as the loop takes it, on the feed's batch of ``epoch`` -> (logits, y, loss)."""
    from pointstowood_amd import trainer as TR
    from pointstowood_amd.loss import Poly1FocalLoss
    feed = _two_voxel_feed()
    feed.set_epoch(epoch)
    data = next(iter(feed))
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        out = net(data)
        loss, _ = criterion(out, data.y)
    (opt.scale(loss) if scaler is None else scaler.scale(loss)).backward()
    if plant_inf:
        next(p for p in net.parameters() if p.grad is not None).grad.view(-1)[0] = float("inf")
    if scaler is None:
        opt.step()
    else:
        TR.finish_step(net, opt, scaler, "fp16")
    return out.detach(), data.y, loss.detach()


@pytest.mark.parametrize("kind", ["adamw", "clip"])
def test_state_functions_round_trip_every_piece(tmp_path, kind):
    from pointstowood_amd import train as T
    from pointstowood_amd import trainer as TR
    from pointstowood_amd.loss import EpochScores
    net, opt, scaler, sched = _objects(kind, 7)
    scores = EpochScores(capacity=4)
    initial = {k: v.clone() for k, v in net.state_dict().items()}
    for k, epoch in enumerate((1, 2, 3)):                       # a skipped step (planted inf), then two real ones
        scores.add(*_step(net, opt, scaler, epoch, plant_inf=k == 0))
        if k == 0:                                              # the skipped step moved no parameter
            assert all(torch.equal(_bits(v), _bits(initial[n])) for n, v in net.state_dict().items() if "num_batches" not in n
                       and "running_" not in n)
    if kind == "clip":
        rec = opt.read()
        assert (rec["skipped"], rec["t"], rec["scale"], rec["growth_tracker"]) == (1, 2, 256.0, 2)
    else:
        assert scaler.state_dict()["scale"] == 256.0 and scaler.state_dict()["_growth_tracker"] == 2
    for _ in range(5):
        sched.step()
    assert sched.cycle == 1 and sched.t == 1
    net.sampler.set_epoch(2)
    net.sampler.step = 3
    history = np.array([[1.0, 1e-4, 0.7, 0.5, 0.25, float("nan"), -0.0, 0.1, 0.2, 0.3, 1.0 / 3.0]])
    best = dict(zip(TR.BEST_KEYS, (0.0, 0.125, 1.0 / 3.0, 0.75, 0.5)))
    fingerprint = {"format": 1, "seed": 7, "amp": "fp16", "fused_step": kind == "clip", "train_lengths_sha256": "00" * 32}
    path = str(tmp_path / "model_state.pth")
    with open(path + ".tmp", "wb") as f:                        # a stale .tmp is overwritten
        f.write(b"stale")
    torch.manual_seed(11)
    torch.rand(5)
    TR.save_state(path, epoch=2, step=3, model=net, optimizer=opt, scaler=scaler, scheduler=sched, history=history, best=best,
                  consec_decreases=4, skipped=1, scores=scores, sampler=net.sampler, fingerprint=fingerprint)
    assert sorted(os.listdir(tmp_path)) == ["model_state.pth"]
    cpu_next, cuda_next = torch.rand(4), torch.rand(4, device=DEV)          # what the generators give behind the save
    torch.load(path, map_location="cpu", weights_only=True)

    net2, opt2, scaler2, sched2 = _objects(kind, 8)             # other weights, a fresh optimiser, scale 512, cycle 0
    state = TR.load_state(path, DEV)
    TR.restore_state(state, model=net2, optimizer=opt2, scaler=scaler2, scheduler=sched2, sampler=net2.sampler)
    assert torch.equal(torch.rand(4), cpu_next) and torch.equal(torch.rand(4, device=DEV), cuda_next)
    assert (state["epoch"], state["step"], state["consec_decreases"], state["skipped"]) == (2, 3, 4, 1)
    assert state["fingerprint"] == fingerprint and TR.fingerprint_mismatch(state["fingerprint"], fingerprint) == []
    assert state["best"] == best and state["history"].dtype == torch.float64
    assert np.array_equal(state["history"].numpy().view(np.int64), history.view(np.int64))
    assert all(v.is_cuda for v in state["model"].values())

    _assert_same_leaves(_leaves(net2.state_dict()), _leaves(net.state_dict()), "model")
    assert len(opt.state_dict()["state"]) > 100
    _assert_same_leaves(_leaves(opt2.state_dict()), _leaves(opt.state_dict()), "optimizer")
    if kind == "clip":
        assert opt2.read() == opt.read() and state["scaler"] == {}
    else:
        assert scaler2.state_dict() == scaler.state_dict() and scaler2.get_scale() == 256.0
    rates = []
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] != 1e-4
    for s, o in ((sched, opt), (sched2, opt2)):
        rates.append([])
        for _ in range(10):
            s.step()
            rates[-1].append(o.param_groups[0]["lr"])
    assert rates[0] == rates[1] and len(set(rates[0])) > 3 and sched2.state_dict() == sched.state_dict()
    assert net2.sampler.state_dict() == {"seed": 7, "epoch": 2, "step": 3}
    assert torch.equal(net2.sampler.draw(1, 501, DEV), net.sampler.draw(1, 501, DEV))

    # the two go on alike: two more steps (the scores' remaining adds among them), the same bits in everything
    scores2 = EpochScores.from_state(state["scores"], DEV)
    assert len(scores2) == 3
    for epoch in (4, 5):
        a = _step(net, opt, scaler, epoch)
        scores.add(*a)
        scores2.add(*_step(net2, opt2, scaler2, epoch))
    ra, rb = scores.result(), scores2.result()
    assert ra["matrices"].shape == (5, 2, 2) and np.isfinite(ra["losses"]).all()
    _assert_same_leaves(_leaves({k: torch.from_numpy(v) if isinstance(v, np.ndarray) else float(v) for k, v in rb.items()}),
                        _leaves({k: torch.from_numpy(v) if isinstance(v, np.ndarray) else float(v) for k, v in ra.items()}), "scores")
    _assert_same_leaves(_leaves(net2.state_dict()), _leaves(net.state_dict()), "model, two steps on")
    _assert_same_leaves(_leaves(opt2.state_dict()), _leaves(opt.state_dict()), "optimizer, two steps on")
    assert net2.sampler.state_dict() == net.sampler.state_dict() == {"seed": 7, "epoch": 2, "step": 5}
    assert not all(torch.equal(_bits(v), _bits(initial[n])) for n, v in net.state_dict().items())


def test_scores_state_of_an_empty_object():
    from pointstowood_amd.loss import EpochScores
    s = EpochScores(threshold=0.25, capacity=7).state()
    assert s["batches"] == 0 and tuple(s["counts"].shape) == (0, 5) and tuple(s["losses"].shape) == (0,) and s["capacity"] == 7
    back = EpochScores.from_state(s, DEV)
    assert len(back) == 0 and back.threshold == 0.25 and back.state()["capacity"] == 7
    assert back.result()["matrices"].shape == (0, 2, 2)


def test_feed_iterate_from_a_batch_is_the_tail_of_the_epoch():
    from pointstowood_amd import feed as F
    from pointstowood_amd import synthetic_voxels as synth
    vox = []
    for i in range(10):
        n = 200 + 41 * i
        p, refl = synth.uniform_points(2.0, n, 50 + i, reflectance=True)
        vox.append(torch.cat([p, refl[:, None], (torch.rand(n, generator=torch.Generator().manual_seed(i)) < 0.3).float()[:, None]], 1))
    feed = F.TrainingFeed(F.TrainingSet(vox, DEV), batch_size=3, shuffle=True, drop_last=True, augmentation=True, mode="train", seed=11)
    feed.set_epoch(4)
    assert len(feed) == 3
    full = [{k: v.clone() for k, v in b.tensors().items()} for b in feed]
    assert len(full) == 3
    built, inner = [], feed.batch

    def counting(ids, plan, epoch=None):
        built.append(tuple(int(i) for i in ids))
        return inner(ids, plan, epoch)
    feed.batch = counting
    for start in (0, 1, len(feed) - 1, len(feed)):
        del built[:]
        tail = [b.tensors() for b in feed.iterate(start=start)]
        assert len(tail) == len(built) == len(feed) - start      # the skipped batches are not built
        for got, want in zip(tail, full[start:]):
            _assert_same_leaves(_leaves(got), _leaves(want), f"start {start}")
    for bad in (-1, len(feed) + 1):
        with pytest.raises(ValueError):
            list(feed.iterate(start=bad))
