"""optim.ClipAdamW on the GPU: against torch's AdamW(foreach=False) + GradScaler(512) + clip_grad_norm_ on a small module, both judged by
the float64 restatement (tests/optim_ref.py); no host wait in step() and scale(); a parameter without a gradient; the state_dict round
trip; the scheduler's lr and beta1 in the record; one step of train.Net; trainer.SemanticTraining with fused_step."""
import io

import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu


class Small(torch.nn.Module):
    """A few Linear + BatchNorm1d layers and a scalar parameter: 11 tensors of 1 .. 96 elements."""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.BatchNorm1d(16), torch.nn.ReLU(), torch.nn.Linear(16, 8),
                                        torch.nn.BatchNorm1d(8), torch.nn.ReLU(), torch.nn.Linear(8, 1))
        self.gain = torch.nn.Parameter(torch.tensor(0.5))

    def forward(self, x):
        return self.body(x)[:, 0] * self.gain


def small(seed=3):
    torch.manual_seed(seed)
    return Small().cuda()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def hyper_of(opt, scaling=1):
    g = opt.param_groups[0]
    return dict(R.HYPER, lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"], scaling=scaling)


def test_against_plain_torch_judged_by_float64():
    """3 steps from the same initial values on the same (scaled) gradients, the second above max_norm: per tensor the fused route's
    relative L2 error against the float64 restatement is at most 8 x the plain route's own; where that is 0, the summed per-step caps
    bound the fused route's absolute error."""
    from pointstowood_amd.optim import ClipAdamW
    fused_net, plain_net = small(), small()
    names = [k for k, _ in fused_net.named_parameters()]
    fused = ClipAdamW(fused_net.parameters(), lr=1e-2, weight_decay=1e-2, loss_scale=512.0)
    plain = torch.optim.AdamW(plain_net.parameters(), lr=1e-2, weight_decay=1e-2, foreach=False)
    scaler = torch.amp.GradScaler("cuda", init_scale=512)
    ps = [p.detach().cpu().numpy().astype(np.float64) for p in fused_net.parameters()]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    caps = [np.zeros_like(p) for p in ps]
    state = R.new_state(512.0)
    n_total = sum(p.size for p in ps)
    gen = torch.Generator().manual_seed(8)
    for size in (0.02, 1.0, 0.05):
        gs = [(torch.randn(p.shape, generator=gen) * size * 512.0) for p in fused_net.parameters()]
        for net in (fused_net, plain_net):
            for p, g in zip(net.parameters(), gs):
                p.grad = g.clone().cuda()
        fused.step()
        scaler.scale(torch.zeros((), device="cuda"))
        scaler.unscale_(plain)
        torch.nn.utils.clip_grad_norm_(plain_net.parameters(), max_norm=1.0)
        scaler.step(plain)
        scaler.update()
        p_in, m_in, v_in = ps, ms, vs                               # the caps come from this step's float64 inputs
        ps, ms, vs, rec = R.step64(ps, [g.numpy() for g in gs], ms, vs, state, hyper_of(fused))
        for i in range(len(ps)):
            caps[i] = caps[i] + R.element_caps(p_in[i], gs[i].numpy(), m_in[i], v_in[i], rec, n_total)[0]
        state = {k: rec[k] for k in state}
        assert (rec["coef"] < 1.0) == (size == 1.0)
    got = fused.read()
    assert got["t"] == 3 and got["skipped"] == 0 and got["scale"] == 512.0 == scaler.get_scale() and got["found_inf"] == 0
    for name, want, pf, pp, cap in zip(names, ps, fused_net.parameters(), plain_net.parameters(), caps):
        ef = np.linalg.norm(pf.detach().cpu().numpy().astype(np.float64) - want) / np.linalg.norm(want)
        ep = np.linalg.norm(pp.detach().cpu().numpy().astype(np.float64) - want) / np.linalg.norm(want)
        print(f"{name}: relative L2 error fused {ef:.3g} plain {ep:.3g}")
        if ep > 0:
            assert ef <= 8 * ep, name
        else:
            assert (np.abs(pf.detach().cpu().numpy().astype(np.float64) - want) <= cap).all(), name
    for p in fused_net.parameters():                               # the moments are where torch keeps them
        assert set(fused.state[p]) == {"exp_avg", "exp_avg_sq"} and fused.state[p]["exp_avg"].shape == p.shape


def test_step_and_scale_wait_for_nothing():
    """scale(), backward() and step() under torch.cuda.set_sync_debug_mode("error"): a host wait would raise."""
    from pointstowood_amd.optim import ClipAdamW
    net = small()
    opt = ClipAdamW(net.parameters(), lr=1e-3)
    x = torch.randn(32, 6, device="cuda")
    opt.scale(net(x).square().mean()).backward()
    opt.step()                                                     # (the first step creates the moments and the workspace)
    before = [p.detach().clone() for p in net.parameters()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.zero_grad()
        loss = opt.scale(net(x).square().mean())
        loss.backward()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rec = opt.read()
    assert rec["t"] == 2 and rec["found_inf"] == 0
    assert all(not torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))
    plain = ClipAdamW(small().parameters(), loss_scale=None)
    l = torch.ones((), device="cuda")
    assert plain.scale(l) is l and float(opt.scale(l)) == 512.0


def test_a_parameter_without_a_gradient_is_left_out():
    from pointstowood_amd.optim import ClipAdamW
    net = small()
    opt = ClipAdamW(net.parameters(), lr=1e-2, weight_decay=0.1)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    for k, p in net.named_parameters():
        p.grad = None if k in ("gain", "body.3.weight") else torch.ones_like(p) * 512.0
    opt.step()
    for k, p in net.named_parameters():
        if k in ("gain", "body.3.weight"):
            assert torch.equal(bits(p), bits(before[k])) and not opt.state[p], k          # no decay either, no moments yet
        else:
            assert not torch.equal(p.detach(), before[k]), k
    assert opt.read()["t"] == 1


def test_a_non_finite_gradient_skips_the_step_and_halves_the_scale():
    from pointstowood_amd.optim import ClipAdamW
    net = small()
    opt = ClipAdamW(net.parameters(), lr=1e-2)
    x = torch.randn(32, 6, device="cuda")
    opt.scale(net(x).square().mean()).backward()
    opt.step()
    before = [p.detach().clone() for p in net.parameters()]
    moments = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in net.parameters()]
    opt.zero_grad()
    opt.scale(net(x).square().mean()).backward()
    net.body[3].weight.grad[2, 5] = float("nan")
    opt.step()
    rec = opt.read()
    assert (rec["found_inf"], rec["t"], rec["skipped"], rec["scale"], rec["growth_tracker"]) == (1, 1, 1, 256.0, 0)
    for p, b, (m, v) in zip(net.parameters(), before, moments):
        assert torch.equal(bits(p), bits(b)) and torch.equal(bits(opt.state[p]["exp_avg"]), bits(m))
        assert torch.equal(bits(opt.state[p]["exp_avg_sq"]), bits(v))
    assert float(opt.scale(torch.ones((), device="cuda"))) == 256.0


def test_state_dict_round_trip_continues_with_the_same_bits():
    from pointstowood_amd.optim import ClipAdamW
    a_net = small()
    a = ClipAdamW(a_net.parameters(), lr=1e-2, growth_interval=2)
    gen = torch.Generator().manual_seed(2)
    grads = [[torch.randn(p.shape, generator=gen).cuda() * 100.0 for p in a_net.parameters()] for _ in range(3)]
    for gs in grads[:2]:
        for p, g in zip(a_net.parameters(), gs):
            p.grad = g.clone()
        a.step()
    blob = io.BytesIO()
    torch.save({"model": a_net.state_dict(), "optimizer": a.state_dict()}, blob)
    blob.seek(0)
    ck = torch.load(blob, map_location="cuda")
    b_net = small(seed=99)
    b_net.load_state_dict(ck["model"])
    b = ClipAdamW(b_net.parameters(), lr=1.0, loss_scale=2.0)
    b.load_state_dict(ck["optimizer"])
    assert b.param_groups[0]["lr"] == 1e-2 and b.param_groups[0]["growth_interval"] == 2 and b.read() == a.read()
    assert b.param_groups[0]["scaling"] is True
    assert a.read()["scale"] == 1024.0 and a.read()["t"] == 2
    for net, opt in ((a_net, a), (b_net, b)):
        for p, g in zip(net.parameters(), grads[2]):
            p.grad = g.clone()
        opt.step()
    assert a.read() == b.read() and a.read()["t"] == 3
    for pa, pb in zip(a_net.parameters(), b_net.parameters()):
        assert torch.equal(bits(pa), bits(pb))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(bits(a.state[pa][k]), bits(b.state[pb][k])) and a.state[pa][k].data_ptr() != b.state[pb][k].data_ptr()


def test_the_record_shows_the_schedulers_lr_and_beta1():
    """OneCycleLR cycles betas[0] with lr: every step uses the group's current values, as torch's AdamW does."""
    from pointstowood_amd.optim import ClipAdamW
    net = small()
    opt = ClipAdamW(net.parameters(), lr=1e-3, weight_decay=0.1, loss_scale=None)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-2, total_steps=5, pct_start=0.4)
    seen = []
    for t in range(1, 5):
        for p in net.parameters():
            p.grad = torch.full_like(p, 0.01)
        hyper = hyper_of(opt, scaling=0)
        opt.step()
        rec = opt.read()
        S, caps = R.scalars64(hyper, t), R.scalar_caps(hyper, t)
        assert rec["t"] == t and rec["scale"] == 1.0
        for k in R.SCALARS:
            assert abs(rec[k] - S[k]) <= caps[k] * abs(S[k]), (t, k, rec[k], S[k])
        assert np.float32(rec["omb1"]) == np.float32(1.0 - hyper["beta1"]) and np.float32(rec["decay"]) == np.float32(1.0 - hyper["lr"] * 0.1)
        seen.append((hyper["lr"], hyper["beta1"]))
        sched.step()
    assert len({lr for lr, _ in seen}) == 4 and len({b for _, b in seen}) >= 3


def test_one_step_of_the_net():
    """train.Net at C = 8 on voxels of 600 and 200 points (tests/test_gpu_train_net.py's case) under float16 autocast, one step with
    ClipAdamW: every parameter is the documented function of its value, its gradient and the record, bit for bit - ReflectanceYesNo
    (zero gradients) and the depthwise biases (gradients exactly 0) decay only, everything else moved; the gradients are left as they
    were; the checkpoint loads into route A."""
    import pointstowood_amd
    from pointstowood_amd.loss import Poly1FocalLoss
    from pointstowood_amd.optim import ClipAdamW
    from tests import net_train_ref as NR
    from tests import test_gpu_train_net as TN
    torch.manual_seed(TN.SEED)
    d = TN._data(NR.inputs(TN.SEED))
    net = TN._net(None)
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    opt = ClipAdamW(net.parameters(), lr=1e-4, weight_decay=1e-2, loss_scale=512.0)
    before = {k: p.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        outputs = net(d)
        loss, _ = criterion(outputs, d.y)
    opt.scale(loss).backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    opt.step()
    rec = opt.read()
    assert len(grads) == 158 and (rec["found_inf"], rec["t"], rec["skipped"], rec["scale"]) == (0, 1, 0, 512.0)
    assert rec["inv_scale"] == 1 / 512 and 0 < rec["coef"] <= 1.0 and np.isfinite(rec["sumsq"])
    decay = np.float32(rec["decay"])
    assert decay == np.float32(1.0 - 1e-4 * 1e-2) and decay < 1
    moved = 0
    for k, p in net.named_parameters():
        g = grads[k]
        assert torch.equal(bits(p.grad), bits(g)), k               # g is only read
        z = np.zeros_like(before[k])
        want, m, v = R.replay32(before[k], g.cpu().numpy(), z, z, rec)
        got = p.detach().cpu().numpy()
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), k
        assert (opt.state[p]["exp_avg"].cpu().numpy().view(np.uint32) == m.view(np.uint32)).all(), k
        assert (opt.state[p]["exp_avg_sq"].cpu().numpy().view(np.uint32) == v.view(np.uint32)).all(), k
        if ".reflectanceyesno." in k or k.endswith("depthwise_conv.bias"):
            assert bool((g == 0).all()) and (got.view(np.uint32) == (before[k] * decay).view(np.uint32)).all(), k      # decay only
        else:
            assert not np.array_equal(got, before[k]), k
            moved += 1
    assert moved > 100
    blob = io.BytesIO()
    torch.save({"model_state_dict": net.state_dict()}, blob)
    blob.seek(0)
    route_a = pointstowood_amd.Net(1, C=NR.C)
    missing, unexpected = route_a.load_state_dict(torch.load(blob, map_location="cpu")["model_state_dict"], strict=True)
    assert not missing and not unexpected


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_semantic_training_with_the_fused_step(amp, tmp_path, capsys):
    """8 synthetic voxels, C = 8, batch_size 4, 2 epochs, --test, fused_step=True: a finite 2 x 11 history, the skipped count on both
    epoch lines in both amp modes, a final checkpoint that loads into route A, and the same history bits from a second run."""
    import pointstowood_amd
    from tests.test_gpu_bf16_io import _training_run, _voxels
    vox = _voxels()
    first = _training_run(str(tmp_path / "a"), vox, amp=amp, fused_step=True)
    assert capsys.readouterr().out.count("  Skipped ") == 2
    h = np.loadtxt(tmp_path / "a" / "model" / "model_history.csv")
    assert h.shape == (2, 11) and np.isfinite(h).all() and h[:, 0].tolist() == [1.0, 2.0]
    assert (h[:, 1] > 0).all() and (h[:, 2] > 0).all() and ((h[:, 3:] >= 0) & (h[:, 3:] <= 1)).all()
    ck = torch.load(tmp_path / "a" / "model" / "model.pth", map_location="cpu")
    assert list(ck) == ["model_state_dict"]
    missing, unexpected = pointstowood_amd.Net(1, C=8).load_state_dict(ck["model_state_dict"], strict=True)
    assert not missing and not unexpected
    assert _training_run(str(tmp_path / "b"), vox, amp=amp, fused_step=True) == first


def test_semantic_training_without_the_flag_never_enters_optim(tmp_path, monkeypatch):
    """fused_step=False gives the history bits of a namespace that never had the attribute, and no function of optim is called."""
    from pointstowood_amd import optim
    from tests.test_gpu_bf16_io import _training_run, _voxels

    def refuse(*a, **k):
        raise AssertionError("optim was entered without fused_step")
    for name in ("__init__", "step", "scale", "read", "state_dict", "load_state_dict"):
        monkeypatch.setattr(optim.ClipAdamW, name, refuse)
    vox = _voxels()
    absent = _training_run(str(tmp_path / "a"), vox)
    assert _training_run(str(tmp_path / "b"), vox, fused_step=False) == absent
