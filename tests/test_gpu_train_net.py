"""pointstowood_amd.train.Net on the GPU, on tests/net_train_ref.py's case (two voxels of 600 and 200 points, C = 8): the state dict,
eval mode against oracle/net.py over the operator module, one whole training step as the reference's trainer takes it, its
determinism, the fused route against the plain one judged by the float64 composition, and the fused = False switch."""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import net_train_ref as R

pytestmark = pytest.mark.gpu

SEED = 4
FUSED_OPS = ("bn_chain", "edge_layer1", "relu_bn", "relu_bn_max", "interp_add_relu", "bn_relu_rowdot")


class _D:
    pass


def _data(inp):
    d = _D()
    d.pos, d.batch, d.reflectance, d.sf = (inp[k].cuda() for k in ("pos", "batch", "reflectance", "sf"))
    d.y = (torch.rand(inp["pos"].shape[0], generator=torch.Generator().manual_seed(SEED)) < 0.3).float().cuda()
    return d


def _sa(net):
    return [net.sa1_module, net.sa2_module, net.sa3_module]


def _net(sd, fused=True, train=True):
    """train.Net(1, 8) on the GPU with `sd` loaded (None: as initialize_weights leaves it).  For training the fixed ascending sample
    is injected in place of random_sample; either sampler's result is recorded on the level as `seen_idx`."""
    from pointstowood_amd import train as T
    net = T.Net(1, R.C)
    if sd is not None:
        net.load_state_dict(sd, strict=True)
    net = net.cuda().train(train)
    if not fused:
        net.fused = False
    for m in _sa(net):
        def sample(n, m=m):
            m.seen_idx = R.fixed_sample(n)
            return m.seen_idx

        def voxels(pos, batch, resolution, m=m, inner=m.voxelsample):
            m.seen_idx = inner(pos, batch, resolution)
            return m.seen_idx
        m.random_sample, m.voxelsample = sample, voxels
    return net


@contextlib.contextmanager
def _searches():
    """Records what ops.radius and ops.knn return while it is open: a list of (target, source) in call order - the three
    set-abstraction levels' edges come first."""
    from pointstowood_amd import ops as H
    found, radius, knn = [], H.radius, H.knn

    def watched(fn):
        def call(*a, **k):
            found.append(fn(*a, **k))
            return found[-1]
        return call
    H.radius, H.knn = watched(radius), watched(knn)
    try:
        yield found
    finally:
        H.radius, H.knn = radius, knn


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_state_dict_is_the_reference():
    import pointstowood_amd
    from pointstowood_amd import synthetic_weights as SW
    from pointstowood_amd import train as T
    for nc, C in ((1, 8), (3, 4)):
        sd = T.Net(nc, C).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s, _ in SW.key_table(nc, C)] and len(sd) == 257
    route_a = pointstowood_amd.Net(1, C=8)
    missing, unexpected = route_a.load_state_dict(T.Net(1, 8).state_dict(), strict=True)
    assert not missing and not unexpected
    assert T.Net.fused is True and T.SAModule.fused is True and T.GlobalSAModule.fused is True


def test_eval_mode_is_the_oracle_composition():
    """Eval mode with a synthetic checkpoint: the logits equal oracle.net.forward over pointstowood_amd.ops within that composition
    test's own tolerances (tests/test_gpu_forward.py: rtol 1e-4, atol 4e-4); the sample indices and the edges are equal exactly."""
    from oracle import net as onet
    from pointstowood_amd import ops as H
    inp, sd = R.inputs(SEED), R.state(SEED)
    d = _data(inp)
    cap = {}
    want = onet.forward({k: v.cuda() for k, v in sd.items()}, d.pos, d.batch, d.reflectance, d.sf, capture=cap, ops=H)
    net = _net(sd, train=False)
    pos_before = d.pos.clone()
    with torch.no_grad(), _searches() as found:
        got = net(d)
    assert got.shape == (800,) and got.dtype == torch.float32 and torch.equal(d.pos, pos_before) and d.x.shape == (800, R.C)
    assert len(found) == 3
    for l, (m, (target, source)) in enumerate(zip(_sa(net), found), start=1):
        assert torch.equal(m.seen_idx, cap[f"sa{l}_module.idx"]) and int(m.seen_idx.numel()) >= 2
        assert torch.equal(target, cap[f"sa{l}_module.edge_q"]) and torch.equal(source, cap[f"sa{l}_module.edge_c"])
    torch.testing.assert_close(got, want, rtol=1e-4, atol=4e-4)
    assert all(int(v) == 0 for k, v in net.state_dict().items() if k.endswith("num_batches_tracked"))


_steps = []


def _train_step():
    """One step as trainer.py:106-186 takes it, seeded: a freshly initialised Net(1, 8), forward under autocast, Poly1FocalLoss,
    GradScaler(init_scale=512), unscale, clip_grad_norm_, AdamW.  Returns the net, the logits, the loss, the unscaled, clipped
    gradients and the state before the step.  (Not the synthetic checkpoint of the other tests: its gains of 4 and 25 put logits
    beyond 100, and the gradients scaled by 512 then overflow fp16 in PyTorch's own GEMM backward, on the plain route as on the
    fused one - the step that GradScaler skips.)"""
    from pointstowood_amd.loss import Poly1FocalLoss
    torch.manual_seed(SEED)
    d = _data(R.inputs(SEED))
    net = _net(None)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    optimizer = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=512)
    optimizer.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        outputs = net(d)
        loss, _ = criterion(outputs, d.y)
    scaler.scale(loss).backward()
    scaler.unscale_(optimizer)
    torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    scaler.step(optimizer)
    scaler.update()
    return net, outputs.detach(), loss.detach(), grads, sd


def _first_step():
    if not _steps:
        _steps.append(_train_step())
    return _steps[0]


def test_one_training_step(tmp_path):
    """After the step: every gradient is finite; the six reflectanceyesno gradients per level are zero tensors, not None; the
    depthwise biases' gradients are exactly zero (BatchNorm removes a bias in front of it: ops.bn_chain returns zeros, as documented
    there); every other parameter has a non-zero gradient and has moved; every BatchNorm's running statistics and
    num_batches_tracked moved; the checkpoint saved after the step loads into route A."""
    import pointstowood_amd
    net, logits, loss, grads, sd = _first_step()
    assert logits.shape == (800,) and logits.dtype == torch.float32 and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss))
    assert len(grads) == 158
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        if ".reflectanceyesno." in k or k.endswith("depthwise_conv.bias"):
            assert bool((g == 0).all()), k
        else:
            assert float(g.abs().max()) > 0, k
            assert not torch.equal(dict(net.named_parameters())[k].detach().cpu(), sd[k]), k
    after = net.state_dict()
    bns = [k[:-len(".running_mean")] for k in after if k.endswith(".running_mean")]
    assert len(bns) == 33
    for p in bns:
        assert int(after[p + ".num_batches_tracked"]) == 1, p
        assert not torch.equal(after[p + ".running_mean"].cpu(), sd[p + ".running_mean"]), p
        assert not torch.equal(after[p + ".running_var"].cpu(), sd[p + ".running_var"]), p
    torch.save(after, tmp_path / "model.pth")
    route_a = pointstowood_amd.Net(1, C=R.C)
    missing, unexpected = route_a.load_state_dict(torch.load(tmp_path / "model.pth", map_location="cpu"), strict=True)
    assert not missing and not unexpected


def test_the_training_step_gives_the_same_bits_twice():
    _, logits, loss, grads, _ = _first_step()
    _, logits2, loss2, grads2, _ = _train_step()
    assert torch.equal(_bits(logits), _bits(logits2)) and torch.equal(_bits(loss), _bits(loss2))
    for k in grads:
        assert torch.equal(_bits(grads[k]), _bits(grads2[k])), k


def _gpu_step(sd, inp, fused):
    net = _net(sd, fused=fused)
    d = _data(inp)
    with _searches() as found:
        logits = net(d)
    (logits * inp["g"].cuda()).sum().backward()
    geo = [dict(idx=m.seen_idx.cpu(), edge_index=torch.stack([source, target]).cpu()) for m, (target, source) in zip(_sa(net), found)]
    return logits.detach().cpu(), {k: p.grad.cpu() for k, p in net.named_parameters() if ".reflectanceyesno." not in k}, geo


def test_fused_route_is_no_worse_than_the_plain_route_against_float64():
    """fp32, no autocast, the cotangent g of net_train_ref.inputs on the logits, the fixed ascending sample injected; the float64
    composition (tests/net_train_ref.py) is given the indices and edges of the fp32 run (asserted equal to oracle.ops' own).  For the
    logits and for each parameter's gradient whose true value is not zero: relative L2 error of the fused route <= 8 x the
    fused = False route's own error.

    23 gradients are zero by algebra: a bias in front of a training-mode BatchNorm with nothing but a linear map between them (per
    residual block expand.0, both depthwise and both pointwise convolutions, project.0 and the BatchNorm conv.4 in front of project;
    fp1's last BatchNorm and conv1 in front of norm).  Their float64 values are summation noise near 1e-15, so a relative error would
    compare noise with noise: they are found by their float64 norm (below 1e-9 of the median gradient norm), left out of the ratio
    and held to an absolute bound instead - a sum of at most N = 800 fp32 terms that cancel exactly errs by at most N EPS of the
    terms' magnitude, and no term of a gradient sum exceeds the largest gradient norm G of the net: |g| <= N EPS G, four orders of
    magnitude below what a gradient that is wrongly not zero would be.  The depthwise biases' are exactly 0 in the fused route.

    THE CAP IS WIDE HERE, wider than the issue hoped for: it asks for a seed at which the plain fp32 composition stays near fp32
    rounding noise against float64, and there is none.  Seed 4, chosen on the CPU among 0 .. 11 as the one where the plain
    composition (tests/net_train_ref.py in float32) stays closest: logits 2.0e-4, gradients 1.3e-2 at the median and 1.9e-2 at worst
    among the 117 tensors whose true gradient is not zero; other seeds, and freshly initialised weights, give 2e-2 to 5e-1.  So the
    8 x rule lets the fused route be about 15 % off per tensor, and what this test can show is that it is no further from float64
    than the plain route is.  Where the floor comes from: the forward difference grows by a factor of 2 to 5 per residual block and
    level through the chain of training-mode BatchNorms on 25 to 400 rows (4e-8 behind the stem, 3e-4 at the head), smoothly and in
    every seed; and an activation error of 2e-4 puts about 2e-4 of the ReLU pre-activations on the other side of zero, each flipped
    mask an error of order 1 in its element of the gradient: sqrt(2e-4) = 1.4e-2 relative L2, which is the gradients' median.  A
    maximum's winner switching would show as an outlier among the seeds, which seed 4 is not.  Observed on an MI355X: logits fused
    1.1e-4, plain 1.5e-4; gradients 1.9e-2 and 1.9e-2 at the median; the worst fused / plain ratio of a tensor 2.7."""
    import statistics
    inp, sd = R.inputs(SEED), R.state(SEED)
    lf, gf, geo = _gpu_step(sd, inp, True)
    lp, gp, geo_p = _gpu_step(sd, inp, False)
    for a, b, c in zip(geo, geo_p, R.geometry(inp)):
        for k in ("idx", "edge_index"):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    l64, g64 = R.step(sd, inp, geo, torch.float64)
    assert set(g64) == set(gf) == set(gp)
    norms = {k: float(v.norm()) for k, v in g64.items()}
    zero = {k for k, n in norms.items() if n < 1e-9 * statistics.median(norms.values())}
    assert len(zero) == 23 and all(k.endswith(".bias") for k in zero), sorted(zero)
    assert {k for k in g64 if k.endswith(("depthwise_conv.bias", "expand.0.bias", "project.0.bias", "conv.4.bias"))} | {"conv1.bias"} <= zero
    bound = inp["pos"].shape[0] * 2.0 ** -23 * max(norms.values())
    for k in sorted(zero):
        nf, np_ = float(gf[k].norm()), float(gp[k].norm())
        print(f"NET_TRAIN_ZERO {k} fused {nf:.3e} plain {np_:.3e} bound {bound:.3e}")
        assert nf <= bound and np_ <= bound, (k, nf, np_, bound)
        if k.endswith("depthwise_conv.bias"):
            assert bool((gf[k] == 0).all()), k
    rows = [("logits", R.rel_l2(lf, l64), R.rel_l2(lp, l64))] + [(k, R.rel_l2(gf[k], g64[k]), R.rel_l2(gp[k], g64[k])) for k in g64 if k not in zero]
    for k, ef, ep in rows:
        print(f"NET_TRAIN_ERR {k} fused {ef:.3e} plain {ep:.3e}")
    bad = [(k, ef, ep) for k, ef, ep in rows if not ef <= 8 * ep]
    assert len(rows) == 118 and not bad, bad


def _plain_forward(net, d):
    """The reference's forward (model.py:226-245) over torch.nn modules and the plain ops callables."""
    from pointstowood_amd import ops as H
    x = net.stem_mlp(d.pos[:, :3])
    pos, batch, refl, sf = d.pos, d.batch, d.reflectance, d.sf
    levels = [(x, pos, batch)]
    for sa in _sa(net):
        pos = torch.cat([pos[:, :3], refl.unsqueeze(-1)], dim=-1)
        if torch.sum(refl) != 0:
            pos[:, 3] *= sa.reflectanceyesno(refl.unsqueeze(-1), batch).squeeze(-1)
        if net.training:
            idx = sa.random_sample(pos.shape[0]).to(pos.device)
        else:
            idx = H.consecutive_cluster(H.voxel_grid(pos[:, :3], sa.resolution, batch))[1]
        if sa.resolution == 0.04:
            row, col = H.radius(pos[:, :3], pos[idx, :3], sa.resolution * 2, batch, batch[idx], max_num_neighbors=sa.k)
        else:
            row, col = H.knn(x=pos[:, :3], y=pos[idx, :3], k=sa.k, batch_x=batch, batch_y=batch[idx])
        pos[:, :3] = pos[:, :3] / sf[batch].unsqueeze(-1)
        pos_j, pos_i = pos[col], pos[idx][row]
        msg = torch.zeros((pos_j.size(0), pos_j.size(1)), device=pos_j.device)
        rel = pos_j[:, :3] - pos_i[:, :3]
        dmax, _ = H.scatter_max(torch.norm(rel, dim=1, keepdim=True), row, dim=0, dim_size=idx.numel())
        msg[:, :3] = rel / (dmax[row] + 1e-8)
        msg[:, 3] = pos_j[:, 3]
        x = H.scatter_max(sa.conv.local_nn(torch.cat([x[col], msg], dim=1)), row, dim=0, dim_size=idx.numel())[0]
        pos[:, :3] = pos[:, :3] * sf[batch].unsqueeze(-1)
        x = sa.residual_block._forward_plain(x)
        pos, batch, refl = pos[idx, :3], batch[idx], refl[idx]
        levels.append((x, pos, batch))
    x = H.global_max_pool(net.sa4_module.NN(torch.cat([x, pos], dim=1)), batch)
    cur = (x, pos.new_zeros((x.size(0), 3)), torch.arange(x.size(0), device=batch.device))
    for fp, skip in zip((net.fp4_module, net.fp3_module, net.fp2_module, net.fp1_module), reversed(levels)):
        h = H.knn_interpolate(cur[0], cur[1], skip[1], cur[2], skip[2], k=fp.k)
        cur = (fp.NN(torch.cat([h, skip[0]], dim=1)), skip[1], skip[2])
    x = F.relu(net.norm(F.linear(cur[0], net.conv1.weight[:, :, 0], net.conv1.bias)))
    return torch.squeeze(F.linear(x, net.conv2.weight[:, :, 0], net.conv2.bias).t()).to(torch.float)


@pytest.mark.parametrize("train", [False, True])
def test_unfused_instance_runs_only_the_plain_statements(monkeypatch, train):
    """net.fused = False on an instance reaches every module with the switch; eval and training forward then call none of the fused
    operators (they are replaced by a function that raises) and equal the plain composition over the same modules bit for bit, the
    running statistics included."""
    from pointstowood_amd import ops as H
    inp, sd = R.inputs(SEED), R.state(SEED)
    d = _data(inp)
    net = _net(sd, fused=False, train=train)
    assert [m.fused for m in net.modules() if hasattr(type(m), "fused")] == [False] * 9
    twin = copy.deepcopy(net)

    def boom(*a, **k):
        raise AssertionError("a fused operator ran with fused = False")
    for name in FUSED_OPS:
        monkeypatch.setattr(H, name, boom)
    monkeypatch.setattr(H.PointNetConv, "forward", boom)
    monkeypatch.setattr(H.InvertedResidualBlock, "forward", boom)
    with torch.no_grad():
        got, want = net(d), _plain_forward(twin, d)
    assert got.shape == (800,) and torch.equal(got, want)
    a, b = net.state_dict(), twin.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(int(v) == int(train) for k, v in a.items() if k.endswith("num_batches_tracked"))
