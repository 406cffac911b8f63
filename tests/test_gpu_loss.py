"""The fused Poly-1 focal loss (pointstowood_amd.loss over p2w_poly1_focal, csrc/p2w_loss.hip) on the GPU: against the values recorded
from the reference's class (tests/golden/loss), against tests/loss_ref.py at the sizes where the chunking and the tree can go wrong,
run-to-run bits, the autograd wiring, and ``EpochScores`` against ``evaluate.confusion`` + ``binary_metrics``.

The error bound of every comparison with a float64 value: a finite element may deviate by at most 8 x the largest |float32 - float64|
of the reference's own class on the CPU for that configuration (tests/golden/loss/noise.json; the factor of
tests/test_gpu_ops_backward.py: another expf / log1pf / powf and another operation order within a few ulp).  A sum over n elements
gets n times that, a mean the same bound as one element, both plus one float32 rounding of the value (the kernel adds in float64).
Nothing is masked out: the NaN logit's loss and gradient are exactly 0, the gradient beyond +-10 and at +-inf is exactly 0, and the
loss at +-inf has the bits of the kernel's own loss at +-10 with the same label (and is within the bound of the recorded value)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss")
CASES = [(c, k) for c in R.CONFIGS for k in R.LABEL_KINDS]
CHUNK = 4096
SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, CHUNK * 257 + 3]
# The trainer's configuration at every size.  The per-element weights (the kernel's third load stream) at every size but the largest:
# with eps = 1e-4 the sigmoid's clamp bound lies inside the logit range, at |z| = 9.21, where the gradient jumps by about 1e-4 as the
# clamp switches; a sigmoid within one float32 ulp of the bound may fall on the other side than in float64 (for the reference's own
# float32 run as much as for the kernel), and among a million draws of randn * 4 about eight come that close, among 8193 none is
# expected.  With the trainer's eps = 1e-6 the bound lies beyond the logit clamp and no comparison depends on a rounding.
SIZE_CASES = [(n, "trainer", "binary") for n in SIZES] + [(n, "g05_weight_n", "soft") for n in SIZES[:-1]]
F32 = 2.0 ** -24          # one rounding to float32, relative
_cache = {}


@pytest.fixture(scope="module")
def PL():
    from pointstowood_amd import loss
    return loss


def _noise(config, kind):
    if "noise" not in _cache:
        _cache["noise"] = json.load(open(os.path.join(GOLDEN, "noise.json")))["cases"]
    return _cache["noise"][f"{config}__{kind}"]


def _fixture(config, kind):
    if "inputs" not in _cache:
        _cache["inputs"] = dict(np.load(os.path.join(GOLDEN, "inputs.npz")))
    key = ("case", config, kind)
    if key not in _cache:
        _cache[key] = dict(np.load(os.path.join(GOLDEN, f"{config}__{kind}.npz")))
    return R.case_tensors(_cache["inputs"], config, kind) + (_cache[key],)


def _sized(n, config, kind):
    """(logits, labels, weight, kwargs, loss64, dloss64) of the fixture's recipe at n elements, seed 1000 + n: computed once."""
    key = ("sized", n, config, kind)
    if key not in _cache:
        logits, labels, weight, kwargs = R.case_tensors(R.make_inputs(n, seed=1000 + n), config, kind)
        _cache[key] = (logits, labels, weight, kwargs) + R.reference(logits, labels, weight, **kwargs)
    return _cache[key]


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _module(PL, kwargs, weight, reduction):
    return PL.Poly1FocalLoss(**dict(kwargs, reduction=reduction, weight=_dev(weight)))


def _run(PL, logits, labels, weight, kwargs, reduction, scale=None):
    """(value, gradient of value.sum() [times scale]) as float64 numpy, through the module."""
    x = _dev(logits).requires_grad_()
    value, gamma = _module(PL, kwargs, weight, reduction)(x, _dev(labels))
    assert gamma == kwargs["gamma"] and value.dtype == torch.float32 and value.grad_fn is not None
    (value.sum() if scale is None else scale * value.sum()).backward()
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    return value.detach().cpu().double().numpy(), x.grad.cpu().double().numpy()


def _report(what, err, bound):
    ratio = float(np.max(err / bound)) if np.size(err) else 0.0
    print(f"{what}: largest error / bound = {ratio:.4f}  (bound = 8 x reference noise; x 8 for the multiple of the noise itself)")
    return ratio


@pytest.mark.parametrize("config,kind", CASES)
def test_fixture_case(PL, config, kind):
    logits, labels, weight, kwargs, g = _fixture(config, kind)
    noise = _noise(config, kind)
    n = len(logits)
    loss, grad = _run(PL, logits, labels, weight, kwargs, "none")
    assert loss.shape == (n,) and not np.isnan(loss).any() and not np.isnan(grad).any()
    r1 = _report(f"{config}/{kind} loss", np.abs(loss - g["loss64"]), 8 * noise["loss"])
    r2 = _report(f"{config}/{kind} grad", np.abs(grad - g["grad64"]), 8 * noise["grad"])
    assert r1 <= 1 and r2 <= 1
    # the rows that are not finite, and the rows beyond +-10
    assert loss[10] == 0 and grad[10] == 0 and g["loss64"][10] == 0
    beyond = ~((logits >= -10) & (logits <= 10))
    assert beyond[:17].sum() == 9 and (grad[beyond] == 0).all() and grad[0] != 0 and grad[1] != 0
    inf = [11, 12]
    w_inf = weight[inf] if weight is not None and len(weight) > 1 else weight
    at10, _ = _run(PL, np.asarray([10.0, -10.0], dtype=np.float32), labels[inf], w_inf, kwargs, "none")
    assert np.array_equal(loss[inf], at10) and np.isfinite(loss[inf]).all()
    print(f"{config}/{kind} +-inf rows equal the reference's float32 bits: {np.array_equal(loss[inf], g['loss32'][inf].astype(np.float64))}")
    # the configuration's own reduction
    red = kwargs["reduction"]
    if red in ("mean", "sum"):
        value, rgrad = _run(PL, logits, labels, weight, kwargs, red)
        per = 1 if red == "sum" else n
        want = float(g["reduced64"])
        bound = 8 * noise["loss"] * (n / per) + F32 * abs(want)
        r3 = _report(f"{config}/{kind} {red}", abs(float(value) - want), bound)
        r4 = _report(f"{config}/{kind} {red} grad", np.abs(rgrad - g["rgrad64"]), 8 * noise["grad"] / per + 2 * F32 * np.abs(g["rgrad64"]))
        assert value.shape == () and r3 <= 1 and r4 <= 1
        assert (rgrad[beyond] == 0).all()


@pytest.mark.parametrize("n,config,kind", SIZE_CASES)
def test_sizes(PL, n, config, kind):
    """Every chunk boundary: per-element loss and gradient, the float64 sum through the ABI (every element in it exactly once: it
    equals the float64 sum of the kernel's own float32 losses up to the rounding of that sum) and the reduced values."""
    logits, labels, weight, kwargs, loss64, dloss64 = _sized(n, config, kind)
    noise = _noise(config, kind)
    loss, grad = _run(PL, logits, labels, weight, kwargs, "none")
    assert loss.shape == (n,) and grad.shape == (n,)
    assert _report(f"n={n} {config} loss", np.abs(loss - loss64), 8 * noise["loss"]) <= 1
    assert _report(f"n={n} {config} grad", np.abs(grad - dloss64), 8 * noise["grad"]) <= 1
    scalars = PL._scalars(kwargs["epsilon"], kwargs["gamma"], kwargs["alpha"], kwargs["label_smoothing"], kwargs["eps"])
    x, y, w = _dev(logits), _dev(labels), _dev(weight)
    _, none, total = PL._launch(x, y, w, scalars, False, False, True)
    assert none is None and total.dtype == torch.float64
    total = float(total)
    own = float(loss.sum())
    assert abs(total - own) <= 1e-12 * own and abs(total - loss64.sum()) <= 8 * noise["loss"] * n
    with torch.no_grad():
        s, _ = _module(PL, kwargs, weight, "sum")(x, y)
        m, _ = _module(PL, kwargs, weight, "mean")(x, y)
    assert s.shape == () and m.shape == () and s.dtype == torch.float32 and m.dtype == torch.float32
    assert float(s) == float(np.float32(total))
    if n == 0:
        assert total == 0 and np.isnan(float(m))
    else:
        assert float(m) == float(np.float32(total / n))
        assert abs(float(m) - loss64.mean()) <= 8 * noise["loss"] + F32 * loss64.mean()


def test_a_view_off_the_16_byte_boundary(PL):
    """``x[1:]`` starts 4 bytes into its storage: same bits as the aligned copy, gradient in the view's shape."""
    logits, labels, weight, kwargs, _, _ = _sized(CHUNK + 1, "g05_weight_n", "soft")
    n = len(logits)
    pad = lambda a: torch.cat([torch.zeros(1), torch.from_numpy(a)]).cuda()        # noqa: E731
    bx, by, bw = pad(logits), pad(labels), pad(weight)
    base = bx.clone().requires_grad_()
    x = base[1:]
    assert x.data_ptr() % 16 == 4 and by[1:].data_ptr() % 16 == 4
    m = PL.Poly1FocalLoss(**dict(kwargs, reduction="none", weight=bw[1:]))
    loss, _ = m(x, by[1:])
    loss.sum().backward()
    want, wgrad = _run(PL, logits, labels, weight, kwargs, "none")
    assert np.array_equal(loss.detach().cpu().double().numpy(), want)
    assert base.grad.shape == (n + 1,) and base.grad[0] == 0 and np.array_equal(base.grad[1:].cpu().double().numpy(), wgrad)


def test_same_bits_on_every_run(PL):
    logits, labels, weight, kwargs, _, _ = _sized(CHUNK * 257 + 3, "g05_weight_n", "soft")
    y = _dev(labels)
    runs = []
    for _ in range(2):
        x = _dev(logits).requires_grad_()
        loss, _ = _module(PL, kwargs, weight, "none")(x, y)
        total, _ = _module(PL, kwargs, weight, "sum")(x, y)
        mean, _ = _module(PL, kwargs, weight, "mean")(x, y)
        mean.backward()
        runs.append((loss.detach(), total.detach(), mean.detach(), x.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_upstream_factor(PL):
    """``GradScaler``'s initial scale: (512 * loss).backward() gives 512 times the gradient of the mean (a power of two: exactly)."""
    logits, labels, weight, kwargs, g = _fixture("trainer", "binary")
    noise = _noise("trainer", "binary")
    _, plain = _run(PL, logits, labels, weight, kwargs, "mean")
    _, scaled = _run(PL, logits, labels, weight, kwargs, "mean", scale=512.0)
    assert np.array_equal(scaled, 512 * plain)
    n = len(logits)
    assert _report("512 x mean grad", np.abs(scaled - 512 * g["rgrad64"]), 512 * (8 * noise["grad"] / n + 2 * F32 * np.abs(g["rgrad64"]))) <= 1
    # and an elementwise upstream gradient for "none"
    up = torch.linspace(-2, 2, n).cuda()
    x = _dev(logits).requires_grad_()
    loss, _ = _module(PL, kwargs, weight, "none")(x, _dev(labels))
    loss.backward(up)
    _, ones = _run(PL, logits, labels, weight, kwargs, "none")
    assert torch.equal(x.grad.cpu(), (up.cpu() * torch.from_numpy(ones).float()))


def test_half_logits_under_autocast(PL):
    logits, labels, weight, kwargs, _ = _fixture("trainer", "binary")
    for dtype in (torch.float16, torch.bfloat16):
        h = _dev(logits).to(dtype)
        x = h.clone().requires_grad_()
        with torch.autocast("cuda", dtype=dtype):
            loss, _ = _module(PL, kwargs, weight, "mean")(x, _dev(labels).to(torch.int64))
            each, _ = _module(PL, kwargs, weight, "none")(x, _dev(labels))
        loss.backward()
        assert loss.dtype == torch.float32 and each.dtype == torch.float32 and x.grad.dtype == dtype
        want, wgrad = _run(PL, h.float().cpu().numpy(), labels, weight, kwargs, "mean")
        assert float(loss) == float(want)
        assert torch.equal(x.grad.cpu(), torch.from_numpy(wgrad).float().to(dtype))


def test_no_grad_allocates_no_gradient_buffer(PL, monkeypatch):
    logits, labels, weight, kwargs, _, _ = _sized(CHUNK * 257 + 3, "trainer", "binary")
    n = len(logits)
    x, y = _dev(logits), _dev(labels)
    xr = x.clone().requires_grad_()
    tracked, _ = _module(PL, kwargs, weight, "none")(xr, y)
    calls = []
    real = PL._launch

    def spy(x, y, w, scalars, want_loss, want_grad, want_sum):
        out = real(x, y, w, scalars, want_loss, want_grad, want_sum)
        calls.append((want_loss, want_grad, want_sum, out[1]))
        return out
    monkeypatch.setattr(PL, "_launch", spy)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - before

    def under_no_grad():
        with torch.no_grad():
            return _module(PL, kwargs, weight, "none")(xr, y)[0]
    free, used = peak(under_no_grad)
    assert 4 * n <= used < 1.5 * 4 * n                                         # the loss, and no second array of its size
    detached, used = peak(lambda: _module(PL, kwargs, weight, "none")(x, y)[0])          # logits that track no gradient
    assert 4 * n <= used < 1.5 * 4 * n
    assert calls == [(True, False, False, None), (True, False, False, None)]
    assert free.grad_fn is None and torch.equal(free, tracked.detach()) and torch.equal(detached, free)
    del free, detached

    def mean_under_no_grad():
        with torch.no_grad():
            return _module(PL, kwargs, weight, "mean")(xr, y)[0]
    mean, used = peak(mean_under_no_grad)
    assert used < 4 * n // 8 and calls[-1] == (False, False, True, None)       # the chunk sums only
    m2, _ = _module(PL, kwargs, weight, "mean")(xr, y)
    assert calls[-1][:3] == (False, True, True) and calls[-1][3] is not None and torch.equal(mean, m2.detach())


def test_linear_in_front_of_the_loss(PL):
    """A Linear(8, 1) in front: features and weights are small dyadic rationals, so the float32 logits are exact and equal the
    float64 ones; what remains is the kernel's per-element gradient error e <= 8 x noise, which reaches parameter j as at most
    mean_i |f_ij| x e (the mean reduction's 1 / n), plus the float32 sum of n terms in the backward matmul: at most
    log2(n) roundings of a pairwise sum, n for a sequential one - the bound takes the geometric middle, sqrt(n) x 2^-24 x mean |terms|."""
    _, labels, _, kwargs, _ = _fixture("trainer", "binary")
    noise = _noise("trainer", "binary")
    n = len(labels)
    g = torch.Generator().manual_seed(5)
    feats = torch.randint(-64, 65, (n, 8), generator=g).float() / 32
    weight = torch.randint(-16, 17, (8, ), generator=g).float() / 16
    bias = torch.tensor([0.25])
    lin = torch.nn.Linear(8, 1)
    with torch.no_grad():
        lin.weight.copy_(weight[None])
        lin.bias.copy_(bias)
    lin64 = torch.nn.Linear(8, 1).double()
    lin64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    z64 = lin64(feats.double())
    R.composite(z64.squeeze(1), torch.from_numpy(labels).double(), **kwargs).backward()
    lin = lin.cuda()
    z = lin(feats.cuda())
    assert z.shape == (n, 1) and torch.equal(z.detach().cpu().double(), z64.detach())          # exact logits
    loss, _ = _module(PL, kwargs, None, "mean")(z, _dev(labels))
    loss.backward()
    d = R.reference(z64.detach().numpy().reshape(-1), labels, None, **kwargs)[1]
    terms = np.abs(d[:, None] * feats.numpy()).mean(axis=0)
    bound_w = 8 * noise["grad"] * feats.abs().mean(dim=0).numpy() + np.sqrt(n) * F32 * terms
    bound_b = 8 * noise["grad"] + np.sqrt(n) * F32 * np.abs(d).mean()
    ew = np.abs(lin.weight.grad.cpu().double().numpy()[0] - lin64.weight.grad.numpy()[0])
    eb = np.abs(lin.bias.grad.cpu().double().numpy() - lin64.bias.grad.numpy())
    assert _report("Linear weight grad", ew, bound_w) <= 1 and _report("Linear bias grad", eb, bound_b) <= 1


def test_gradient_targets_and_shapes(PL):
    x = torch.randn(6, 5, device="cuda", requires_grad=True)
    y = (torch.rand(6, 5, device="cuda") < 0.3).float()
    loss, gamma = PL.Poly1FocalLoss(reduction="whatever")(x, y, label_weights=torch.ones(3))      # any other string: "none"
    assert loss.shape == (6, 5) and gamma == 2.0
    loss.sum().backward()
    assert x.grad.shape == (6, 5)
    with pytest.raises(ValueError, match="logits only"):
        PL.Poly1FocalLoss()(x, y.clone().requires_grad_())
    with torch.no_grad():
        PL.Poly1FocalLoss()(x, y.clone().requires_grad_())                       # nothing is tracked: nothing can be missing


def test_epoch_scores(PL):
    """Three batches of different sizes, one with all-negative truth, through a buffer that has to double: the figures equal
    ``binary_metrics`` of ``evaluate.confusion``'s own matrices, summed in batch order and divided by the count, bit for bit."""
    from pointstowood_amd import evaluate as EV
    g = torch.Generator().manual_seed(9)
    sizes, losses = [5000, 1, 777], [0.625, 0.1, 0.3]
    scores = PL.EpochScores(threshold=0.5, capacity=2)
    rows = []
    for i, (n, l) in enumerate(zip(sizes, losses)):
        logits = (torch.randn(n, 1, generator=g) * 3).cuda()
        truth = torch.zeros(n) if i == 2 else (torch.rand(n, generator=g) < 0.4).float()
        truth = truth.cuda()
        loss = torch.tensor(l, device="cuda", requires_grad=True) * 1.0
        scores.add(logits, truth, loss)
        counts, _, invalid = EV.confusion(truth, (torch.sigmoid(logits.reshape(-1)) >= 0.5), classes=2)
        assert int(invalid) == 0
        rows.append(counts[0].cpu().numpy())
    assert len(scores) == 3 and scores._capacity == 4
    out = scores.result()
    assert np.array_equal(out["matrices"], np.stack(rows)) and out["matrices"].dtype == np.int64
    assert rows[2][1].sum() == 0 and rows[1].sum() == 1
    assert np.array_equal(out["losses"], np.asarray(losses, dtype=np.float32))
    for k in ("balanced_accuracy", "f1", "precision", "recall"):
        total = 0.0
        for m in rows:
            total += EV.binary_metrics(m)[k]
        assert out[k] == total / 3, k
    total = 0.0
    for l in np.asarray(losses, dtype=np.float32):
        total += float(l)
    assert out["loss"] == total / 3
    empty = PL.EpochScores().result()
    assert np.isnan(empty["loss"]) and empty["matrices"].shape == (0, 2, 2)
    bad = PL.EpochScores()
    bad.add(torch.zeros(4, device="cuda"), torch.tensor([0.0, 1.0, 2.0, 0.5], device="cuda"))
    with pytest.raises(ValueError, match="batch 0"):
        bad.result()
