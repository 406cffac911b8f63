"""The float64 reference of p2w_relu_bn_max / p2w_relu_bn_max_bwd (tests/bn_max_ref.py) against PyTorch itself on the CPU: the
extremum trick (BN of the segment maximum, of the minimum where gamma < 0), the closed form of the backward and the running
statistics are pinned here, where no kernel is involved."""
import torch

from tests import bn_max_ref as R


def _bn(C, gamma, beta, rm, rv):
    bn = torch.nn.BatchNorm1d(C, eps=R.BN_EPS, momentum=R.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    return bn.train()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_forward_is_the_segment_max_of_batch_norm_of_relu():
    """On the kernels' own case at C2 = 16 (gamma > 0, < 0 and = 0, an all-negative and a constant column, an all-tie target, empty
    targets): out equals the segment max of torch.nn.functional.batch_norm(relu(z), training=True) in float64, empty targets 0; the
    running statistics and num_batches_tracked's companion values equal BatchNorm1d's; arg points at a row of its own target that
    holds ext, and no lower row does."""
    c, d = R.targets(), R.columns(16)
    ref, _ = R.forward_reference(d["z"], c["index"], R.M_DST, d["gamma"], d["beta"], d["running_mean"], d["running_var"])
    bn = _bn(16, d["gamma"], d["beta"], d["running_mean"], d["running_var"])
    want = R.composition(d["z"].double(), c["index"], R.M_DST, bn).detach()
    assert _rel(ref["out"], want) <= 1e-12
    assert bool((ref["out"][c["deg"] == 0] == 0).all()) and bool((ref["arg"][c["deg"] == 0] == -1).all())
    assert _rel(ref["running_mean"], bn.running_mean) <= 1e-12 and _rel(ref["running_var"], bn.running_var) <= 1e-12
    y = torch.relu(d["z"].double())
    ptr = c["ptr"].long()
    for t in (1, 2, 5, R.TIE_TARGET, 700):
        rows = y[ptr[t]:ptr[t + 1]]
        for col in range(16):
            a = int(ref["arg"][t, col])
            assert ptr[t] <= a < ptr[t + 1] and y[a, col] == ref["ext"][t, col]
            assert not bool((rows[:a - ptr[t], col] == ref["ext"][t, col]).any())
            want_ext = rows[:, col].min() if d["gamma"][col] < 0 else rows[:, col].max()
            assert ref["ext"][t, col] == want_ext
    assert bool((ref["arg"][R.TIE_TARGET, 4:] == ptr[R.TIE_TARGET]).all())            # all ties: the first row
    assert bool((ref["out"][c["deg"] > 0][:, R.ALL_NEG] == d["beta"].double()[R.ALL_NEG]).all())
    assert float(ref["var"][R.CONST]) <= 1e-15


def test_backward_is_autograd_of_the_composition():
    """dz, dgamma and dbeta of the reference equal float64 autograd of segment max(batch_norm(relu(z))) to 1e-12 relative, with gamma
    of both signs.  The inputs are free of ties among positive values (randn); the ties they do have are ReLU zeros, whose rows have
    z <= 0 and so carry no gradient to z, and whose xhat is the same whichever of them wins: PyTorch's even split and the lowest-row
    rule give the same three gradients there."""
    g = torch.Generator().manual_seed(5)
    M, C = 60, 7
    deg = torch.randint(0, 9, (M,), generator=g)
    deg[3], deg[M - 1] = 40, 0
    index = torch.repeat_interleave(torch.arange(M), deg)
    E = index.numel()
    z = torch.randn(E, C, generator=g).float()
    gamma = torch.tensor([1.3, -0.7, 0.4, -1.1, 2.0, 0.9, -0.2])
    beta, go = torch.randn(C, generator=g), torch.randn(M, C, generator=g)
    rm, rv = torch.zeros(C), torch.ones(C)
    ref, _ = R.forward_reference(z, index, M, gamma, beta, rm, rv)
    (dz, dgamma, dbeta), _ = R.backward_reference(go, z, index, ref["arg"], ref["ext"], ref["mean"], ref["invstd"], gamma)
    bn = _bn(C, gamma, beta, rm, rv)
    zz = z.double().requires_grad_()
    out = R.composition(zz, index, M, bn)
    assert _rel(ref["out"], out.detach()) <= 1e-12
    (out * go.double()).sum().backward()
    assert _rel(dz, zz.grad) <= 1e-12 and _rel(dgamma, bn.weight.grad) <= 1e-12 and _rel(dbeta, bn.bias.grad) <= 1e-12
    assert bool((dz[z <= 0] == 0).all()) and float(dz.abs().max()) > 0


def test_caps_and_ratio():
    """ratio(): a cap of 0 asks for exactness; the case has what its docstring says."""
    c = R.targets()
    assert c["E"] % 2 == 1 and int(c["deg"].max()) == 1500 and bool((c["deg"][-R.TRAILING_EMPTY:] == 0).all())
    assert set(int(x) for x in (0, 1, 32, 33, 100, 1500)) <= set(int(x) for x in c["deg"])
    assert (R.M_DST + R.GROUP - 1) // R.GROUP > 1 and R.M_DST % R.GROUP
    one = torch.ones(3, dtype=torch.float64)
    assert R.ratio(one, one, torch.zeros(3, dtype=torch.float64)) == 0.0
    assert R.ratio(one + 1e-9, one, torch.zeros(3, dtype=torch.float64)) == float("inf")
    for C2 in R.WIDTHS:
        d = R.columns(C2)
        assert bool((d["z"][:, R.ALL_NEG] < 0).all()) and bool((d["z"][:, R.CONST] == d["z"][0, R.CONST]).all())
        assert d["gamma"][R.GAMMA_NEG] < 0 and d["gamma"][R.GAMMA_ZERO] == 0
