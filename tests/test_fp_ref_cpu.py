"""The two identities behind the fused training route of ops.FPModule, in float64 on the CPU (tests/fp_ref.py), and the condition on
the inputs that tests/test_gpu_fp.py relies on."""
import pytest
import torch
import torch.nn.functional as F

from tests import fp_ref as R


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("name", list(R.MODULE_CASES))
def test_hoisted_layer0_equals_the_plain_layer0(name):
    """relu(interp(xc Wc^T) + x_skip Ws^T + b) against relu(Linear0(cat[interp(xc), x_skip])) over oracle/ops.py's knn_interpolate under
    float64 autograd: the output and the gradients to xc, x_skip, W0 and b0.  'ragged' has a batch with two coarse points under k = 3
    (rows of two neighbours), 'fp4' batches of one coarse point (rows of one neighbour).  The identity is exact; what is left is float64
    rounding of sums of at most a few hundred O(1) terms, some 1e-14 relative - held to 1e-12."""
    c = R.module_case(name)
    deg = torch.bincount(c["batch"])[c["batch_skip"]].clamp_max(c["k"])
    assert int(deg.min()) == (1 if name == "fp4" else 2) and int(torch.bincount(c["batch"]).min()) in (1, 2)
    got = {}
    for hoisted in (False, True):
        x, xs = (c[k].double().requires_grad_() for k in ("x", "x_skip"))
        W0, b0 = (c["sd"][k].double().requires_grad_() for k in ("NN.0.0.weight", "NN.0.0.bias"))
        out = torch.relu(R.layer0(c, x, xs, W0, b0, hoisted))
        (out * torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)).sum().backward()
        got[hoisted] = dict(out=out.detach(), x=x.grad, x_skip=xs.grad, W0=W0.grad, b0=b0.grad)
    for k in got[True]:
        assert float(got[False][k].norm()) > 0
        assert _rel(got[True][k], got[False][k]) <= 1e-12, k


def test_one_neighbour_rows_copy_their_coarse_row():
    """Rows with a single neighbour (fp4: the weights sum to 1 with one term) interpolate to that coarse row."""
    c = R.module_case("fp4")
    t = R.interp(c, c["x"].double())
    assert _rel(t, c["x"].double()[c["batch_skip"]]) <= 1e-15


def test_relu_bn_closed_form_equals_autograd():
    """dz, dgamma, dbeta of fp_ref.relu_bn_backward against float64 autograd of F.batch_norm(relu(z), training=True); column 0 is all
    z <= 0 (zero variance: dz = 0 there, dgamma = 0), column 1 has gamma < 0, column 2 gamma = 0.  Both sides are float64 evaluations of
    the same closed form; they differ by rounding amplified by invstd <= 1 / sqrt(eps) = 316 in the zero-variance column - 1e-10."""
    g = torch.Generator().manual_seed(5)
    M, C = 57, 7
    z = torch.randn(M, C, generator=g, dtype=torch.float64)
    z[:, 0] = -z[:, 0].abs()
    z[3, 0] = 0.0
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gamma[1], gamma[2] = -0.7, 0.0
    beta, gout = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(M, C, generator=g, dtype=torch.float64)
    zz, gg, bb = z.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    out = F.batch_norm(torch.relu(zz), None, None, gg, bb, True, 0.0, R.BN_EPS)
    (out * gout).sum().backward()
    dz, dgamma, dbeta = R.relu_bn_backward(z, gamma, gout)
    assert bool((dz[:, 0] == 0).all()) and bool((zz.grad[:, 0] == 0).all()) and bool((dz[:, 2] == 0).all())
    for a, b in ((dz, zz.grad), (dgamma, gg.grad), (dbeta, bb.grad)):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", list(R.MODULE_CASES))
def test_module_cases_keep_every_preactivation_away_from_zero(name):
    """Every float64 pre-activation of both layers is further from 0 than MARGIN = 1e-4 of its tensor's RMS (the seeds are chosen for
    it): fp32 routes whose pre-activations agree to some 1e-6 of the RMS cannot disagree on a ReLU mask.  The hoisted form keeps it."""
    c = R.module_case(name)
    for hoisted in (False, True):
        m = R.margins(R.train_step(c, hoisted=hoisted)["pre"])
        print(f"FP_MARGIN {name} hoisted={hoisted} {m}")
        assert len(m) == 2 and min(m) > R.MARGIN


def test_state_keys_are_the_reference_mlp():
    assert [k for k, _ in R.state_keys([96, 80, 64])] == [
        "NN.0.0.weight", "NN.0.0.bias", "NN.1.0.weight", "NN.1.0.bias", "NN.1.2.weight", "NN.1.2.bias", "NN.1.2.running_mean",
        "NN.1.2.running_var", "NN.1.2.num_batches_tracked"]
