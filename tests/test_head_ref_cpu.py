"""tests/head_ref.py on the CPU: head64 (the closed forms of ops.bn_relu_rowdot's forward and backward) against PyTorch's float64
autograd of the literal composition, and the kernel references against head64 on statistics rounded to fp32.  Also what the package
must offer for the head: the entry points in the ABI table and the operator."""
import os

import pytest
import torch

from tests import head_ref as R


@pytest.mark.parametrize("M,C", [(2, 1), (33, 5), (257, 67)])
def test_head64_equals_float64_autograd(M, C):
    c = R.case(M, C)
    leaves = {k: c[k].double().requires_grad_() for k in ("z", "gamma", "beta", "w", "bias")}
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    out = R.composition(leaves["z"], leaves["gamma"], leaves["beta"], leaves["w"], leaves["bias"], rm, rv)
    out.backward(c["g"].double())
    r = R.head64(c["z"], c["gamma"], c["beta"], c["w"], c["bias"], c["g"])
    torch.testing.assert_close(r["logit"], out.detach(), rtol=1e-12, atol=1e-12)
    for k, leaf in (("dz", "z"), ("dgamma", "gamma"), ("dbeta", "beta"), ("dw", "w"), ("dbias", "bias")):
        torch.testing.assert_close(r[k], leaves[leaf].grad, rtol=1e-9, atol=1e-9, msg=lambda m, k=k: f"{k}: {m}")
    torch.testing.assert_close((1 - R.MOMENTUM) * c["rm"].double() + R.MOMENTUM * r["mean"], rm, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close((1 - R.MOMENTUM) * c["rv"].double() + R.MOMENTUM * r["var"] * M / (M - 1), rv, rtol=1e-12, atol=1e-12)


def test_kernel_references_agree_with_head64_and_caps_are_small():
    """On the float64 statistics rounded to fp32 the kernel references are head64 up to those roundings, and a cap is a few dozen ulp of
    its tensor's scale, not a licence."""
    M, C = 257, 67
    c = R.case(M, C)
    r = R.head64(c["z"], c["gamma"], c["beta"], c["w"], c["bias"], c["g"])
    mean32, invstd32 = r["mean"].float(), r["invstd"].float()
    ref, caps = R.forward_reference(c, mean32, invstd32)
    bref, bcaps = R.backward_reference(c, mean32, invstd32)
    assert float((ref["logit"] - r["logit"]).abs().max()) < 1e-4
    for k in ("dgamma", "dbeta", "dw", "dbias"):
        assert float((bref[k] - r[k]).abs().max()) < 1e-3 * max(1.0, float(r[k].abs().max())), k
    torch.testing.assert_close(bref["dw"], r["dw"], rtol=1e-4, atol=1e-4)
    assert float(caps["logit"].max()) < 1e-3 * float(ref["logit"].abs().max())
    assert float(bcaps["dw"].max()) < 1e-5 and float(bcaps["dbias"].max()) < 1e-5
    assert float((caps["logit"] > 0).float().mean()) == 1.0


def test_the_package_offers_the_head():
    from pointstowood_amd import _lib, ops
    for name in ("p2w_bn_relu_rowdot_ws_size", "p2w_bn_relu_rowdot", "p2w_bn_relu_rowdot_bwd"):
        assert name in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p2w.h")).read()
    assert "p2w_bn_relu_rowdot_bwd(" in header and "p2w_bn_relu_rowdot_ws_size(" in header
    assert callable(ops.bn_relu_rowdot)
    import pointstowood_amd.train as T
    assert T.Net.fused is True
