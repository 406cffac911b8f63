"""tests/bn_chain_ref.py's float64 algebra (chain64: the forward, the closed forms of the backward, the running statistics) against
PyTorch's float64 autograd of the literal composition (F.batch_norm(training=True), relu, w * x + b) on the CPU, for every stage
pattern of the GPU tests: L = 1, 2, 3, with and without depthwise convolution, ReLU and residual.  The GPU tests rest on it.

Tolerances.  Both sides are float64 (D = 2^-53 per operation) over M rows, so a column sum carries at most M D of its terms.  What a
stage does to an error in its input is multiplication by |a| invstd |gamma| per column - up to 1 / sqrt(eps) = 316 in a planted
zero-variance column, where the two sides' means of M equal numbers may differ in the last bit.  Per column the bar is therefore
    tol[c] = 64 M D prod_s (1 + |a_s| invstd_s |gamma_s|)[c] max(1, max |ref|)
for every [M, C] and [C] tensor (64: the handful of operations per stage and the two sides' different orders).
ddw_b: chain64 returns exact zeros; autograd's value is its own summation noise sum gv.  Every gv is the result of at most 8 float64
roundings on T = |gamma| invstd (|gy| + |dbeta / M| + |xhat dgamma / M|), the means inside it carry M D of their terms (T again), and
the sum of M such terms adds M D sum T: |ddw_b| <= 4 (M + 8) D sum_rows T, with the factor 4 for the unknown order of PyTorch's
batch_norm backward.  The gradient arriving at the stage carries the noise of the stages above it, amplified as above."""
import pytest
import torch

from tests import bn_chain_ref as R

M, C = 517, 6


def _leaf(t):
    return None if t is None else t.double().clone().requires_grad_()


def _autograd(c):
    z, res = _leaf(c["z"]), _leaf(c["res"])
    stages = [dict(a=_leaf(st["a"]), b=_leaf(st["b"]), gamma=_leaf(st["gamma"]), beta=_leaf(st["beta"]), relu=st["relu"],
                   running_mean=st["running_mean"].double().clone(), running_var=st["running_var"].double().clone()) for st in c["stages"]]
    out = R.composition(z, stages, res)
    (out * c["g"].double()).sum().backward()
    return z, res, stages, out.detach()


@pytest.mark.parametrize("name", list(R.PATTERNS))
def test_chain64_equals_float64_autograd(name):
    c = R.case(name, C, M)
    r = R.chain64(c["z"], c["stages"], c["res"], c["g"])
    z, res, stages, out = _autograd(c)
    amp = torch.ones(C, dtype=torch.float64)
    for s, st in enumerate(c["stages"]):
        a = st["a"].double().abs() if st["a"] is not None else 1.0
        amp = amp * (1 + a * r["invstd"][s] * st["gamma"].double().abs())

    def close(got, ref, what):
        tol = 64 * M * R.D * amp * max(1.0, float(ref.abs().max()))
        err = (got - ref).abs()
        worst = float((err / tol).max())
        print(f"BNCHAIN_CPU {name} {what}: worst error / tolerance {worst:.3e}")
        assert worst <= 1.0, (name, what, worst)

    close(r["out"], out, "out")
    close(r["dz"], z.grad, "dz")
    if res is not None:
        close(r["dres"], res.grad, "dres")
    else:
        assert r["dres"] is None
    g_in = amp.clone()
    for s, st in enumerate(stages):
        close(r["dgamma"][s], st["gamma"].grad, f"dgamma{s}")
        close(r["dbeta"][s], st["beta"].grad, f"dbeta{s}")
        close(r["running_mean"][s], st["running_mean"], f"running_mean{s}")
        close(r["running_var"][s], st["running_var"], f"running_var{s}")
        if st["a"] is not None:
            close(r["ddw_w"][s], st["a"].grad, f"ddw_w{s}")
            assert bool((r["ddw_b"][s] == 0).all())
        else:
            assert r["ddw_w"][s] is None and r["ddw_b"][s] is None
    # the depthwise bias: autograd's gradient is summation noise around the exact zero
    full = R.chain64(c["z"], c["stages"], c["res"], c["g"])
    gg = c["g"].double() if c["res"] is None else full["dres"]
    keep = []
    u = c["z"].double()
    for s, st in enumerate(c["stages"]):                                   # the forward once more, for xhat and the masks
        a = st["a"].double() if st["a"] is not None else None
        v = a * u + st["b"].double() if a is not None else u
        xhat = (v - full["mean"][s]) * full["invstd"][s]
        y = xhat * st["gamma"].double() + st["beta"].double()
        keep.append((xhat, y))
        u = torch.relu(y) if st["relu"] else y
    for s in range(len(stages) - 1, -1, -1):
        st, (xhat, y) = c["stages"][s], keep[s]
        gy = torch.where(y > 0, gg, torch.zeros_like(gg)) if st["relu"] else gg
        sc = st["gamma"].double().abs() * full["invstd"][s]
        T = sc * (gy.abs() + (full["dbeta"][s] / M).abs() + (xhat * full["dgamma"][s] / M).abs())
        if st["a"] is not None:
            cap = 4 * (M + 8) * R.D * T.sum(0) * g_in
            got = stages[s]["a"].grad * 0 + stages[s]["b"].grad
            print(f"BNCHAIN_CPU {name} ddw_b{s}: autograd max |value| {float(got.abs().max()):.3e}, worst value / cap {float((got.abs() / cap.clamp_min(1e-300)).max()):.3e}")
            assert bool((got.abs() <= cap).all()), (name, s)
        gg = st["gamma"].double() * full["invstd"][s] * (gy - full["dbeta"][s] / M - xhat * full["dgamma"][s] / M)
        if st["a"] is not None:
            gg = st["a"].double() * gg


def test_case_has_its_planted_columns():
    c = R.case("middle", 16)
    st = c["stages"]
    assert c["z"].shape == (R.M_ROWS, 16) and R.M_ROWS % 2 == 1 and R.M_ROWS % R.ROWS and -(-R.M_ROWS // R.ROWS) > 128
    assert bool((c["z"][:, R.CONST] == c["z"][0, R.CONST]).all())
    assert all(float(s["gamma"][R.GAMMA_NEG]) < 0 and float(s["gamma"][R.GAMMA_ZERO]) == 0 for s in st)
    assert float(st[2]["a"][R.DW_ZERO]) == 0 and float(st[2]["a"][R.DW_NEG]) < 0 and st[0]["a"] is None
    r = R.chain64(c["z"], st)
    assert float(r["var"][1][R.ALL_NEG]) == 0.0 and float(r["mean"][1][R.ALL_NEG]) == 0.0       # all-negative before stage 1's ReLU
    assert set(len(p) for p, _ in R.PATTERNS.values()) == {1, 2, 3}
    assert {(len(p), res) for p, res in R.PATTERNS.values()} >= {(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)}
