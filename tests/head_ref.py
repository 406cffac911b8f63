"""float64 references of p2w_bn_relu_rowdot / p2w_bn_relu_rowdot_bwd (csrc/p2w_head.hip, ops.bn_relu_rowdot), the per-element caps the
GPU tests hold the kernels to, and the case.

    xhat = (z - mean) invstd,   u = relu(xhat gamma + beta),   logit[r] = bias + sum_c w[c] u[r, c]
    gy[r, c] = g[r] w[c] [u[r, c] > 0],   dbeta = sum gy,   dgamma = sum gy xhat,   dw = sum g u   (per column),   dbias = sum g,
    dz = ((gy - dbeta / M) - xhat dgamma / M) gamma invstd

Two references, as in tests/bn_chain_ref.py:

  head64()       everything in float64 with its own statistics - the algebra.  tests/test_head_ref_cpu.py holds it against PyTorch's
                 float64 autograd of F.linear(torch.relu(F.batch_norm(z, ..., training=True)), w, b).
  forward_reference() / backward_reference()
                 what the kernels must give on the fp32 tensors THEY are given.  Everything up to u, and everything from gy down to dz,
                 is the one-stage chain with a ReLU: bn_chain_ref's forward_reference / backward_reference are called for it, with their
                 caps, on the kernel's own rounded mean and invstd (the ReLU mask comes from the fp32 replay of the kernel's operations,
                 which are IEEE one by one).  The gradient that enters the chain is G[r, c] = fl32(g[r] w[c]), what the kernel forms in
                 registers (include/p2w.h) and what the bit-for-bit test feeds p2w_bn_chain_bwd: it is given, e_g = 0.

Caps added here (EPS = 2^-23, D = 2^-53; a sum of n terms in any fixed order gets n ulp of sum |terms|, twice the textbook bound, as in
bn_chain_ref; cap_u = bn_chain_ref's cap of the one-stage output, 2 e):

  logit       = fl32(sum_c fl32(w[c] u[r, c]) + bias) over the kernel's u.  What u carries: sum_c |w[c]| cap_u[r, c].  The C products: EPS / 2
              |w u| each.  The sum of the C products and the bias, C + 1 terms in the fixed order of include/p2w.h (the zeros of lanes
              without a column add nothing): (C + 1) EPS (sum_c |w u| + |bias|).
              cap = sum_c |w| cap_u + (C + 1.5) EPS sum_c |w u| + (C + 1) EPS |bias|.
  dw          = fl32(sum_r g[r] u[r, c]) with the replayed fp32 u, products and sums in fp64: cap EPS |dw| + (M + 1) D sum |g u|.
  dbias       = fl32(sum_r g[r]) in fp64: cap EPS |dbias| + M D sum |g|.
  dz, dgamma, dbeta, mean, invstd, running_*: bn_chain_ref's.

The tests print the worst ratio per tensor; a cap is derived here and never tuned to a kernel's output."""
import torch

from tests import bn_chain_ref as BR
from tests.bn_chain_ref import D, EPS, MOMENTUM, BN_EPS, ratio  # noqa: F401

ZERO_VAR, GAMMA_ZERO, GAMMA_NEG, W_ZERO, NAN_COL = 0, 1, 2, 3, 4          # planted columns (C >= 5; NAN_COL only on request)
_cases = {}


def case(M, C, nan=False):
    """z [M, C], g [M], gamma, beta, w [C], bias [1], running statistics, fp32.  With C >= 5: column ZERO_VAR of z is constant, gamma = 0
    in column GAMMA_ZERO, gamma < 0 in column GAMMA_NEG, w = 0 in column W_ZERO and, with `nan`, one NaN in column NAN_COL of z."""
    key = (M, C, nan)
    if key not in _cases:
        gen = torch.Generator().manual_seed(1000 * M + 7 * C + 1)
        z, g = torch.randn(M, C, generator=gen), torch.randn(M, generator=gen)
        gamma, beta = torch.rand(C, generator=gen) + 0.5, 0.5 * torch.randn(C, generator=gen)
        w, bias = torch.randn(C, generator=gen), torch.randn(1, generator=gen)
        rm, rv = 0.1 * torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
        if C >= 5:
            z[:, ZERO_VAR] = 0.25
            gamma[GAMMA_ZERO], gamma[GAMMA_NEG], w[W_ZERO] = 0.0, -0.8, 0.0
            beta[ZERO_VAR] = 0.3
            if nan:
                z[M // 2, NAN_COL] = float("nan")
        _cases[key] = dict(z=z, g=g, gamma=gamma, beta=beta, w=w, bias=bias, rm=rm, rv=rv)
    return _cases[key]


def stage(c):
    """The case as bn_chain_ref's one-stage chain with a ReLU."""
    return [dict(a=None, b=None, gamma=c["gamma"], beta=c["beta"], running_mean=c["rm"], running_var=c["rv"], relu=True)]


# ------------------------------------------------------------------------------------------------ float64 throughout: the algebra
def head64(z, gamma, beta, w, bias, g=None, eps=BN_EPS):
    """Forward and, with g [M], backward in float64 with its own statistics: a dict of logit, mean, var, invstd and dz, dgamma, dbeta,
    dw, dbias."""
    z, gamma, beta, w, bias = (t.double() for t in (z, gamma, beta, w, bias))
    M = z.shape[0]
    mean = z.sum(0) / M
    var = ((z * z).sum(0) / M - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * invstd
    y = xhat * gamma + beta
    u = torch.relu(y)
    r = dict(mean=mean, var=var, invstd=invstd, logit=bias.reshape(()) + (u * w).sum(1))
    if g is None:
        return r
    g = g.double()
    gy = torch.where(y > 0, g[:, None] * w[None, :], torch.zeros_like(y))
    dbeta, dgamma = gy.sum(0), (gy * xhat).sum(0)
    r.update(dbeta=dbeta, dgamma=dgamma, dw=(g[:, None] * u).sum(0), dbias=g.sum().reshape(1),
             dz=((gy - dbeta / M) - xhat * (dgamma / M)) * gamma * invstd)
    return r


def composition(z, gamma, beta, w, bias, rm, rv):
    """The literal composition in z's dtype under ordinary autograd; [M]."""
    import torch.nn.functional as F
    return F.linear(torch.relu(F.batch_norm(z, rm, rv, gamma, beta, True, MOMENTUM, BN_EPS)), w.reshape(1, -1), bias.reshape(1))[:, 0]


# ------------------------------------------------------------------------------------------------ what the kernels must give
def forward_reference(c, mean32, invstd32):
    """float64 results of p2w_bn_relu_rowdot on the case's fp32 tensors, u on the kernel's own mean32 / invstd32 [C]: (ref, caps), dicts
    of mean, invstd, running_mean, running_var [C] and logit [M] (module docstring)."""
    ref, caps = BR.forward_reference(c["z"], stage(c), None, mean32[None], invstd32[None])
    u, cap_u = ref.pop("out"), caps.pop("out")
    ref, caps = {k: v[0] for k, v in ref.items()}, {k: v[0] for k, v in caps.items()}
    w, bias, C = c["w"].double(), c["bias"].double().reshape(()), c["z"].shape[1]
    wu = (u * w).abs().sum(1)
    ref["logit"] = (u * w).sum(1) + bias
    caps["logit"] = (cap_u * w.abs()).sum(1) + (C + 1.5) * EPS * wu + (C + 1) * EPS * bias.abs()
    return ref, caps


def materialised_gradient(c):
    """G[r, c] = fl32(g[r] w[c]): the gradient of u that the kernel forms in registers."""
    return c["g"][:, None] * c["w"][None, :]


def backward_reference(c, mean32, invstd32):
    """float64 results of p2w_bn_relu_rowdot_bwd: (ref, caps), dicts of dz [M, C], dgamma, dbeta, dw [C], dbias [1]."""
    M = c["z"].shape[0]
    ref, caps = BR.backward_reference(materialised_gradient(c), c["z"], stage(c), None, mean32[None], invstd32[None])
    ref = dict(dz=ref["dz"], dgamma=ref["dgamma"][0], dbeta=ref["dbeta"][0])
    caps = dict(dz=caps["dz"], dgamma=caps["dgamma"][0], dbeta=caps["dbeta"][0])
    u = BR.replay32(c["z"], stage(c), mean32[None], invstd32[None])[0]["out"].double()
    g = c["g"].double()
    gu = g[:, None] * u
    ref["dw"] = gu.sum(0)
    caps["dw"] = EPS * ref["dw"].abs() + (M + 1) * D * gu.abs().sum(0)
    ref["dbias"] = g.sum().reshape(1)
    caps["dbias"] = EPS * ref["dbias"].abs() + M * D * g.abs().sum().reshape(1)
    return ref, caps
