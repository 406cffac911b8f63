"""Float64 references for the training route of the feature-propagation module (pointstowood_amd/ops.py: interp_add_relu, relu_bn,
FPModule; include/p2w.h: p2w_interp_add_relu*, p2w_relu_bn*), over oracle/ops.py's knn_interpolate and PyTorch's float64 autograd.

Two identities carry the fused route, and tests/test_fp_ref_cpu.py checks both in float64 before any kernel is compared:

  hoisting   knn_interpolate is linear in its features and its weights sum to 1, so for W0 = [Wc | Ws]
                 relu(Linear0(cat[interp(xc), x_skip])) = relu(interp(xc Wc^T) + (x_skip Ws^T + b0))
             in the output and in every gradient (xc, x_skip, W0, b0).
  relu_bn    out = BN(u), u = relu(z), training mode.  With xhat = (u - mean) invstd, dbeta = sum g, dgamma = sum g xhat:
                 dz = [z > 0] gamma invstd (g - dbeta / M - xhat dgamma / M)
             (the one-stage chain of tests/bn_chain_ref.py with the ReLU's mask in front).

The module-level cases (module_case) are what tests/test_gpu_fp.py trains on the GPU.  Their seeds are chosen so that every float64
pre-activation of every layer is further from 0 than MARGIN times that tensor's RMS: no ReLU mask can then differ between two fp32
routes whose pre-activations agree to fp32 rounding, and the comparison of the routes measures roundings, not mask flips.
test_fp_ref_cpu.py asserts that condition."""
import torch
import torch.nn.functional as F

from oracle import ops as O

BN_EPS, MOMENTUM = 1e-5, 0.1
MARGIN = 1e-4

# name -> k, the channel list, the coarse width Fc, points per batch (coarse, fine), the seed
MODULE_CASES = {
    # three ragged batches, 300 coarse and 600 fine points; the middle batch has fewer coarse points than k (rows of two neighbours)
    "ragged": dict(k=3, NN=[40, 32, 24], Fc=24, coarse=[150, 2, 148], fine=[300, 40, 260], seed=12),
    # the reference's fp4: one coarse point per batch at the origin, batch = arange(B); every fine row has one neighbour
    "fp4": dict(k=2, NN=[40, 32, 24], Fc=20, coarse=[1, 1, 1], fine=[210, 170, 220], seed=19),
}
_cases = {}


def state_keys(NN):
    """(key, shape) of MLP(NN) under FPModule's name, written from model.py:142-153,198-202: layer i = Seq(Lin, ReLU[, BN]), the
    BatchNorm in every layer but the first."""
    keys = []
    for i in range(1, len(NN)):
        keys += [(f"NN.{i - 1}.0.weight", (NN[i], NN[i - 1])), (f"NN.{i - 1}.0.bias", (NN[i],))]
        if i != 1:
            keys += [(f"NN.{i - 1}.2.{k}", (NN[i],)) for k in ("weight", "bias", "running_mean", "running_var")]
            keys += [(f"NN.{i - 1}.2.num_batches_tracked", ())]
    return keys


def build_case(k, NN, Fc, coarse, fine, seed):
    g = torch.Generator().manual_seed(seed)
    n_c, m, Fs = sum(coarse), sum(fine), NN[0] - Fc
    c = dict(k=k, NN=list(NN), Fc=Fc)
    c["batch"] = torch.repeat_interleave(torch.arange(len(coarse)), torch.tensor(coarse))
    c["batch_skip"] = torch.repeat_interleave(torch.arange(len(fine)), torch.tensor(fine))
    c["pos_skip"] = torch.rand(m, 3, generator=g)
    c["pos"] = torch.zeros(n_c, 3) if max(coarse) == 1 else torch.rand(n_c, 3, generator=g)
    c["x"], c["x_skip"] = torch.randn(n_c, Fc, generator=g), torch.randn(m, Fs, generator=g)
    c["g"] = torch.randn(m, NN[-1], generator=g)
    sd = {}
    for key, shape in state_keys(NN):
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros((), dtype=torch.long)
        elif key.endswith("running_var") or (key.endswith("weight") and len(shape) == 1):
            sd[key] = torch.rand(shape, generator=g) + 0.5
        elif key.endswith("running_mean"):
            sd[key] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 2:
            sd[key] = torch.randn(shape, generator=g) / shape[1] ** 0.5
        else:
            sd[key] = 0.5 * torch.randn(shape, generator=g)
    c["sd"] = sd
    return c


def module_case(name):
    if name not in _cases:
        _cases[name] = build_case(**MODULE_CASES[name])
    return _cases[name]


def interp(c, feat):
    """oracle knn_interpolate of the case's coarse features `feat` onto its fine points, positions in feat's dtype."""
    return O.knn_interpolate(feat, c["pos"].to(feat.dtype), c["pos_skip"].to(feat.dtype), c["batch"], c["batch_skip"], k=c["k"])


def layer0(c, x, x_skip, W0, b0, hoisted):
    """The pre-activation of layer 0: Linear0(cat[interp(x), x_skip]), or the hoisted form of it."""
    Fc = x.shape[1]
    if hoisted:
        return interp(c, x @ W0[:, :Fc].t()) + (x_skip @ W0[:, Fc:].t() + b0)
    return F.linear(torch.cat([interp(c, x), x_skip], 1), W0, b0)


def train_step(c, dtype=torch.float64, hoisted=False, lr=None):
    """One training step of the module on the CPU in `dtype` under ordinary autograd (training-mode F.batch_norm): the output, the
    gradients to x, x_skip and every parameter by state-dict name, the running statistics after the step, the pre-activations of every
    layer (`pre`); with lr, every parameter after one AdamW step (`step.<name>`)."""
    sd, nl = c["sd"], len(c["NN"]) - 1
    leaf = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    x, x_skip = (c[k].to(dtype).clone().requires_grad_() for k in ("x", "x_skip"))
    r, pre = {}, []
    z = layer0(c, x, x_skip, leaf["NN.0.0.weight"], leaf["NN.0.0.bias"], hoisted)
    pre.append(z.detach())
    h = torch.relu(z)
    for i in range(1, nl):
        z = F.linear(h, leaf[f"NN.{i}.0.weight"], leaf[f"NN.{i}.0.bias"])
        pre.append(z.detach())
        u = torch.relu(z)
        p = f"NN.{i}.2."
        r[p + "running_mean"] = (1 - MOMENTUM) * sd[p + "running_mean"].to(dtype) + MOMENTUM * u.mean(0).detach()
        r[p + "running_var"] = (1 - MOMENTUM) * sd[p + "running_var"].to(dtype) + MOMENTUM * u.var(0, unbiased=True).detach()
        h = F.batch_norm(u, None, None, leaf[p + "weight"], leaf[p + "bias"], True, 0.0, BN_EPS)
    (h * c["g"].to(dtype)).sum().backward()
    r.update(out=h.detach(), x=x.grad, x_skip=x_skip.grad, **{k: v.grad for k, v in leaf.items()})
    if lr is not None:
        torch.optim.AdamW(list(leaf.values()), lr=lr).step()
        r.update({"step." + k: v.detach().clone() for k, v in leaf.items()})
    r["pre"] = pre
    return r


def margins(pre):
    """min |z| / rms(z) per pre-activation tensor."""
    return [float(z.abs().min() / z.pow(2).mean().sqrt()) for z in pre]


def relu_bn_backward(z, gamma, g, eps=BN_EPS):
    """The closed form above in z's dtype: (dz, dgamma, dbeta)."""
    M = z.shape[0]
    u = torch.relu(z)
    mean = u.sum(0) / M
    var = ((u * u).sum(0) / M - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (u - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    gv = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    return torch.where(z > 0, gv, torch.zeros_like(gv)), dgamma, dbeta
