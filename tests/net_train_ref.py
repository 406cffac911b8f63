"""The training forward of the reference's Net (model.py:226-245 with training-mode BatchNorm) as one composition over a plain state
dict and oracle/ops.py, in any dtype on the CPU, differentiable by ordinary autograd - float64 is the reference that
tests/test_gpu_train_net.py judges pointstowood_amd.train.Net's two routes against, float32 the plain composition's own noise.

Geometry is not part of the comparison: the sample indices and the edges of every set-abstraction level are GIVEN (`geo`: what the
fp32 run drew and found, or on the CPU what oracle.ops finds), and positions are carried in float32 exactly as the modules carry them
(the division and multiplication by sf are single IEEE operations: the same bits on both devices) and cast where they enter
arithmetic.  The neighbours of the feature-propagation levels are oracle.ops.knn's on those float32 positions.  ReflectanceYesNo is
omitted by its effect (exactly 1.0, zero gradients: oracle/net.py).

The case: two voxels of 600 and 200 uniform points in cubes of 0.5 m and 0.35 m with reflectance, C = 8 - in training mode the levels
hold 300 / 150 / 75 and 100 / 50 / 25 points, so sa3's k = 32 search still has 150 and 50 sources per voxel, and sa1's ball of 0.08 m
holds about ten points; in eval mode the voxel grid keeps enough points per level for the same to hold."""
import torch
import torch.nn.functional as F

from oracle import ops as O
from pointstowood_amd import synthetic_voxels as SV
from pointstowood_amd import synthetic_weights as SW

C = 8
SIZES = ((0.5, 600), (0.35, 200))
BN_EPS = 1e-5
LEVELS = (("sa1_module", 0.04), ("sa2_module", 0.08), ("sa3_module", 0.16))
K = 32


def inputs(seed):
    """pos [800, 3], batch, reflectance, sf [2] (fp32, CPU) of the case, and a cotangent g [800] for the logits."""
    b = SV.collate([SV.uniform_voxel(side, n, 100 * seed + i, reflectance=True) for i, (side, n) in enumerate(SIZES)])
    g = torch.randn(b["pos"].shape[0], generator=torch.Generator().manual_seed(seed)) / b["pos"].shape[0]
    return dict(pos=b["pos"], batch=b["batch"], reflectance=b["reflectance"], sf=b["sf"], g=g)


def state(seed):
    return SW.synth_state_dict(1, C, seed=seed)


def fixed_sample(n):
    """The injected training sample: every second point, ascending."""
    return torch.arange(0, n - n % 2, 2)


def geometry(inp, sample=fixed_sample):
    """idx and edge_index [2, E] (source, target) of the three levels as oracle.ops finds them for `sample` - what the GPU searches
    must return too (the test asserts it)."""
    pos, batch, geo = inp["pos"][:, :3], inp["batch"], []
    for _, res in LEVELS:
        idx = sample(pos.shape[0])
        if res == 0.04:
            row, col = O.radius(pos, pos[idx], res * 2, batch, batch[idx], max_num_neighbors=K)
        else:
            row, col = O.knn(pos, pos[idx], K, batch_x=batch, batch_y=batch[idx])
        geo.append(dict(idx=idx, edge_index=torch.stack([col, row], 0)))
        # the positions a level hands on have been divided and multiplied by sf (model.py:122-124)
        s = inp["sf"][batch].unsqueeze(-1)
        pos, batch = ((pos / s) * s)[idx], batch[idx]
    return geo


def _bn(P, p, x):
    return F.batch_norm(x, None, None, P[p + ".weight"], P[p + ".bias"], True, 0.0, BN_EPS)


def _mlp(P, p, x, n_layers):
    for i in range(n_layers):
        x = F.relu(F.linear(x, P[f"{p}.{i}.0.weight"], P[f"{p}.{i}.0.bias"]))
        if i != 0:
            x = _bn(P, f"{p}.{i}.2", x)
    return x


def _conv1x1(P, p, x):
    return F.linear(x, P[p + ".weight"][:, :, 0], P[p + ".bias"])


def _dsc(P, p, x):
    x = x * P[p + ".depthwise_conv.weight"][:, 0, 0] + P[p + ".depthwise_conv.bias"]
    x = F.relu(_bn(P, p + ".depthwise_bn", x))
    return F.relu(_bn(P, p + ".pointwise_bn", _conv1x1(P, p + ".pointwise_conv", x)))


def _resblock(P, p, x):
    out = F.relu(_bn(P, p + ".expand.1", _conv1x1(P, p + ".expand.0", x)))
    out = _dsc(P, p + ".conv.0", out)
    out = F.relu(_bn(P, p + ".conv.1", out))
    out = _dsc(P, p + ".conv.3", out)
    out = _bn(P, p + ".conv.4", out)
    out = _bn(P, p + ".project.1", _conv1x1(P, p + ".project.0", out))
    return F.relu(out + x)


def _pointnet_conv(P, p, x, pos_src, pos_dst, src, dst):
    pos_j, pos_i = pos_src[src], pos_dst[dst]
    rel = pos_j[:, :3] - pos_i[:, :3]
    dmax, _ = O.scatter_max(torch.norm(rel, dim=1, keepdim=True), dst, dim=0, dim_size=pos_dst.shape[0])
    msg = torch.cat([x[src], rel / (dmax[dst] + 1e-8), pos_j[:, 3:4]], dim=1)
    return O.segment_max_rows(_mlp(P, p + ".local_nn", msg, 2), dst, pos_dst.shape[0])


def _interp(x, pos_x, pos_y, batch_x, batch_y, k):
    y_idx, x_idx = O.knn(pos_x, pos_y, k, batch_x=batch_x, batch_y=batch_y)
    diff = (pos_x[x_idx] - pos_y[y_idx]).to(x.dtype)
    w = 1.0 / torch.clamp((diff * diff).sum(dim=-1, keepdim=True), min=1e-16)
    m = pos_y.shape[0]
    num = torch.zeros((m, x.shape[1]), dtype=x.dtype).index_add(0, y_idx, x[x_idx] * w)
    den = torch.zeros((m, 1), dtype=x.dtype).index_add(0, y_idx, w)
    return num / den


def forward(P, inp, geo):
    """logits [N] in the dtype of the state dict P."""
    dtype = P["conv1.weight"].dtype
    pos, batch, refl, sf = inp["pos"][:, :3], inp["batch"], inp["reflectance"], inp["sf"]
    x = _mlp(P, "stem_mlp", pos.to(dtype), 1)
    levels = [(x, pos, batch)]
    for (p, _), g in zip(LEVELS, geo):
        idx, (src, dst) = g["idx"], g["edge_index"]
        s = sf[batch].unsqueeze(-1)
        pos4 = torch.cat([pos / s, refl.unsqueeze(-1)], dim=-1)                 # fp32, as the module scales it
        x = _pointnet_conv(P, p + ".conv", x, pos4.to(dtype), pos4[idx].to(dtype), src, dst)
        x = _resblock(P, p + ".residual_block", x)
        pos, batch, refl = ((pos / s) * s)[idx], batch[idx], refl[idx]
        levels.append((x, pos, batch))
    x4 = O.global_max_pool(_mlp(P, "sa4_module.NN", torch.cat([x, pos.to(dtype)], dim=1), 2), batch)
    nb = x4.shape[0]
    cur = (x4, torch.zeros((nb, 3)), torch.arange(nb))
    for l, skip in zip((4, 3, 2, 1), reversed(levels)):
        h = _interp(cur[0], cur[1], skip[1], cur[2], skip[2], 2)
        cur = (_mlp(P, f"fp{l}_module.NN", torch.cat([h, skip[0]], dim=1), 2), skip[1], skip[2])
    x = F.relu(_bn(P, "norm", _conv1x1(P, "conv1", cur[0])))
    return _conv1x1(P, "conv2", x)[:, 0]


def step(sd, inp, geo, dtype):
    """Forward and backward of sum(logits g) in `dtype`: (logits, {parameter name: gradient})."""
    P = {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    logits = forward(P, inp, geo)
    (logits * inp["g"].to(dtype)).sum().backward()
    return logits.detach(), {k: v.grad for k, v in P.items() if v.grad is not None}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
