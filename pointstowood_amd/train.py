"""The reference's ``src/model.py`` as trainable modules on MI355X: ``from pointstowood_amd.train import Net`` in place of
``from src.model import Net`` (route A-train).

Same constructors, same submodule names and therefore the same 257-key ``state_dict`` (``synthetic_weights.key_table``: a
checkpoint saved here loads into ``pointstowood_amd.Net``, route A, with ``strict=True``, and into the reference), the same
``forward`` signatures over a duck-typed batch with ``pos``, ``batch``, ``reflectance``, ``sf``.  Every level is built from the
operator route's modules - ``ops.PointNetConv``, ``ops.InvertedResidualBlock``, ``ops.FPModule`` - and what those leave over
(the sampling, the searches, the global level and the head) is written here on ``ops`` callables: no PyG, no torch-cluster.

``fused`` (class attribute of ``Net``, ``SAModule`` and ``GlobalSAModule``, default True) selects in training mode the fused routes
(``bn_chain``, ``edge_layer1``, ``relu_bn``, ``interp_add_relu``, ``bn_relu_rowdot``: the same function as the plain statements,
other roundings, the same bits on every run); False runs the reference's statements one by one on ``torch.nn`` modules and the
plain ``ops`` callables - the baseline of an A/B comparison.  Assigning ``net.fused`` on a ``Net`` instance assigns it on every
submodule that has the switch (``ops.FPModule`` included).  ``ops.PointNetConv.fused_bn_max`` is a separate switch, default False:
``net.fused`` does not touch it; ``trainer.set_fused_bn_max(net)`` (``train.py --fused_bn_max``) sets it on the three ``PointNetConv``
instances of a ``Net``, whose layer-2 tail then runs through ``ops.relu_bn_max`` - under autocast on the GEMM's 16-bit output as it
is.  Gradients with respect to positions are not provided.

``sampler`` (attribute of ``Net`` and ``SAModule``, default None): a ``DeviceSampler`` draws the three training samples on the GPU
(``ops.random_subset``) as a function of (seed, epoch, step, level) in place of the reference's CPU ``randperm`` - the same law, a
uniform half of the level's rows, from another random stream.  None is the reference's draw."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d, Conv1d, Linear, ReLU, Sequential

from . import ops
from .synthetic_weights import fp_channels, sa_channels


def initialize_weights(model):
    """The reference's initialisation (``model.py:9-16``) by its effect: zero biases; Xavier-uniform Linear weights; Kaiming-uniform
    (fan_in, ReLU gain) Conv1d weights.  A Conv1d weight takes the Xavier draw first and is then overwritten, as there, so a seeded
    construction consumes the generator exactly as the reference's does and gives the reference's weights."""
    init = torch.nn.init
    for layer in model.modules():
        if not isinstance(layer, (Linear, Conv1d)):
            continue
        init.xavier_uniform_(layer.weight)
        if isinstance(layer, Conv1d):
            init.kaiming_uniform_(layer.weight, mode="fan_in", nonlinearity="relu")
        if layer.bias is not None:
            init.zeros_(layer.bias)


def MLP(channels):
    """The reference's layer stack (``model.py:198-202``) and therefore its keys ``<i>.0.*`` / ``<i>.2.*``: per pair of widths a
    Sequential of Linear and ReLU, followed by a BatchNorm1d in every layer but the first."""
    layers = []
    for i, (c_in, c_out) in enumerate(zip(channels[:-1], channels[1:])):
        block = [Linear(c_in, c_out), ReLU()]
        if i > 0:
            block.append(BatchNorm1d(c_out))
        layers.append(Sequential(*block))
    return Sequential(*layers)


class ReflectanceYesNo(torch.nn.Module):
    """The reference's per-voxel gate on the reflectance channel (``model.py:155-175``), kept for its six parameters
    (``fc1``, ``fc2``, ``fc3``): a two-layer MLP per point, its mean per voxel, one score per voxel, and a hard gumbel-softmax of that
    score over an axis of size 1 - exactly 1.0 for every input, with an exactly zero gradient to every parameter."""

    def __init__(self, input_dim, hidden_dim, temperature=1.0):
        super().__init__()
        self.fc1 = Linear(input_dim, hidden_dim)
        self.fc2 = Linear(hidden_dim, hidden_dim)
        self.fc3 = Linear(hidden_dim, 1)
        self.temperature = temperature

    def forward(self, x, batch):
        voxel = batch.long()
        h = torch.relu(self.fc2(torch.relu(self.fc1(x.float()))))
        n_voxels = int(voxel.max()) + 1
        total = h.new_zeros((n_voxels, h.shape[1])).index_add(0, voxel, h)
        count = torch.bincount(voxel, minlength=n_voxels).to(h.dtype)
        score = self.fc3(total / count.unsqueeze(1))
        gate = F.gumbel_softmax(score, tau=self.temperature, hard=True)[:, 0]
        return gate[voxel]


class _ZeroGrads(torch.autograd.Function):
    """``x`` passed through; in the backward every tensor of ``params`` receives zeros.  What ``ReflectanceYesNo`` contributes to a
    training step without evaluating it: a parameter whose gradient is zero is still decayed by AdamW, one whose gradient is None is
    skipped."""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.save_for_backward(*params)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad_out):
        return (grad_out, *[torch.zeros_like(p) for p in ctx.saved_tensors])


def _conv_plain(conv, x, pos_src, pos_dst, edge_index):
    """The reference's edge message and max aggregation (``pointnet.py:116-132``) on materialised edge tensors: per edge the source's
    features, the offset to the target divided by the target's largest offset length (+ 1e-8) and the source's reflectance, through
    ``conv.local_nn``, then the maximum per target."""
    src, dst = edge_index[0], edge_index[1]
    n_dst = pos_dst.shape[0]
    offset = pos_src[src, :3] - pos_dst[dst, :3]
    reach = ops.scatter_max(torch.norm(offset, dim=1, keepdim=True), dst, dim=0, dim_size=n_dst)[0]
    geo = torch.zeros((src.numel(), 4), device=offset.device)
    geo[:, :3] = offset / (reach[dst] + 1e-8)
    geo[:, 3] = pos_src[src, 3]
    out = ops.scatter_max(conv.local_nn(torch.cat([x[src], geo], dim=1)), dst, dim=0, dim_size=n_dst)[0]
    return out if conv.global_nn is None else conv.global_nn(out)


class DeviceSampler:
    """The training sample of the three set-abstraction levels drawn on the device: level ``level`` of step ``step`` of epoch ``epoch``
    keeps ``ops.random_subset(n, n // 2, seed, counter=(4 * step + level, epoch))`` - nothing of it depends on the process-wide
    generators, so a run resumed at (epoch, step) draws what the uninterrupted run drew.  ``Net.forward`` advances ``step`` once per
    training-mode forward; ``set_epoch`` starts an epoch at step 0; ``step`` may be assigned."""

    def __init__(self, seed):
        self.seed, self.epoch, self.step = int(seed), 0, 0

    def set_epoch(self, epoch):
        self.epoch, self.step = int(epoch), 0

    def draw(self, level, n, device):
        return ops.random_subset(n, n // 2, self.seed, counter=(4 * self.step + level, self.epoch), device=device)

    def state_dict(self):
        """Everything a draw depends on: three integers."""
        return {"seed": self.seed, "epoch": self.epoch, "step": self.step}

    def load_state_dict(self, state):
        self.seed, self.epoch, self.step = int(state["seed"]), int(state["epoch"]), int(state["step"])


class SAModule(torch.nn.Module):
    """The reference's set-abstraction level (``model.py:87-127``): sample centres, search their neighbours, ``PointNetConv`` on
    positions divided by the voxel's ``sf``, the inverted residual block.

    ``fused = True``: ``self.conv`` and ``self.residual_block`` run their own routes (training: ``edge_layer1`` and ``bn_chain``; eval:
    the fused inference kernel and the plain block), and ``reflectanceyesno`` is not evaluated - its result is exactly 1.0, so nothing
    is multiplied - but its six parameters still receive ZERO gradients, as they do in the reference.  One deviation: the reference
    skips the call (and leaves those gradients None) in a batch whose reflectance sums to exactly 0; here the zeros are attached
    regardless, which needs no host synchronisation.  ``fused = False``: the reference's statements, with the plain compositions of
    the conv and the block in both modes.  The caller's tensors are not written to.

    ``sampler`` (default None): in training mode a ``DeviceSampler`` draws the sample as this module's ``level`` (0, 1, 2 in ``Net``) and
    ``random_sample`` is not called; eval mode never looks at it."""

    fused = True
    sampler = None
    level = 0

    def __init__(self, resolution, radius, k, NN, RNN):
        super().__init__()
        self.resolution, self.radius, self.k = resolution, radius, k
        self.conv = ops.PointNetConv(local_nn=MLP(NN), global_nn=None, add_self_loops=False, radius=radius)
        self.residual_block = ops.InvertedResidualBlock(RNN, RNN)
        self.reflectanceyesno = ReflectanceYesNo(input_dim=1, hidden_dim=32)

    def random_sample(self, num_points):
        """The training sample: the first half of a CPU ``randperm`` from the global generator, ascending - the reference's draw, so
        a seeded run takes the reference's sample.  Override it to inject one."""
        return torch.randperm(num_points)[:num_points // 2].sort().values

    def voxelsample(self, pos, batch, resolution):
        """The eval sample: one point per occupied cell of a ``resolution`` grid."""
        return ops.consecutive_cluster(ops.voxel_grid(pos, resolution, batch))[1]

    def forward(self, x, pos, batch, reflectance, sf):
        xyz, gated = pos[:, :3], reflectance
        if not self.fused and torch.sum(reflectance) != 0:
            gated = reflectance * self.reflectanceyesno(reflectance.unsqueeze(-1), batch)
        if self.training:
            if self.sampler is not None:
                keep = self.sampler.draw(self.level, xyz.shape[0], xyz.device)
            else:
                keep = self.random_sample(xyz.shape[0]).to(xyz.device)      # the one host-to-device copy of the index
        else:
            keep = self.voxelsample(xyz, batch, self.resolution)
        centres, centre_batch = xyz[keep], batch[keep]
        if self.resolution == 0.04:                                         # the finest level searches a ball, the others k nearest
            target, source = ops.radius(xyz, centres, 2 * self.resolution, batch, centre_batch, max_num_neighbors=self.k)
        else:
            target, source = ops.knn(xyz, centres, self.k, batch_x=batch, batch_y=centre_batch)
        edge_index = torch.stack([source, target])
        scale = sf[batch].unsqueeze(-1)
        scaled = torch.cat([xyz / scale, gated.unsqueeze(-1)], dim=1)       # [n, 4]: what the conv sees
        if self.fused:
            x = self.conv(x, (scaled, scaled[keep]), edge_index)
            if self.training and torch.is_grad_enabled() and x.requires_grad:
                x = _ZeroGrads.apply(x, *self.reflectanceyesno.parameters())
            x = self.residual_block(x)
        else:
            x = self.residual_block._forward_plain(_conv_plain(self.conv, x, scaled, scaled[keep], edge_index))
        # the positions handed on have been divided and multiplied by sf, as the reference's are (model.py:122-126)
        return x, (scaled[:, :3] * scale)[keep], centre_batch, reflectance[keep], sf


class GlobalSAModule(torch.nn.Module):
    """The reference's global level (``model.py:129-140``): an MLP on features and positions, the maximum per voxel, and one point
    at the origin per voxel.  Training with ``fused = True``: layer 0 is ``F.linear`` + ReLU, layer 1 is ``ops.relu_bn`` on its GEMM's
    output, then ``ops.global_max_pool``.  Eval mode and ``fused = False``: ``self.NN`` as it stands."""

    fused = True

    def __init__(self, NN):
        super().__init__()
        self.NN = MLP(NN)

    def forward(self, x, pos, batch, reflectance, sf):
        h = torch.cat([x, pos], dim=1)
        if self.training and self.fused:
            # ReLU, BatchNorm and the max as three steps, not ops.relu_bn_max: that kernel's work item is 16 consecutive targets, and
            # here a target is a whole voxel of thousands of rows - with B targets a single item would walk the whole tensor
            lin0, lin1, bn = self.NN[0][0], self.NN[1][0], self.NN[1][2]
            h = torch.relu(F.linear(h, lin0.weight, lin0.bias))
            h = ops.relu_bn(F.linear(h, lin1.weight, lin1.bias), bn)        # (fp32 out: it feeds a max, not a GEMM - ops.half_io)
        else:
            h = self.NN(h)
        pooled = ops.global_max_pool(h, batch)
        n = pooled.shape[0]
        return pooled, pos.new_zeros((n, 3)), torch.arange(n, device=batch.device), reflectance.new_zeros(n), sf


class Net(torch.nn.Module):
    """The reference's network (``model.py:204-245``): the stem, three set-abstraction levels, the global level, four
    feature-propagation levels and the head, on rows.  Training with ``fused = True`` and ``num_classes == 1`` (what the trainer
    builds) runs the head behind ``conv1`` as ``ops.bn_relu_rowdot``: neither ``relu(norm(conv1(x)))`` [N, 16 C] nor its gradient is
    formed.  More classes, eval mode and ``fused = False`` run the plain statements.  The output is [N] float32 for one class
    ([num_classes, N] otherwise), as the reference's.  Assigning ``net.sampler`` hands the object to the three set-abstraction
    levels; a training-mode forward with a sampler ends with ``sampler.step += 1``."""

    fused = True
    sampler = None

    def __init__(self, num_classes, C=32):
        super().__init__()
        self.num_classes = num_classes
        self.stem_mlp = MLP([3, C])
        for level, (resolution, (channels, width)) in enumerate(zip((0.04, 0.08, 0.16), sa_channels(C)), start=1):
            setattr(self, f"sa{level}_module", SAModule(resolution, resolution, 32, channels, width))
            getattr(self, f"sa{level}_module").level = level - 1
        self.sa4_module = GlobalSAModule([16 * C + 3, 16 * C, 16 * C])
        for level in (4, 3, 2, 1):
            setattr(self, f"fp{level}_module", ops.FPModule(2, fp_channels(C)[level]))
        self.conv1 = Conv1d(16 * C, 16 * C, 1)
        self.conv2 = Conv1d(16 * C, num_classes, 1)
        self.norm = BatchNorm1d(16 * C)
        initialize_weights(self)

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if name == "fused":                                      # the switch of an instance is the switch of everything below it
            for m in self.modules():
                if m is not self and hasattr(type(m), "fused"):
                    m.fused = value
        if name == "sampler":
            for m in self.modules():
                if isinstance(m, SAModule):
                    m.sampler = value

    def forward(self, data):
        data.x = self.stem_mlp(data.pos[:, :3])                  # the reference leaves the stem features on the batch
        level = (data.x, data.pos, data.batch, data.reflectance, data.sf)
        skips = [level[:3]]
        for sa in (self.sa1_module, self.sa2_module, self.sa3_module):
            level = sa(*level)
            skips.append(level[:3])
        coarse = self.sa4_module(*level)[:3]
        for fp, skip in zip((self.fp4_module, self.fp3_module, self.fp2_module, self.fp1_module), reversed(skips)):
            coarse = fp(*coarse, *skip)
        z = F.linear(coarse[0], self.conv1.weight[:, :, 0], self.conv1.bias)
        if self.training and self.sampler is not None:
            self.sampler.step += 1                               # the next forward draws other samples
        if self.training and self.fused and self.num_classes == 1:
            return ops.bn_relu_rowdot(z, self.norm, self.conv2.weight, self.conv2.bias)
        out = F.linear(F.relu(self.norm(z)), self.conv2.weight[:, :, 0], self.conv2.bias)
        return torch.squeeze(out.t()).to(torch.float)
