"""The training feed on the GPU: the reference's ``TrainingDataset`` (``pointstowood/src/trainer.py:28-60``), its ``augmentations``
(``pointstowood/src/augmentation.py:41-55``) and PyG's shuffling loader, over ``p2w_train_feed`` (``csrc/p2w_feed.hip``).

* ``TrainingSet``      - every voxel file read ONCE; ``xyzr`` [N, 4] float32, ``y`` [N] float32 and ``set_ptr`` [V + 1] int64 stay on the
                         device (20 B per point), the voxel lengths on the host.
* ``plan_from_draws``  - the reference's augmentation decisions as plan records: a pure host function of its uniform draws.
* ``draw_plan``        - the draws themselves, vectorised from a ``torch.Generator``.
* ``train_feed``       - the kernel's wrapper: one batch from ``ids``, two launches, no host synchronisation.
* ``TrainingFeed``     - the loader: per epoch one plan upload, per batch one small ``ids`` / ``out_ptr`` upload and one kernel call;
                         yields ``data.Batch(pos, reflectance, y, sf, batch, ptr)`` on the device.

The arithmetic is not the reference's order of operations: the kernel centres first (float64 centroid, one rounding) and rotates after,
which is the same function (``mean(x R) = mean(x) R``) without the reference's three float32 matrix products on plot coordinates.
numpy and torch only; CUDA tensors only (there is no CPU fallback).
"""
from __future__ import annotations

import glob
import hashlib
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr as _p
from .data import Batch

REFL_KEEP, REFL_ZERO, REFL_PERTURB = 0, 1, 2                      # include/p2w.h p2w_feed_plan.refl_mode
PLAN_DTYPE = np.dtype([("refl_mode", np.int32), ("rotate", np.int32), ("R", np.float32, (9,)), ("reserved", np.int32)])
assert PLAN_DTYPE.itemsize == 48


class TrainingSet:
    """A whole training set on the device.  ``voxels``: a directory of ``voxel_*.pt`` files (every ``*.pt`` of it, sorted, as the
    reference's ``glob``) or a list of [n_i, >= 5] tensors; columns 0 .. 2 are x, y, z, ``reflectance_index`` and ``label_index`` as in
    the reference.  Each file is read once.  ``xyzr`` [N, 4] float32, ``y`` [N] float32 and ``set_ptr`` [V + 1] int64 live on
    ``device``; ``lengths`` (numpy int64 [V]) stays on the host.  20 bytes per point - a 10^8-point set is 2 GB; a set beyond
    ``max_bytes`` raises (there is no host-resident fallback)."""

    def __init__(self, voxels, device="cuda", reflectance_index: int = 3, label_index: int = 4, max_bytes: int = 64 << 30):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TrainingSet keeps the set on an MI355X (cuda) device; there is no CPU fallback")
        if isinstance(voxels, (str, os.PathLike)):
            if not voxels:
                raise ValueError("The 'voxels' parameter cannot be empty.")
            self.keys = sorted(glob.glob(os.path.join(voxels, "*.pt")))
            if not self.keys:
                raise ValueError(f"{voxels}: no *.pt voxel file")
            load = (torch.as_tensor(torch.load(k, map_location="cpu")) for k in self.keys)
        else:
            voxels = list(voxels)
            if not voxels:
                raise ValueError("The 'voxels' parameter cannot be empty.")
            self.keys = list(range(len(voxels)))
            load = (torch.as_tensor(v) for v in voxels)
        cols = [0, 1, 2, int(reflectance_index)]
        rows, labels, lengths, used = [], [], [], 0
        for key, pc in zip(self.keys, load):
            if pc.dim() != 2 or pc.shape[1] <= max(cols + [int(label_index)]):
                raise ValueError(f"voxel {key}: a [n, > {max(cols + [int(label_index)])}] tensor is needed, got {list(pc.shape)}")
            used += 20 * pc.shape[0]
            if used > max_bytes:
                raise MemoryError(f"the training set needs more than max_bytes = {max_bytes} bytes of device memory (20 bytes per "
                                  f"point; voxel {key} passes the limit); a host-resident set is not provided")
            pc = pc.detach().cpu()
            rows.append(pc[:, cols].to(torch.float32))
            labels.append(pc[:, int(label_index)].to(torch.float32))
            lengths.append(int(pc.shape[0]))
        self.lengths = np.asarray(lengths, dtype=np.int64)
        ptr = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(self.lengths)])
        self.device = device
        self.xyzr = torch.cat(rows, 0).contiguous().to(device)
        self.y = torch.cat(labels, 0).contiguous().to(device)
        self.set_ptr = torch.from_numpy(ptr).to(device)

    def __len__(self):
        return len(self.lengths)

    @property
    def num_points(self):
        return int(self.xyzr.shape[0])


def rotation_from_angles(angles_deg_uniform):
    """R [V, 3, 3] float32 of ``rotate_3d`` (augmentation.py:5-12) from its uniform draws u [V, 3]: the angles ``deg2rad(u * 180 - 90)``
    and their cos / sin in float32 with the reference's torch calls, the matrices as written there, and roll @ pitch @ yaw formed ONCE in
    float64 and rounded to float32 (the reference multiplies the points through the three float32 matrices in turn)."""
    u = torch.as_tensor(angles_deg_uniform, dtype=torch.float32).reshape(-1, 3)
    rot = torch.deg2rad(u * 180 - 90)
    c, s = torch.cos(rot).double().numpy(), torch.sin(rot).double().numpy()
    V = u.shape[0]
    roll, pitch, yaw = (np.tile(np.eye(3), (V, 1, 1)) for _ in range(3))
    roll[:, 1, 1], roll[:, 1, 2], roll[:, 2, 1], roll[:, 2, 2] = c[:, 0], -s[:, 0], s[:, 0], c[:, 0]
    pitch[:, 0, 0], pitch[:, 0, 2], pitch[:, 2, 0], pitch[:, 2, 2] = c[:, 1], s[:, 1], -s[:, 1], c[:, 1]
    yaw[:, 0, 0], yaw[:, 0, 1], yaw[:, 1, 0], yaw[:, 1, 1] = c[:, 2], -s[:, 2], s[:, 2], c[:, 2]
    return (roll @ pitch @ yaw).astype(np.float32)


def plan_from_draws(u_refl, u_pos, u_angles, mode: str = "train"):
    """The reference's decisions (augmentation.py:41-55) for V voxels as plan records (``PLAN_DTYPE`` [V]): ``u_refl < 0.25`` silences
    the reflectance; in ``mode == "train"`` only, ``0.25 <= u_refl < 0.5`` perturbs it; ``u_pos < 0.25`` rotates by the angles of
    ``u_angles`` [V, 3] (``rotation_from_angles``).  The comparisons are made on float32 values, as the reference's ``torch.rand(1)``
    draws are.  A voxel that is not rotated gets the identity and ``rotate = 0``.  Pure host arithmetic."""
    if mode not in ("train", "test"):
        raise ValueError(f"mode must be 'train' or 'test', got {mode!r}")
    u_refl = np.asarray(torch.as_tensor(u_refl, dtype=torch.float32).reshape(-1).numpy())
    u_pos = np.asarray(torch.as_tensor(u_pos, dtype=torch.float32).reshape(-1).numpy())
    V = u_refl.shape[0]
    u_angles = torch.as_tensor(u_angles, dtype=torch.float32).reshape(-1, 3)
    if u_pos.shape[0] != V or u_angles.shape[0] != V:
        raise ValueError(f"{V} reflectance draws, {u_pos.shape[0]} position draws and {u_angles.shape[0]} angle triples")
    quarter, half = np.float32(0.25), np.float32(0.5)
    plan = np.zeros(V, dtype=PLAN_DTYPE)
    plan["refl_mode"][u_refl < quarter] = REFL_ZERO
    if mode == "train":
        plan["refl_mode"][(u_refl >= quarter) & (u_refl < half)] = REFL_PERTURB
    rotate = u_pos < quarter
    plan["rotate"] = rotate
    R = rotation_from_angles(u_angles)
    R[~rotate] = np.eye(3, dtype=np.float32)
    plan["R"] = R.reshape(V, 9)
    return plan


def identity_plan(V: int):
    """``augmentation=False``: every record keeps the reflectance and does not rotate."""
    plan = np.zeros(int(V), dtype=PLAN_DTYPE)
    plan["R"] = np.eye(3, dtype=np.float32).reshape(9)
    return plan


def draw_plan(V: int, mode: str, generator: torch.Generator):
    """One epoch's plan: ``u_refl`` [V], ``u_pos`` [V] and ``u_angles`` [V, 3] drawn in that order from ``generator`` (CPU,
    ``torch.rand``) and handed to ``plan_from_draws``.  The DISTRIBUTIONS and the DECISIONS are the reference's; its random stream is
    not and cannot be: the reference draws from the global generator inside 32 worker processes, the angles only for the voxels it
    rotates."""
    V = int(V)
    u_refl = torch.rand(V, generator=generator)
    u_pos = torch.rand(V, generator=generator)
    u_angles = torch.rand(V, 3, generator=generator)
    return plan_from_draws(u_refl, u_pos, u_angles, mode)


def plan_to_device(plan, device):
    plan = np.ascontiguousarray(plan, dtype=PLAN_DTYPE)
    return torch.from_numpy(plan.view(np.int32).reshape(-1, 12).copy()).to(device)


def train_feed(tset: TrainingSet, ids, out_ptr, n: int, plan, seed: int = 0, epoch: int = 0, noise=None, words: bool = False):
    """One batch through ``p2w_train_feed``: ``ids`` [B] int32 and ``out_ptr`` [B + 1] int64 DEVICE tensors (distinct voxels;
    ``out_ptr`` the running sum of their lengths, ``n = out_ptr[B]`` known to the host), ``plan`` the [V, 12] int32 device tensor of
    ``plan_to_device``.  Returns ``(pos [n, 3], reflectance [n], y [n], batch [n] int64, sf [B], nonfinite [B] int32)`` and, with
    ``words=True``, the generator's words [n, 4] (int32 storage of the uint32 values) as a seventh entry.  No host wait."""
    _lib.require_cuda(tset.xyzr, ids, out_ptr, plan, noise)
    dev = tset.xyzr.device
    B, n, V = int(ids.numel()), int(n), len(tset)
    if ids.dtype != torch.int32 or out_ptr.dtype != torch.int64 or out_ptr.numel() != B + 1:
        raise ValueError("ids must be int32 [B] and out_ptr int64 [B + 1]")
    if plan.dtype != torch.int32 or plan.numel() != 12 * V or not plan.is_contiguous():
        raise ValueError(f"plan must be a contiguous int32 [{V}, 12] tensor (plan_to_device)")
    if noise is not None and (noise.dtype != torch.float32 or noise.numel() != n or not noise.is_contiguous()):
        raise ValueError(f"noise must be a contiguous float32 tensor of {n} elements")
    pos = torch.empty((n, 3), dtype=torch.float32, device=dev)
    refl = torch.empty(n, dtype=torch.float32, device=dev)
    y = torch.empty(n, dtype=torch.float32, device=dev)
    batch = torch.empty(n, dtype=torch.int64, device=dev)
    sf = torch.empty(B, dtype=torch.float32, device=dev)
    nonfinite = torch.empty(B, dtype=torch.int32, device=dev)
    w = torch.empty((n, 4), dtype=torch.int32, device=dev) if words else None
    L = lib()
    ws = torch.empty(max(16, int(L.p2w_train_feed_ws_size(n, B))), dtype=torch.uint8, device=dev)
    check(L.p2w_train_feed(_p(tset.xyzr), _p(tset.y), _p(tset.set_ptr), tset.num_points, V, _p(ids), _p(out_ptr), B, n, _p(plan),
                           int(seed) & (2**64 - 1), int(epoch) & 0xffffffff, _p(noise), _p(pos), _p(refl), _p(y), _p(batch), _p(sf),
                           _p(nonfinite), _p(w), _p(ws), ws.numel(), _lib.stream()), "p2w_train_feed")
    out = (pos, refl, y, batch, sf, nonfinite)
    return out + (w,) if words else out


def _seed_of(seed: int, epoch: int, what: str) -> int:
    """A 63-bit generator seed per (seed, epoch, purpose)."""
    return int.from_bytes(hashlib.sha256(f"{int(seed)}:{int(epoch)}:{what}".encode()).digest()[:8], "little") >> 1


class TrainingFeed:
    """The reference's training loader (trainer.py:109-114: ``shuffle=True, drop_last=True``) over a ``TrainingSet``: iteration yields
    ``data.Batch(pos, reflectance, y, sf, batch, ptr)`` on the device with ``num_graphs`` (and ``nonfinite`` [B] int32, the rows of
    each voxel with a non-finite value - passed through, as the reference's training set passes them) - what ``train.Net.forward`` and
    ``loss.Poly1FocalLoss`` consume.

    ``augmentation=True`` applies ``draw_plan``'s decisions of the epoch in ``mode`` ("train", or "test": no perturbation, as the
    reference's test loader); False keeps every reflectance and rotates nothing.  Everything random is a function of ``(seed, epoch)``:
    the order of the voxels, the plan and the reflectance noise (keyed by voxel and point, so it does not depend on the batching) - two
    feeds with the same ``(seed, epoch)`` yield the same bits; ``set_epoch(e)`` selects the epoch (it does not advance by itself).
    Per epoch one plan upload; per batch one small upload (``ids`` and ``out_ptr`` in one buffer) and one ``p2w_train_feed`` call;
    nothing waits for the device."""

    def __init__(self, tset: TrainingSet, batch_size: int, shuffle: bool = True, drop_last: bool = True, augmentation: bool = False,
                 mode: str = "train", seed: int = 0):
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size}")
        if mode not in ("train", "test"):
            raise ValueError(f"mode must be 'train' or 'test', got {mode!r}")
        self.set, self.batch_size, self.shuffle, self.drop_last = tset, int(batch_size), bool(shuffle), bool(drop_last)
        self.augmentation, self.mode, self.seed, self.epoch = bool(augmentation), mode, int(seed), 0

    def __len__(self):
        V = len(self.set)
        return V // self.batch_size if self.drop_last else -(-V // self.batch_size)

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def order(self):
        """The epoch's voxel order (numpy int64 [V])."""
        V = len(self.set)
        if not self.shuffle:
            return np.arange(V, dtype=np.int64)
        g = torch.Generator().manual_seed(_seed_of(self.seed, self.epoch, "order"))
        return torch.randperm(V, generator=g).numpy()

    def plan(self):
        """The epoch's plan records (host)."""
        if not self.augmentation:
            return identity_plan(len(self.set))
        return draw_plan(len(self.set), self.mode, torch.Generator().manual_seed(_seed_of(self.seed, self.epoch, "plan")))

    def batches(self):
        order, bs = self.order(), self.batch_size
        return [order[i * bs:(i + 1) * bs] for i in range(len(self))]

    def batch(self, ids, plan, epoch=None):
        """The batch of the voxels ``ids`` (host integers, distinct) under the device plan ``plan``: one upload, one kernel call."""
        tset = self.set
        dev = tset.device
        ids = np.asarray(ids, dtype=np.int64)
        B = len(ids)
        host = np.zeros(B + 1 + (B + 1) // 2, dtype=np.int64)              # out_ptr [B + 1], then ids as int32 pairs: one upload
        np.cumsum(tset.lengths[ids], out=host[1:B + 1])
        host[B + 1:].view(np.int32)[:B] = ids
        n = int(host[B])
        up = torch.from_numpy(host).to(dev, non_blocking=True)
        ptr = up[:B + 1]
        pos, refl, y, batch, sf, nonfinite = train_feed(tset, up[B + 1:].view(torch.int32)[:B], ptr, n, plan, self.seed,
                                                        self.epoch if epoch is None else epoch)
        out = Batch(pos=pos, reflectance=refl, y=y, sf=sf, batch=batch, ptr=ptr, nonfinite=nonfinite)
        out.num_graphs = B
        return out

    def iterate(self, start: int = 0):
        """The epoch's batches from batch ``start`` on (``0 <= start <= len(self)``; ``len(self)`` yields nothing): what a full
        iteration yields behind its first ``start`` batches, bit for bit, without building those - a batch is a function of the epoch's
        order and plan alone.  This is how a resumed run re-enters an epoch."""
        start = int(start)
        if not 0 <= start <= len(self):
            raise ValueError(f"start must lie in [0, {len(self)}], got {start}")
        epoch = self.epoch
        plan = plan_to_device(self.plan(), self.set.device)
        for ids in self.batches()[start:]:
            yield self.batch(ids, plan, epoch)

    def __iter__(self):
        return self.iterate(0)
