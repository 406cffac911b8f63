"""The loss and the per-batch scores of the reference's training step (``pointstowood/src/trainer.py:174-215``) on the GPU.

* ``Poly1FocalLoss``  - the reference's criterion (``pointstowood/src/loss.py``), constructor and ``forward`` signature included, over
                        ``p2w_poly1_focal`` (``csrc/p2w_loss.hip``): one kernel reads every logit and label once and leaves the
                        per-element loss, its derivative and one fp64 partial sum per 4096 elements; a second short launch adds the
                        partials in a fixed order.  The backward is one multiply by the incoming gradient.  The reduced values have
                        the same bits on every run.
* ``poly1_focal``     - the same as a function.
* ``EpochScores``     - the bookkeeping of trainer.py:194-215 and :256-267 without sklearn and without a host wait per batch: one
                        ``evaluate.confusion`` per batch into a device buffer, the epoch's figures from one device-to-host copy.

numpy and torch only; CUDA tensors only (there is no CPU fallback).
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import aligned16 as _aligned, check, lib, ptr as _p

_NOT_SET = float("nan")          # include/p2w.h: alpha / label_smoothing "not set" (the reference's None); a batch without a loss


def _flat32(t: torch.Tensor) -> torch.Tensor:
    return _aligned(t.detach().reshape(-1).to(torch.float32).contiguous())


def _finite(name, v):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {v}")
    return v


def _scalars(epsilon, gamma, alpha, label_smoothing, eps):
    """The five scalars as the doubles the ABI takes, checked: ``eps`` in (0, 0.5), ``gamma`` >= 0, everything finite."""
    epsilon, gamma, eps = _finite("epsilon", epsilon), _finite("gamma", gamma), float(eps)
    if gamma < 0:
        raise ValueError(f"gamma must be at least 0, got {gamma}")
    if not 0.0 < eps < 0.5:
        raise ValueError(f"eps must lie in (0, 0.5), got {eps}")
    alpha = _NOT_SET if alpha is None else _finite("alpha", alpha)
    label_smoothing = _NOT_SET if label_smoothing is None else _finite("label_smoothing", label_smoothing)
    return epsilon, gamma, alpha, label_smoothing, eps


def _launch(x, y, w, scalars, want_loss: bool, want_grad: bool, want_sum: bool):
    """(loss [n] float32, dloss [n] float32, sum [1] float64) of flat, aligned float32 CUDA tensors; what is not wanted is None and
    is neither allocated nor written.  Two launches on the current stream (one without the sum), no host wait."""
    n, dev = x.numel(), x.device
    loss = torch.empty(n, dtype=torch.float32, device=dev) if want_loss else None
    dloss = torch.empty(n, dtype=torch.float32, device=dev) if want_grad else None
    total = ws = None
    L = lib()
    if want_sum:
        total = torch.empty(1, dtype=torch.float64, device=dev)
        ws = torch.empty(int(L.p2w_poly1_focal_ws_bytes(n)), dtype=torch.uint8, device=dev)
    check(L.p2w_poly1_focal(_p(x), _p(y), _p(w), 0 if w is None else w.numel(), n, *scalars, _p(loss), _p(dloss), _p(total), _p(ws),
                            0 if ws is None else ws.numel(), _lib.stream()), "p2w_poly1_focal")
    return loss, dloss, total


def _reduced(total, n, reduction):
    """float32 of the fp64 sum, or of sum / n (NaN at n = 0, as ``torch.mean``), on the device."""
    if reduction == "mean":
        total = total / n
    return total.to(torch.float32).reshape(())


class _Poly1Focal(torch.autograd.Function):
    """Forward: the two launches, with ``dloss`` written beside the loss and saved.  Backward: one multiply."""

    @staticmethod
    def forward(ctx, logits, y, w, scalars, reduction):
        x = _flat32(logits)
        reduce = reduction in ("mean", "sum")
        loss, dloss, total = _launch(x, y, w, scalars, not reduce, True, reduce)
        ctx.save_for_backward(dloss)
        ctx.shape, ctx.dtype, ctx.reduction = logits.shape, logits.dtype, reduction
        return _reduced(total, x.numel(), reduction) if reduce else loss.view(logits.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        dloss, = ctx.saved_tensors
        g = grad_out.to(torch.float32)
        if ctx.reduction == "mean":
            g = g / dloss.numel()
        elif ctx.reduction != "sum":
            g = g.reshape(-1)
        return (g * dloss).view(ctx.shape).to(ctx.dtype), None, None, None, None


def poly1_focal(logits, labels, weight=None, epsilon: float = 0.1, gamma: float = 2.0, alpha=0.25, reduction: str = "none",
                label_smoothing=None, eps: float = 1e-6):
    """The reference's ``Poly1FocalLoss.forward`` without its second result: the per-element loss in the logits' shape for
    ``reduction="none"`` (and for any string other than ``"mean"`` / ``"sum"``, as in the reference), a float32 scalar otherwise.

    ``logits`` and ``labels`` are CUDA tensors of equal numel (the reference broadcasts; its training step passes equal shapes);
    ``weight`` has one element or as many as the logits.  Everything is computed in float32 whatever the dtypes and whatever
    ``torch.autocast`` says: the loss comes back in float32, the gradient in the logits' dtype.  The gradient flows to the logits
    only: labels or a weight that require one raise.  Without a gradient to track (``torch.no_grad()``, detached logits) the
    derivative is neither allocated nor written."""
    scalars = _scalars(epsilon, gamma, alpha, label_smoothing, eps)
    n = logits.numel()
    if labels.numel() != n:
        raise ValueError(f"logits have {n} elements, labels {labels.numel()}")
    if weight is not None and weight.numel() not in (1, n):
        raise ValueError(f"weight must have 1 or {n} elements, got {weight.numel()}")
    if torch.is_grad_enabled() and (labels.requires_grad or (weight is not None and weight.requires_grad)):
        raise ValueError("the gradient of Poly1FocalLoss flows to the logits only: labels and weight must not require one")
    _lib.require_cuda(logits, labels, weight)
    y = _flat32(labels)
    w = None if weight is None else _flat32(weight).to(logits.device)
    if torch.is_grad_enabled() and logits.requires_grad:
        return _Poly1Focal.apply(logits, y, w, scalars, reduction)
    reduce = reduction in ("mean", "sum")
    loss, _, total = _launch(_flat32(logits), y, w, scalars, not reduce, False, reduce)
    return _reduced(total, n, reduction) if reduce else loss.view(logits.shape)


class Poly1FocalLoss(nn.Module):
    """The reference's criterion with its constructor: ``forward(logits, labels, label_weights=None) -> (loss, gamma)``;
    ``label_weights`` is accepted and ignored, as there.  See ``poly1_focal``."""

    def __init__(self, epsilon: float = 0.1, gamma: float = 2.0, alpha: float = 0.25, reduction: str = "none", weight=None,
                 label_smoothing: float = None, eps: float = 1e-6):
        super().__init__()
        _scalars(epsilon, gamma, alpha, label_smoothing, eps)
        self.epsilon = epsilon
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.weight = weight
        self.label_smoothing = label_smoothing
        self.eps = eps

    def forward(self, logits, labels, label_weights=None):
        loss = poly1_focal(logits, labels, weight=self.weight, epsilon=self.epsilon, gamma=self.gamma, alpha=self.alpha,
                           reduction=self.reduction, label_smoothing=self.label_smoothing, eps=self.eps)
        return loss, self.gamma


class EpochScores:
    """The running scores of one epoch of the reference's training loop (trainer.py:194-215) and its history row (:256-267).

    ``add(logits, y, loss=None)`` counts ``sigmoid(logits) >= threshold`` against ``y`` with ``evaluate.confusion`` into the next
    2 x 2 slot of a device buffer and keeps the detached loss beside it; nothing in it waits for the device.  ``result()`` makes one
    device-to-host copy and returns the reference's figures: ``loss``, ``balanced_accuracy``, ``f1``, ``precision`` and ``recall``,
    each the sum over the batches of the per-batch value (``evaluate.binary_metrics`` of the batch's matrix) divided by the batch
    count - ``evaluate_voxels``' ``"mean"`` - with the per-batch ``matrices`` [B, 2, 2] and ``losses`` [B] (NaN where none was
    given; ``loss`` is then NaN too)."""

    def __init__(self, threshold: float = 0.5, capacity: int = 64):
        self.threshold = float(threshold)
        self._capacity = max(1, int(capacity))
        self._counts = self._loss = None          # [capacity, 5] int64: tn, fp, fn, tp, invalid; [capacity] float32
        self._batches = 0

    def __len__(self):
        return self._batches

    def _slot(self, dev):
        if self._counts is None:
            self._counts = torch.zeros((self._capacity, 5), dtype=torch.int64, device=dev)
            self._loss = torch.full((self._capacity,), _NOT_SET, dtype=torch.float32, device=dev)
        elif self._batches == self._capacity:     # full: double
            counts = torch.zeros((2 * self._capacity, 5), dtype=torch.int64, device=dev)
            loss = torch.full((2 * self._capacity,), _NOT_SET, dtype=torch.float32, device=dev)
            counts[:self._capacity] = self._counts
            loss[:self._capacity] = self._loss
            self._counts, self._loss, self._capacity = counts, loss, 2 * self._capacity
        return self._batches

    def add(self, logits, y, loss=None):
        from .evaluate import confusion
        _lib.require_cuda(logits, y, loss)
        with torch.no_grad():
            i = self._slot(logits.device)
            preds = torch.sigmoid(logits.detach().reshape(-1).to(torch.float32)) >= self.threshold
            confusion(y.detach(), preds, classes=2, strict=False, out=(self._counts[i, :4], None, self._counts[i, 4:]))
            if loss is not None:
                self._loss[i] = loss.detach().reshape(()).to(torch.float32)
        self._batches += 1

    def state(self):
        """What has been added so far, for a training state: the first ``len(self)`` rows of the counts ([B, 5] int64) and of the
        losses ([B] float32) as CPU tensors, the batch count, the threshold and the capacity.  One device-to-host copy each."""
        B = self._batches
        if self._counts is None:
            counts, losses = torch.zeros((0, 5), dtype=torch.int64), torch.zeros(0, dtype=torch.float32)
        else:
            counts, losses = self._counts[:B].cpu(), self._loss[:B].cpu()
        return {"counts": counts, "losses": losses, "batches": B, "threshold": self.threshold, "capacity": self._capacity}

    @classmethod
    def from_state(cls, state, device):
        """The object that ``state()`` described, its buffers on ``device``: the remaining ``add`` calls on it give ``result()`` the
        bits of the object that was never stored, ``matrices`` and ``losses`` included."""
        B = int(state["batches"])
        counts, losses = state["counts"], state["losses"]
        if tuple(counts.shape) != (B, 5) or tuple(losses.shape) != (B,) or counts.dtype != torch.int64 or losses.dtype != torch.float32:
            raise ValueError(f"a scores state of {B} batches needs int64 counts [{B}, 5] and float32 losses [{B}]")
        self = cls(threshold=state["threshold"], capacity=max(int(state["capacity"]), B))
        if B:
            self._slot(torch.device(device))
            self._counts[:B] = counts.to(device)
            self._loss[:B] = losses.to(device)
            self._batches = B
        return self

    def result(self):
        from .evaluate import _raise_invalid, binary_metrics
        B = self._batches
        if B == 0:
            nan = float("nan")
            return {"loss": nan, "balanced_accuracy": nan, "f1": nan, "precision": nan, "recall": nan,
                    "matrices": np.zeros((0, 2, 2), dtype=np.int64), "losses": np.zeros(0, dtype=np.float32)}
        # one copy: the counts (below 2^53: exact in float64) and the losses side by side
        host = torch.cat([self._counts[:B].to(torch.float64), self._loss[:B].to(torch.float64)[:, None]], dim=1).cpu().numpy()
        _raise_invalid(host[:, 4].astype(np.int64), "batch")
        matrices = host[:, :4].astype(np.int64).reshape(B, 2, 2)
        losses = host[:, 5].astype(np.float32)
        rows = [binary_metrics(m) for m in matrices]
        out = {}
        for k in ("balanced_accuracy", "f1", "precision", "recall"):
            total = 0.0
            for r in rows:
                total += r[k]
            out[k] = total / B
        total = 0.0
        for v in losses:
            total += float(v)
        return {"loss": total / B, **out, "matrices": matrices, "losses": losses}
