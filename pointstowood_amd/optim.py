"""``ClipAdamW``: the optimiser step of the training loop as one fused operator (``p2w_clip_adamw``, ``csrc/p2w_optim.hip``).

What ``trainer.finish_step`` composes from ``scaler.unscale_``, ``clip_grad_norm_(max_norm)``, ``scaler.step(AdamW)`` and
``scaler.update()`` runs here as ``2 * ceil(T / 32) + 1`` launches over the T tensors that have a gradient: the global norm in fp64, one
finalising workgroup that decides skip-or-apply, clips, moves the loss scale by ``GradScaler``'s law and forms the step's scalars, and
the update.  The decision stays on the device: ``step()`` reads nothing back, and ``read()`` is the one device-to-host copy, meant for
the epoch line.  The fp32 operation order is the one ``include/p2w.h`` documents, so the parameter bits are a function of the inputs
alone - they do not depend on which multi-tensor implementation the installed torch would pick.  The roundings differ from torch's
AdamW (which divides by the bias correction where this multiplies by its reciprocal, for one); the function is the same.

Out of scope: more than one parameter group, ``amsgrad``, ``maximize``, 16-bit parameters or moments, graph capture.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import OptimHyper, OptimState, OptimTensor

_WORDS = C.sizeof(OptimState) // 4                              # the record as fp32 words: 20
_SCALE_WORD = OptimState.scale.offset // 4


class ClipAdamW(torch.optim.Optimizer):
    """AdamW (``amsgrad=False``, ``maximize=False``) behind a clip of the global gradient norm to ``max_norm`` and a dynamic loss scale.

    ``loss_scale`` is the initial scale (``GradScaler``'s ``init_scale``; the reference trains with 512); ``None`` means no scaling: the
    scale is 1 and stays 1, and a step whose gradients are not finite is still skipped and counted.  One parameter group; ``lr`` and
    ``betas`` are read from it at every step, so ``OneCycleLR`` (which cycles ``betas[0]`` with ``lr``) and
    ``trainer.CosineAnnealingWarmupRestarts`` work on it unchanged.  Parameters are contiguous fp32 CUDA tensors on one device.
    Every hyper-parameter, ``scaling`` (whether there is a loss scale) among them, lives in the group and travels with ``state_dict()``.
    ``state[p]`` holds ``exp_avg`` and ``exp_avg_sq``, zeros from the first step that sees a gradient of ``p``; the step count lives on
    the device (``read()["t"]``), because only the device knows whether a step counted.  A parameter whose ``.grad`` is ``None`` is
    left out of that step (no decay either, as in torch).

        loss = ...
        optimizer.zero_grad()
        optimizer.scale(loss).backward()
        optimizer.step()
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1.0, loss_scale=512.0,
                 growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= max_norm < float("inf"):
            raise ValueError(f"Invalid max_norm: {max_norm}")
        if loss_scale is not None and not 0.0 < loss_scale < float("inf"):
            raise ValueError(f"Invalid loss_scale: {loss_scale}")
        if not 1.0 < growth_factor < float("inf") or not 0.0 < backoff_factor < 1.0 or int(growth_interval) < 1:
            raise ValueError("the growth factor must be above 1, the backoff factor inside (0, 1) and the growth interval at least 1")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm, growth_factor=growth_factor,
                        backoff_factor=backoff_factor, growth_interval=int(growth_interval), scaling=loss_scale is not None)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"ClipAdamW takes one parameter group, not {len(self.param_groups)}")
        ps = self.param_groups[0]["params"]
        if len(ps) > _lib.OPTIM_MAX_TENSORS:
            raise ValueError(f"ClipAdamW takes at most {_lib.OPTIM_MAX_TENSORS} parameters, not {len(ps)}")
        for p in ps:
            if not p.is_cuda:
                raise ValueError("ClipAdamW needs parameters on an MI355X (cuda) device; there is no CPU fallback")
            if p.dtype != torch.float32:
                raise TypeError(f"ClipAdamW needs float32 parameters, not {p.dtype}")
            if not p.is_contiguous():
                raise ValueError("ClipAdamW needs contiguous parameters")
            if p.device != ps[0].device:
                raise ValueError("ClipAdamW needs every parameter on the same device")
        self.device = ps[0].device
        first = OptimState(scale=1.0 if loss_scale is None else float(loss_scale))
        self._record = torch.frombuffer(bytearray(bytes(first)), dtype=torch.float32).to(self.device)
        self._ws = None

    def scale(self, loss):
        """``loss * scale`` with the scale read on the device; ``loss`` itself without scaling."""
        return loss * self._record[_SCALE_WORD] if self.param_groups[0]["scaling"] else loss

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        rows = []
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or g.is_sparse:
                raise TypeError("ClipAdamW needs dense float32 gradients")
            st = self.state[p]
            if not st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            rows.append((p, g if g.is_contiguous() else g.contiguous(), st["exp_avg"], st["exp_avg_sq"]))
        T = len(rows)
        if T == 0:
            return loss
        table = (OptimTensor * T)()
        numel = (C.c_int64 * T)()
        for k, (p, g, m, v) in enumerate(rows):
            e = table[k]
            e.p, e.g, e.m, e.v, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            numel[k] = e.n
        hyper = OptimHyper(lr=group["lr"], beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"],
                           weight_decay=group["weight_decay"], max_norm=group["max_norm"], growth_factor=group["growth_factor"],
                           backoff_factor=group["backoff_factor"], growth_interval=group["growth_interval"], scaling=int(group["scaling"]))
        L = _lib.lib()
        with torch.cuda.device(self.device):
            need = int(L.p2w_clip_adamw_ws_size(numel, T))
            if need == 0:
                raise RuntimeError("p2w_clip_adamw_ws_size failed")
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.check(L.p2w_clip_adamw(table, T, C.byref(hyper), _lib.ptr(self._record), _lib.ptr(self._ws), self._ws.numel(),
                                        _lib.stream()), "p2w_clip_adamw")
        return loss

    def read(self):
        """The device record as a dict (``include/p2w.h`` ``p2w_optim_state``): ``sumsq``, ``norm``, ``coef``, ``inv_scale``, ``scale``,
        ``found_inf``, ``growth_tracker``, ``t``, ``skipped`` and the seven scalars of the last applied step.  One device-to-host copy."""
        rec = OptimState.from_buffer_copy(self._record.cpu().numpy().tobytes())
        return {name: getattr(rec, name) for name, _ in OptimState._fields_ if name != "reserved"}

    def state_dict(self):
        sd = super().state_dict()
        sd["record"] = self._record.clone()
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict({"state": state_dict["state"], "param_groups": state_dict["param_groups"]})
        self._record.copy_(state_dict["record"].to(torch.float32).reshape(_WORDS))
