"""The reference's training loop (``pointstowood/src/trainer.py:96-320`` ``SemanticTraining``) over this package's parts:
``train.Net``, two ``feed.TrainingFeed`` s over device-resident ``feed.TrainingSet`` s, ``loss.Poly1FocalLoss`` and ``loss.EpochScores``.

Kept from the reference: ``Net(num_classes=1)``; ``shuffle=True, drop_last=True`` loaders, the held-out one in ``mode="test"`` with
``batch_size // 2`` voxels; ``Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)``; autocast,
``GradScaler(init_scale=512)``, ``clip_grad_norm_(1.0)``; AdamW with ``OneCycleLR`` (``--tune``: the cosine schedule with warm restarts)
stepped once per epoch; the history rows and their column order (7 columns, 11 with ``--test``) written with ``np.savetxt`` after every
epoch; ``{'model_state_dict': ...}`` checkpoints at ``args.checkpoints``; the ``ba-`` / ``f1-`` / ``precision-`` best-model files under
its epoch conditions; the final model.

Deviations (route A-train): no per-step ``deepcopy(state_dict)`` with a try / except rollback (``GradScaler`` already
skips a step with non-finite gradients); no ``set_detect_anomaly``; no ``.item()`` per batch - ``EpochScores`` reads the device once
per epoch; and the early-stop counter PERSISTS across epochs: the reference resets it to 0 at every epoch, so its ``>= 10`` can never
fire - what is built is the intent its message documents (training accuracy decreased for 10 consecutive epochs).

``args.amp`` (``train.py --amp``, ``"fp16"`` when absent) chooses the autocast dtype.  ``"fp16"`` is the loop above.  ``"bf16"`` runs
autocast in bfloat16, which has fp32's exponent: the scaler is built disabled, so no loss scale exists and no step is lost to one;
the norm that ``clip_grad_norm_`` returns is read once per step and a step whose norm is not finite is skipped and counted
(``finish_step``), the count printed with the epoch line.  Parameters, history layout and checkpoints are the same in both modes.

``args.fused_step`` (``train.py --fused_step``, off when absent) replaces ``finish_step`` and both optimisers by ``optim.ClipAdamW``:
unscale, clip, AdamW and the loss-scale law as one fused operator that decides skip-or-apply on the device (loss scale 512 under
``"fp16"``, none under ``"bf16"``).  The step then reads nothing back in either mode; the skipped count comes with the epoch's scores.

``args.state_every``, ``args.stop_at`` and ``args.resume`` (``train.py --state_every / --stop_at / --resume``, all absent: the loop
above) stop a run after any step and continue it with the bits of the run that never stopped: ``save_state`` / ``load_state`` /
``restore_state`` carry everything that moves (DESIGN.md lists it), ``request_stop`` and ``stop_handlers`` end a run behind the step in
flight, ``fingerprint_mismatch`` refuses a resume that could not be exact.
"""
from __future__ import annotations

import contextlib
import hashlib
import math
import os
import signal
from collections import OrderedDict

import numpy as np
import torch

from . import train as _train
from .feed import TrainingFeed, TrainingSet
from .loss import EpochScores, Poly1FocalLoss


class CosineAnnealingWarmupRestarts:
    """Cosine annealing with a linear warm-up and warm restarts, from the schedule's definition (the reference takes a third-party
    class of this name; only its ``step()``-without-argument path is used there and provided here).

    A cycle has ``cycle_steps`` steps (``first_cycle_steps`` at first; after a cycle ``int((cycle_steps - warmup_steps) * cycle_mult) +
    warmup_steps``).  At step t of a cycle the rate is ``min_lr + (max_lr - min_lr) * t / warmup_steps`` for ``t < warmup_steps`` and
    ``min_lr + (max_lr - min_lr) * (1 + cos(pi * (t - warmup_steps) / (cycle_steps - warmup_steps))) / 2`` after; cycle c's ``max_lr`` is
    ``max_lr * gamma ** c``.  Construction sets every group's rate to ``min_lr`` and then takes step 0 (the rate stays ``min_lr``)."""

    def __init__(self, optimizer, first_cycle_steps: int, cycle_mult: float = 1.0, max_lr: float = 0.1, min_lr: float = 0.001,
                 warmup_steps: int = 0, gamma: float = 1.0):
        if not warmup_steps < first_cycle_steps:
            raise ValueError(f"warmup_steps ({warmup_steps}) must be below first_cycle_steps ({first_cycle_steps})")
        self.optimizer = optimizer
        self.cycle_mult, self.base_max_lr, self.min_lr, self.warmup_steps, self.gamma = cycle_mult, max_lr, min_lr, warmup_steps, gamma
        self.cycle_steps, self.cycle, self.t = first_cycle_steps, 0, -1
        self.step()

    def rate(self):
        lo, hi = self.min_lr, self.base_max_lr * self.gamma ** self.cycle
        if self.t < self.warmup_steps:
            return (hi - lo) * self.t / self.warmup_steps + lo
        return lo + (hi - lo) * (1 + math.cos(math.pi * (self.t - self.warmup_steps) / (self.cycle_steps - self.warmup_steps))) / 2

    def step(self):
        self.t += 1
        if self.t >= self.cycle_steps:
            self.cycle += 1
            self.t -= self.cycle_steps
            self.cycle_steps = int((self.cycle_steps - self.warmup_steps) * self.cycle_mult) + self.warmup_steps
        lr = self.rate()
        for group in self.optimizer.param_groups:
            group["lr"] = lr

    def state_dict(self):
        """What moves: the cycle, its length and the step inside it.  The rate of the groups travels with the optimiser's state."""
        return {"cycle": self.cycle, "cycle_steps": self.cycle_steps, "t": self.t}

    def load_state_dict(self, state):
        self.cycle, self.cycle_steps, self.t = int(state["cycle"]), int(state["cycle_steps"]), int(state["t"])


def load_checkpoint(model, path, device):
    """trainer.py:67-75: ``model_state_dict`` with ``module.`` prefixes stripped, strict."""
    checkpoint = torch.load(path, map_location=device)
    sd = OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in checkpoint["model_state_dict"].items())
    model.load_state_dict(sd)
    return model


def _save(model, path):
    torch.save({"model_state_dict": model.state_dict()}, path)


def _save_best(model, stat, best, path):
    if stat > best:
        best = stat
        _save(model, path)
        print("Saving ", path)
    return best


AMP_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def finish_step(model, optimizer, scaler, amp="fp16"):
    """What the loop does with the gradients of one batch, behind ``scaler.scale(loss).backward()``: unscale, clip to norm 1, step.
    -> 1 where the step was skipped here, else 0.  ``"fp16"``: the enabled scaler finds non-finite gradients itself (its one host
    read per step, inside ``scaler.step``) and skips without saying so: 0.  ``"bf16"``: the scaler is disabled and finds nothing, so
    the clip's norm is read - the step's one host read - and, where it is not finite, ``optimizer.step()`` is not called: no
    parameter and no optimizer state moves."""
    scaler.unscale_(optimizer)
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    if amp == "bf16" and not math.isfinite(float(norm)):
        scaler.update()
        return 1
    scaler.step(optimizer)
    scaler.update()
    return 0


def set_fused_bn_max(model, on=True):
    """``fused_bn_max = on`` on every ``ops.PointNetConv`` instance of ``model`` - on the instances, so the class default (False) and
    every other model stay as they are.  -> the number of layers set."""
    n = 0
    for m in model.modules():
        if isinstance(m, _train.ops.PointNetConv):
            m.fused_bn_max = bool(on)
            n += 1
    return n


# ---- the training state: everything that moves during a run, so that a run can stop after any step and go on in another process ----

STATE_FORMAT = 1
BEST_KEYS = ("best_ba_train", "best_f1_train", "best_ba_test", "best_f1_test", "best_precision_test")
_ABSENT = "<absent>"
_stop_requested = False


def request_stop():
    """Asks the loop to stop: after the step in flight it writes the state and returns, as for ``--stop_at`` at that position."""
    global _stop_requested
    _stop_requested = True


def stop_requested():
    return _stop_requested


def clear_stop():
    global _stop_requested
    _stop_requested = False


@contextlib.contextmanager
def stop_handlers():
    """While open, SIGTERM and SIGINT call ``request_stop()`` - a job scheduler's signal then ends the run cleanly behind the step in
    flight; on exit the previous handlers are back.  (Signal handlers belong to the main thread.)"""
    def handler(signum, frame):
        request_stop()
    previous = {s: signal.signal(s, handler) for s in (signal.SIGTERM, signal.SIGINT)}
    try:
        yield
    finally:
        for s, h in previous.items():
            signal.signal(s, h)


def set_fingerprint(tset):
    """(voxel count, SHA-256 of the ``lengths`` array) of a ``TrainingSet``: what a state remembers of a data set."""
    return len(tset), hashlib.sha256(np.ascontiguousarray(tset.lengths, dtype=np.int64).tobytes()).hexdigest()


def fingerprint(args, train_set, test_set=None):
    """What a resumed run must share with the run that wrote the state for its bits to be the uninterrupted run's: a flat dict."""
    fp = {"format": STATE_FORMAT, "seed": int(getattr(args, "seed", 141190)), "batch_size": int(args.batch_size),
          "C": int(getattr(args, "C", 32)), "amp": str(getattr(args, "amp", "fp16")), "tune": bool(args.tune),
          "num_epochs": int(args.num_epochs), "augmentation": bool(args.augmentation), "test": bool(args.test),
          "fused_step": bool(getattr(args, "fused_step", False)), "device_sample": bool(getattr(args, "device_sample", False)),
          "fused_bn_max": bool(getattr(args, "fused_bn_max", False))}
    fp["train_voxels"], fp["train_lengths_sha256"] = set_fingerprint(train_set)
    if test_set is not None:
        fp["test_voxels"], fp["test_lengths_sha256"] = set_fingerprint(test_set)
    return fp


def fingerprint_mismatch(saved, current):
    """-> [(field, saved value, current value)] of every field in which the two fingerprints differ, in sorted field order; a field
    that one of them lacks counts as differing, its value there given as ``"<absent>"``.  Empty: the resume can be exact."""
    out = []
    for k in sorted(set(saved) | set(current)):
        a, b = saved.get(k, _ABSENT), current.get(k, _ABSENT)
        if type(a) is not type(b) or a != b:
            out.append((k, a, b))
    return out


def save_state(path, *, epoch, step, model, optimizer, scaler, scheduler, history, best, consec_decreases, skipped, scores, sampler,
               fingerprint):
    """The whole training state at the position (``epoch``, ``step`` finished steps of it) into ``path``: written to ``path + ".tmp"``
    and moved into place, so a kill during the write leaves the previous state as it was.  Tensors, numbers, strings, lists and
    dicts only - ``torch.load(weights_only=True)`` reads it.  ``history``: the rows so far ([epochs done, columns], stored as
    float64); ``best``: the five thresholds (``BEST_KEYS``); ``skipped``: the open epoch's running count on the plain route,
    ``skipped_before`` under ``fused_step``; ``scores``: the open epoch's ``EpochScores``; ``scaler`` and ``sampler`` may be None.
    Reads the process-wide generators without advancing them; waits for the device."""
    device = next(model.parameters()).device
    state = {
        "format": STATE_FORMAT,
        "fingerprint": dict(fingerprint),
        "epoch": int(epoch),
        "step": int(step),
        "model": model.state_dict(),
        "optimizer": optimizer.state_dict(),
        "scaler": {} if scaler is None else scaler.state_dict(),
        "scheduler": scheduler.state_dict(),
        "history": torch.from_numpy(np.array(history, dtype=np.float64, ndmin=2)),
        "best": {k: float(best[k]) for k in BEST_KEYS},
        "consec_decreases": int(consec_decreases),
        "skipped": int(skipped),
        "scores": scores.state(),
        "sampler": None if sampler is None else sampler.state_dict(),
        "rng": {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(device)},
    }
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def load_state(path, device):
    """The dict that ``save_state`` wrote, read with ``weights_only=True``: the model's tensors, the optimiser's moments and its
    ``record`` on ``device``; what lives on the host during a run (AdamW's step counts, the scores, the history, the generator
    states) stays there."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if state.get("format") != STATE_FORMAT:
        raise ValueError(f"{path}: state format {state.get('format')!r}, this build reads format {STATE_FORMAT}")
    for k, v in state["model"].items():
        state["model"][k] = v.to(device)
    opt = state["optimizer"]
    for st in opt["state"].values():
        for k, v in st.items():
            if k != "step" and torch.is_tensor(v):
                st[k] = v.to(device)
    if "record" in opt:
        opt["record"] = opt["record"].to(device)
    return state


def restore_state(state, *, model, optimizer, scaler, scheduler, sampler):
    """Puts the pieces of a loaded state back into freshly built objects: the model, the optimiser BEFORE the scheduler (so the
    group's ``lr`` and ``betas`` are the saved ones), the scaler (an empty dict - a disabled scaler, or ``fused_step`` - is passed
    over), the sampler, and last of all the two generator states: nothing that draws from the CPU generator may run between this
    call and the first step."""
    model.load_state_dict(state["model"])
    optimizer.load_state_dict(state["optimizer"])
    if scaler is not None and state.get("scaler"):
        scaler.load_state_dict(state["scaler"])
    scheduler.load_state_dict(state["scheduler"])
    if sampler is not None:
        sampler.load_state_dict(state["sampler"])
    torch.cuda.set_rng_state(state["rng"]["cuda"], next(model.parameters()).device)
    torch.set_rng_state(state["rng"]["cpu"])


def SemanticTraining(args):
    """``args``: the namespace of ``train.py`` - ``wdir``, ``model``, ``trfile`` / ``tefile`` (voxel directories), ``batch_size``,
    ``num_epochs``, ``checkpoints``, ``augmentation``, ``test``, ``tune``, ``stop_early``, ``wandb``, ``seed``, ``device_sample`` (absent
    or False: the reference's CPU draw of the training sample); ``args.C`` (not on the command line) is the network's width, 32 when
    absent; ``args.amp``, ``"fp16"`` (absent: the same) or ``"bf16"``; ``args.fused_bn_max`` (``train.py --fused_bn_max``; absent or
    False: nothing changes): every ``ops.PointNetConv`` of the model runs ReLU, BatchNorm1d and the segment max behind its layer-2
    GEMM as ``ops.relu_bn_max``, on the GEMM's float16 / bfloat16 output as it is - the same function as the three statements, other
    roundings, the same bits on every run, the same ``state_dict``; ``args.fused_step`` (``train.py --fused_step``; absent or False:
    nothing changes): the optimiser is ``optim.ClipAdamW`` with the same ``lr`` and ``weight_decay`` and the loop is
    ``optimizer.scale(loss).backward(); optimizer.step()`` - same history layout, same checkpoints.  Returns the history array.

    The training state (all absent: nothing changes).  ``args.state_every`` (``train.py --state_every N``): ``save_state`` into
    ``model/<stem>_state.pth`` at the end of every epoch and, for N > 0, behind every N-th step of an epoch.  ``args.stop_at = (E, S)``
    (``--stop_at E:S``): once S steps of epoch E are done the state is written and the history so far returned (S = the steps of an
    epoch: behind that epoch's held-out pass and end-of-epoch work, as (E + 1, 0)); ``request_stop()`` does the same at the position
    the loop is at.  ``args.resume`` (``--resume``; implies ``state_every = 0``): where the state file exists the run goes on from it -
    the model file is neither loaded nor rewritten - and produces the bits of the run that was never stopped; a state whose
    fingerprint differs from this run's raises ``ValueError`` before anything is written; where it does not exist the run starts as
    usual."""
    if not torch.cuda.is_available():
        raise RuntimeError("SemanticTraining needs an MI355X (cuda) device; there is no CPU fallback")
    device = torch.device("cuda")
    amp = getattr(args, "amp", "fp16")
    if amp not in AMP_DTYPES:
        raise ValueError(f"amp is 'fp16' or 'bf16', not {amp!r}")
    seed = int(getattr(args, "seed", 141190))                   # the reference's module-level torch.manual_seed(141190)
    torch.manual_seed(seed)
    wandb = None
    if args.wandb:
        try:
            import wandb
        except ImportError as e:
            raise SystemExit("--wandb needs the wandb module, which is not installed here; run without --wandb") from e
        wandb.init(project="PointsToWood", config={"architecture": "pointnet++", "dataset": "high resolution 2 & 4 m voxels",
                                                   "epochs": args.num_epochs})

    model = _train.Net(num_classes=1, C=int(getattr(args, "C", 32))).to(device)
    print("Model contains", sum(p.numel() for p in model.parameters()), " parameters")
    if getattr(args, "device_sample", False):                   # the training samples drawn on the GPU (train.DeviceSampler)
        model.sampler = _train.DeviceSampler(seed)
    if getattr(args, "fused_bn_max", False):                    # relu_bn_max behind every PointNetConv's layer-2 GEMM
        set_fused_bn_max(model)

    train_feed = TrainingFeed(TrainingSet(args.trfile, device), args.batch_size, shuffle=True, drop_last=True,
                              augmentation=args.augmentation, mode="train", seed=seed)
    test_feed = None
    if args.test:
        test_feed = TrainingFeed(TrainingSet(args.tefile, device), int(args.batch_size / 2), shuffle=True, drop_last=True,
                                 augmentation=args.augmentation, mode="test", seed=seed + 1)
    for name, f in (("training", train_feed), ("test", test_feed)):
        if f is not None and len(f) == 0:
            raise ValueError(f"the {name} set has {len(f.set)} voxels: fewer than one batch of {f.batch_size}")

    criterion = Poly1FocalLoss(reduction="mean", gamma=2.0, alpha=None, label_smoothing=0.1)
    params = [p for p in model.parameters() if p.requires_grad]
    fused_step = bool(getattr(args, "fused_step", False))
    if fused_step:
        from .optim import ClipAdamW

        def make_optimizer(params, lr, weight_decay):
            return ClipAdamW(params, lr=lr, weight_decay=weight_decay, max_norm=1.0, loss_scale=512.0 if amp == "fp16" else None)
    else:
        make_optimizer = torch.optim.AdamW
    if args.tune:
        optimizer = make_optimizer(params, lr=1e-6, weight_decay=1e-2)
        lr_scheduler = CosineAnnealingWarmupRestarts(optimizer, first_cycle_steps=args.num_epochs // 5, cycle_mult=1.0, max_lr=1e-6,
                                                     min_lr=1e-8, warmup_steps=5, gamma=0.5)
    else:
        optimizer = make_optimizer(params, lr=1e-4, weight_decay=1e-2)
        lr_scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=1e-4, total_steps=args.num_epochs, pct_start=0.05,
                                                           anneal_strategy="cos", div_factor=100)

    model_dir = os.path.join(args.wdir, "model")
    model_path = os.path.join(model_dir, args.model)
    stem = os.path.splitext(args.model)[0]
    steps = len(train_feed)

    # the training state (all opt-in: with none of the three arguments nothing below saves, stops or reads a state)
    state_path = os.path.join(model_dir, stem + "_state.pth")
    state_every = getattr(args, "state_every", None)
    stop_at = getattr(args, "stop_at", None)
    resume = bool(getattr(args, "resume", False))
    if resume and state_every is None:
        state_every = 0
    if state_every is not None and int(state_every) < 0:
        raise ValueError(f"state_every must be at least 0, got {state_every}")
    if stop_at is not None:
        stop_at = (int(stop_at[0]), int(stop_at[1]))
        if stop_at[0] < 1 or not 0 <= stop_at[1] <= steps:
            raise ValueError(f"stop_at = (epoch >= 1, 0 <= step <= {steps} steps of an epoch), got {stop_at}")
        if stop_at[1] == steps:                                 # behind an epoch's last step: behind its end-of-epoch work
            stop_at = (stop_at[0] + 1, 0)
    run_fingerprint = fingerprint(args, train_feed.set, None if test_feed is None else test_feed.set)
    state = None
    if resume and os.path.isfile(state_path):
        state = load_state(state_path, device)
        differing = fingerprint_mismatch(state["fingerprint"], run_fingerprint)
        if differing:                                           # refused before anything is written
            raise ValueError(f"{state_path} cannot be resumed exactly by this run; differing fields (saved state, this run): "
                             + "; ".join(f"{k}: {a!r}, {b!r}" for k, a, b in differing))

    os.makedirs(model_dir, exist_ok=True)
    if state is not None:
        print(f"Resuming at epoch {state['epoch']}, step {state['step']}")       # the state wins: the model file is not touched
    elif os.path.isfile(model_path):
        print("Loading model")
        try:
            load_checkpoint(model, model_path, device)
        except KeyError:
            print("Failed to load, creating new...")
            torch.save(model.state_dict(), model_path)
    else:
        print("\nModel not found, creating new file...")
        torch.save(model.state_dict(), model_path)

    def log_history(history):
        try:
            np.savetxt(os.path.join(model_dir, stem + "_history.csv"), history)
            print("Saved training history successfully.")
        except OSError:
            np.savetxt(os.path.join(model_dir, stem + "_history_backup.csv"), history)

    best_ba_train = best_f1_train = best_ba_test = best_f1_test = best_precision_test = 0.0
    scaler = torch.amp.GradScaler("cuda", init_scale=512, enabled=amp == "fp16")
    history = None
    consec_decreases = 0
    skipped_before = 0                                          # (fused_step) the device's count at the end of the last epoch
    start_epoch, start_step = 1, 0

    def save(epoch, step, scores, skipped):
        save_state(state_path, epoch=epoch, step=step, model=model, optimizer=optimizer, scaler=None if fused_step else scaler,
                   scheduler=lr_scheduler, history=np.zeros((0, 11 if args.test else 7)) if history is None else history,
                   best=dict(zip(BEST_KEYS, (best_ba_train, best_f1_train, best_ba_test, best_f1_test, best_precision_test))),
                   consec_decreases=consec_decreases, skipped=skipped_before if fused_step else skipped, scores=scores,
                   sampler=model.sampler, fingerprint=run_fingerprint)
        print(f"Saved the training state at epoch {epoch}, step {step}")

    def stops(epoch, step):
        """Whether the run ends at this position: ``stop_at``, or a stop request (which is cleared)."""
        if stop_requested():
            clear_stop()
            return True
        return stop_at == (epoch, step)

    if state is not None:
        start_epoch, start_step = state["epoch"], state["step"]
        history = state["history"].numpy() if state["history"].shape[0] else None
        best_ba_train, best_f1_train, best_ba_test, best_f1_test, best_precision_test = (state["best"][k] for k in BEST_KEYS)
        consec_decreases = state["consec_decreases"]
        if fused_step:
            skipped_before = state["skipped"]
        restore_state(state, model=model, optimizer=optimizer, scaler=None if fused_step else scaler, scheduler=lr_scheduler,
                      sampler=model.sampler)                    # ends with the generator states: nothing below draws before the step
    if stops(start_epoch, start_step):                          # a resumed run's state file already holds this position
        if state is None:
            save(start_epoch, start_step, EpochScores(capacity=steps), 0)
        return history

    for epoch in range(start_epoch, args.num_epochs + 1):
        model.train()
        print("\n=============================================================================================")
        print("EPOCH ", epoch)
        train_feed.set_epoch(epoch)
        if model.sampler is not None:
            model.sampler.set_epoch(epoch)
        first = start_step if epoch == start_epoch else 0       # a resumed epoch goes on behind its finished steps
        if first:
            if model.sampler is not None:
                model.sampler.step = first
            scores = EpochScores.from_state(state["scores"], device)
            skipped = 0 if fused_step else state["skipped"]
        else:
            scores = EpochScores(capacity=steps)
            skipped = 0
        step = first
        for data in train_feed.iterate(first):
            optimizer.zero_grad()
            with torch.autocast("cuda", dtype=AMP_DTYPES[amp]):
                outputs = model(data)
                loss, _ = criterion(outputs, data.y)
            if fused_step:
                optimizer.scale(loss).backward()
                optimizer.step()
            else:
                scaler.scale(loss).backward()
                skipped += finish_step(model, optimizer, scaler, amp)
            scores.add(outputs, data.y, loss)
            step += 1
            if step < steps:                                    # (behind the last step the epoch's end comes first)
                if stops(epoch, step):
                    save(epoch, step, scores, skipped)
                    return history
                if state_every and step % state_every == 0:
                    save(epoch, step, scores, skipped)
        lr_scheduler.step()
        tr = scores.result()                                    # the epoch's one device-to-host copy
        lr = optimizer.param_groups[0]["lr"]
        if fused_step:                                          # read with the scores: the steps this epoch skipped
            total = optimizer.read()["skipped"]
            skipped, skipped_before = total - skipped_before, total
        print(f"Train  Lr {lr:.3g}  Lo {tr['loss']:.5f}  Ac {tr['balanced_accuracy']:.3f}  Pr {tr['precision']:.3f}  "
              f"Re {tr['recall']:.3f}  F1 {tr['f1']:.3f}" + (f"  Skipped {skipped}" if amp == "bf16" or fused_step else ""))

        te = None
        if test_feed is not None:
            model.eval()
            test_feed.set_epoch(epoch)
            scores = EpochScores(capacity=len(test_feed))
            with torch.no_grad():
                for data in test_feed:
                    scores.add(model(data), data.y)
            te = scores.result()
            print(f"Test   Ac {te['balanced_accuracy']:.3f}  Pr {te['precision']:.3f}  Re {te['recall']:.3f}  F1 {te['f1']:.3f}")

        row = [epoch, lr, tr["loss"], tr["balanced_accuracy"], tr["f1"], tr["precision"], tr["recall"]]
        if te is not None:
            row += [te["balanced_accuracy"], te["f1"], te["precision"], te["recall"]]
        row = np.array([row], dtype=np.float64)
        history = row if history is None else np.vstack((history, row))
        log_history(history)

        if epoch in args.checkpoints:
            folder = os.path.join(args.wdir, "checkpoints")
            os.makedirs(folder, exist_ok=True)
            _save(model, os.path.join(folder, f"epoch_{epoch}.pth"))

        if args.stop_early and epoch > 10:
            consec_decreases = consec_decreases + 1 if history[-1, 3] < history[-2, 3] else 0
            if consec_decreases >= 10:
                print(f"\nStopping early at epoch {epoch} - training accuracy decreased for {consec_decreases} consecutive epochs")
                print(f"Best accuracy was {max(history[:, 3]):.4f} at epoch {np.argmax(history[:, 3]) + 1}")
                if state_every is not None:                     # the run is over: a resume of this state has nothing left to do
                    save(args.num_epochs + 1, 0, EpochScores(capacity=steps), 0)
                break

        base = os.path.basename(args.model)
        if epoch > int(args.num_epochs * 0.10) and not args.test:
            best_ba_train = _save_best(model, tr["balanced_accuracy"], best_ba_train, os.path.join(model_dir, "ba-" + base))
            best_f1_train = _save_best(model, tr["f1"], best_f1_train, os.path.join(model_dir, "f1-" + base))
        if args.test and epoch > int(args.num_epochs * 0.5):
            best_ba_test = _save_best(model, te["balanced_accuracy"], best_ba_test, os.path.join(model_dir, "ba-" + base))
            best_f1_test = _save_best(model, te["f1"], best_f1_test, os.path.join(model_dir, "f1-" + base))
            best_precision_test = _save_best(model, te["precision"], best_precision_test, os.path.join(model_dir, "precision-" + base))

        if epoch == args.num_epochs:
            print("Saving final GLOBAL model")
            _save(model, model_path)

        if wandb is not None:
            wandb.log({"Epoch": epoch, "Learning Rate": lr, "Loss": np.around(tr["loss"], 4),
                       "Accuracy": np.around(tr["balanced_accuracy"], 4), "Precision": np.around(tr["precision"], 4),
                       "Recall": np.around(tr["recall"], 4), "F1": np.around(tr["f1"], 4),
                       "Test F1": np.around(te["f1"], 4) if te is not None else 0.0,
                       "Test Accuracy": np.around(te["balanced_accuracy"], 4) if te is not None else 0.0})

        # the epoch is wholly finished: its state is the next epoch's position before its first step
        stop = stops(epoch + 1, 0)
        if state_every is not None or stop:
            save(epoch + 1, 0, EpochScores(capacity=steps), 0)
        if stop:
            break
    return history
