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
"""
from __future__ import annotations

import math
import os
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


def SemanticTraining(args):
    """``args``: the namespace of ``train.py`` - ``wdir``, ``model``, ``trfile`` / ``tefile`` (voxel directories), ``batch_size``,
    ``num_epochs``, ``checkpoints``, ``augmentation``, ``test``, ``tune``, ``stop_early``, ``wandb``, ``seed``, ``device_sample`` (absent
    or False: the reference's CPU draw of the training sample); ``args.C`` (not on the command line) is the network's width, 32 when
    absent; ``args.amp``, ``"fp16"`` (absent: the same) or ``"bf16"``; ``args.fused_bn_max`` (``train.py --fused_bn_max``; absent or
    False: nothing changes): every ``ops.PointNetConv`` of the model runs ReLU, BatchNorm1d and the segment max behind its layer-2
    GEMM as ``ops.relu_bn_max``, on the GEMM's float16 / bfloat16 output as it is - the same function as the three statements, other
    roundings, the same bits on every run, the same ``state_dict``; ``args.fused_step`` (``train.py --fused_step``; absent or False:
    nothing changes): the optimiser is ``optim.ClipAdamW`` with the same ``lr`` and ``weight_decay`` and the loop is
    ``optimizer.scale(loss).backward(); optimizer.step()`` - same history layout, same checkpoints.  Returns the history array."""
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
    os.makedirs(model_dir, exist_ok=True)
    model_path = os.path.join(model_dir, args.model)
    stem = os.path.splitext(args.model)[0]
    if os.path.isfile(model_path):
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

    for epoch in range(1, args.num_epochs + 1):
        model.train()
        print("\n=============================================================================================")
        print("EPOCH ", epoch)
        train_feed.set_epoch(epoch)
        if model.sampler is not None:
            model.sampler.set_epoch(epoch)
        scores = EpochScores(capacity=len(train_feed))
        skipped = 0
        for data in train_feed:
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
    return history
