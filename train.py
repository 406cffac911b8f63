#!/usr/bin/env python3
"""train.py - the training command line of the MI355X build, with the reference's flags (``pointstowood/train.py:60-76``).

    python train.py --wdir DIR [--preprocess] [--test] [--augmentation] --num_epochs 300 --batch_size 8 --model model.pth

``DIR`` holds what the reference keeps in its ``pointstowood`` folder: ``data/train/voxels/*.pt`` and ``data/test/voxels/*.pt`` (float32
``[n, >= 5]`` = x, y, z, reflectance, label, ...; written by ``--preprocess`` from ``data/train/*.ply`` and ``data/test/*.ply``),
``model/`` (the model, its ``_history.csv`` and the ``ba-`` / ``f1-`` / ``precision-`` best models) and ``checkpoints/``.  The reference
finds that folder by searching its own checkout's name in the working directory; here it is ``--wdir`` (default: the working
directory).  ``--seed`` seeds the initialisation, the network's training sample and the feed (default: the reference's 141190).

The loop is ``pointstowood_amd.trainer.SemanticTraining``: the whole set lives on the GPU, and every batch is gathered, augmented,
centred and collated there (``pointstowood_amd.feed``).  ``--fused_bn_max`` (default off) sets ``fused_bn_max`` on every
``ops.PointNetConv`` of the model: ReLU, training-mode BatchNorm and the segment max behind the layer-2 GEMM run as ``ops.relu_bn_max``,
which under ``--amp`` of either dtype reads the GEMM's 16-bit output and writes its gradient in that dtype.  ``--fused_step`` (default
off) runs unscale, clip, AdamW and the loss-scale law of every step as one fused operator (``pointstowood_amd.optim.ClipAdamW``).

A run can be cut into pieces: ``--state_every N`` writes the whole training state to ``model/<model>_state.pth`` at every epoch's end
(N > 0: and after every N-th step), ``--stop_at E:S`` writes it and exits once S steps of epoch E are done, and with either, or with
``--resume``, SIGTERM and SIGINT do the same after the step in flight.  ``--resume`` continues from that file where it exists - the
continued run produces the bits of the uninterrupted one - and starts as usual where it does not:

    python train.py --wdir DIR ... --resume --state_every 200        # the same line for every submission of a time-boxed job
"""
from __future__ import annotations

import argparse
import glob
import os
import shutil

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--device', type=str, default='cuda', help='Insert either "cuda" or "cpu" (only cuda is built: there is no CPU path)')
    p.add_argument('--num_procs', type=int, default=1, help='Number of cpu cores to use')
    p.add_argument('--num_epochs', default=2, type=int, metavar='N', help='number of total epochs to run')
    p.add_argument('--checkpoint_saves', default=1, type=int, metavar='N', help='number of times to save model')
    p.add_argument('--model', type=str, default='model.pth', help='Name of global model [e.g. model.pth]')
    p.add_argument('--resolution', type=float, default=0.01, help='Resolution to which point cloud is downsampled [m]')
    p.add_argument('--grid_size', type=float, nargs='+', default=[2.0, 4.0], help='Grid sizes for voxelization')
    p.add_argument('--min_pts', type=int, default=8192, help='Minimum number of points in voxel')
    p.add_argument('--max_pts', type=int, default=16384, help='Maximum number of points in voxel')
    p.add_argument('--batch_size', type=int, default=2, help='Batch size for cuda processing [Lower less memory usage]')
    p.add_argument('--augmentation', action='store_true', help="Perform data augmentation")
    p.add_argument('--preprocess', action='store_true', help="Preprocess point clouds into voxels")
    p.add_argument('--test', action='store_true', help="Perform model testing during training")
    p.add_argument('--tune', action='store_true', help="Tune model hyperparameters with lower learning rate schedule")
    p.add_argument('--stop_early', action='store_true', help="Break training run if training accuracy continually decreases")
    p.add_argument('--wandb', action='store_true', help="Use wandb for logging")
    p.add_argument('--verbose', action='store_true', help="print stuff")
    # extensions of this build
    p.add_argument('--wdir', type=str, default=os.getcwd(), help='working directory with data/, model/ and checkpoints/')
    p.add_argument('--seed', type=int, default=141190, help='seed of the initialisation, the sampling and the feed')
    p.add_argument('--device_sample', action='store_true',
                   help="Draw each level's training sample on the GPU: the reference's law (a uniform half of the rows) from another "
                        "random stream, a function of (seed, epoch, step, level), so a seeded run samples other points than without it")
    p.add_argument('--device_cap', action='store_true',
                   help="With --preprocess: cut voxels above --max_pts down on the GPU, all of a grid size in one operator call, "
                        "seeded with --seed: the reference's laws from another random stream, so other points are kept than without it")
    p.add_argument('--amp', choices=['fp16', 'bf16'], default='fp16',
                   help="autocast dtype: fp16 with GradScaler(512) (the reference's loop), or bf16 without a loss scale, where a step "
                        "whose gradient norm is not finite is skipped and counted")
    p.add_argument('--fused_bn_max', action='store_true',
                   help="Run ReLU, BatchNorm and the max behind every PointNetConv's layer-2 GEMM as one fused operator "
                        "(ops.relu_bn_max) that reads the GEMM's 16-bit output as it is: less memory traffic and a lower peak, "
                        "other roundings than the three statements")
    p.add_argument('--fused_step', action='store_true',
                   help="Run unscale, clip_grad_norm_(1.0), AdamW and the loss-scale update of every step as one fused operator "
                        "(optim.ClipAdamW): skip-or-apply is decided on the GPU and no step reads the device; a documented fp32 "
                        "operation order, other roundings than torch's AdamW; the skipped count is printed with every epoch")
    p.add_argument('--state_every', type=int, default=None, metavar='N',
                   help="Write the whole training state (model, optimiser, loss scale, schedule, history, best-model thresholds, "
                        "open epoch's scores, random generators) to model/<model>_state.pth at the end of every epoch and, for "
                        "N > 0, after every N-th step of an epoch; each save waits for the GPU once")
    p.add_argument('--stop_at', type=stop_position, default=None, metavar='E:S',
                   help="Write the training state and exit (status 0) once S steps of epoch E are done; S = 0: before the first step "
                        "of epoch E; S = the steps of an epoch: after that epoch's test pass and checkpoints")
    p.add_argument('--resume', action='store_true', default=None,
                   help="Continue from model/<model>_state.pth where it exists (else start as usual): the continued run produces "
                        "the bits of the uninterrupted one; implies --state_every 0; the old checkpoints are kept; a state written "
                        "with other flags, another seed, batch size, --num_epochs or data set is refused; not with --preprocess. "
                        "With any of the three flags SIGTERM and SIGINT stop the run after the step in flight, state written")
    return p


def stop_position(text):
    """``E:S`` -> (E, S): epoch E >= 1, S >= 0 finished steps of it."""
    try:
        epoch, step = (int(v) for v in text.split(':'))
    except ValueError:
        raise argparse.ArgumentTypeError(f"E:S (two integers) is needed, got {text!r}") from None
    if epoch < 1 or step < 0:
        raise argparse.ArgumentTypeError(f"an epoch from 1 and a step from 0 are needed, got {text!r}")
    return epoch, step


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.resume and args.preprocess:
        p.error("--resume continues a run on the voxels it was started on: it cannot be combined with --preprocess")
    return args


def training_columns(columns):
    """``preprocess_point_cloud_data`` of the reference's train.py (:36-49) over ``io.prepare_columns``: the label (a ``truth`` or
    ``label`` column, ``scalar_`` prefix or not) is kept and placed at column 4, behind x, y, z, reflectance - where the training set
    reads it.  -> (names, [n, cols] float32 array, had_reflectance)."""
    from pointstowood_amd import io as pio
    label = None
    rest = {}
    for name, v in columns.items():
        if name.lower().replace("scalar_", "") in ("truth", "label"):
            label = v
        else:
            rest[name] = v
    if label is None:
        raise SystemExit("no 'truth' or 'label' column: a training cloud needs one")
    cols, _, had = pio.prepare_columns(rest)
    names = list(cols)
    names.insert(4, "label")
    cols["label"] = label
    xyz = np.stack([np.asarray(cols[c], dtype=np.float64) for c in names[:3]], 1)
    xyz -= xyz.min(0)                                           # plot-local coordinates: fp32 keeps millimetres at any easting
    arr = np.concatenate([xyz] + [np.asarray(cols[c], dtype=np.float64)[:, None] for c in names[3:]], 1)
    return names, arr.astype(np.float32), had


def preprocess(files, out_dir, args):
    """Every PLY of ``files`` through the voxeliser into ``out_dir/voxel_<i>.pt`` (float32 [n, >= 5] CPU tensors)."""
    import torch
    from pointstowood_amd import io as pio
    from pointstowood_amd.preprocessing import DeviceCap, voxelise
    if os.path.exists(out_dir):
        shutil.rmtree(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    count = 0
    for number, path in enumerate(files):
        names, arr, had = training_columns(pio.read_ply(path))
        print('Reflectance detected' if had else 'No reflectance detected, column added with zeros.')
        print(f'Voxelising {path} to {args.grid_size} grid sizes')
        cap = DeviceCap(args.seed, counter=number) if getattr(args, 'device_cap', False) else None   # (a counter per file)
        voxels, _ = voxelise(torch.from_numpy(arr).to('cuda'), args.grid_size, args.min_pts, args.max_pts, ground='n_z' not in names,
                             cap=cap)
        for v in voxels:
            torch.save(v.cpu().clone(), os.path.join(out_dir, f'voxel_{count}.pt'))
            count += 1
    return count


def main(argv=None):
    args = parse_args(argv)
    import torch
    if args.device != 'cuda' or not torch.cuda.is_available():
        raise SystemExit('train.py needs an MI355X: the HIP path has no CPU fallback')
    torch.set_num_threads(max(1, args.num_procs))
    args.wdir = os.path.abspath(args.wdir)
    args.mode = 'train'
    print('Mode: {}'.format(args.mode))

    # checkpointing, as the reference organises it (train.py:88-94): the old checkpoints are archived, then removed - unless this
    # run continues the one that wrote them (--resume with its state file there)
    args.checkpoints = np.arange(0, args.num_epochs + 1, max(1, int(args.num_epochs / args.checkpoint_saves)))
    resuming = bool(args.resume) and os.path.isfile(os.path.join(args.wdir, 'model', os.path.splitext(args.model)[0] + '_state.pth'))
    old = [] if resuming else glob.glob(os.path.join(args.wdir, 'checkpoints', '*.pth'))
    if old:
        shutil.make_archive(os.path.join(args.wdir, 'checkpoints_backup'), 'zip', os.path.join(args.wdir, 'checkpoints'))
    for f in old:
        os.remove(f)

    args.trfile = os.path.join(args.wdir, 'data', 'train', 'voxels')
    args.tefile = os.path.join(args.wdir, 'data', 'test', 'voxels')
    if args.preprocess:
        n = preprocess(sorted(glob.glob(os.path.join(args.wdir, 'data', 'train', '*.ply'))), args.trfile, args)
        print(f'{n} training voxels')
        if args.test:
            n = preprocess(sorted(glob.glob(os.path.join(args.wdir, 'data', 'test', '*.ply'))), args.tefile, args)
            print(f'{n} test voxels')
    if args.augmentation:
        print('Training with data augmentation performed on 25% of samples')

    from pointstowood_amd.trainer import SemanticTraining, stop_handlers
    if args.state_every is None and args.stop_at is None and not args.resume:
        return SemanticTraining(args)
    with stop_handlers():                                       # SIGTERM / SIGINT: the state is written behind the step in flight
        return SemanticTraining(args)


if __name__ == '__main__':
    main()
