"""Inference driver pieces that feed and consume the forward (reference ``pointstowood/src/predicter.py``).

* ``VoxelDataset``      - ``TestingDataset`` (:65-94): per voxel ``local_shift = mean(xyz)``, centre,
                          ``sf = max ||p||`` and only then the NaN-row filter (same order as the reference).
* ``BalancedBatchSampler`` (:23-63): pairs short with long voxels.  ``reference=True`` reproduces the
                          reference exactly (unseeded numpy shuffles, remainder silently dropped, batch_size 1
                          is an error); the default keeps the pairing but covers every voxel and is deterministic.
* ``load_model``        (:97-105): strips ``module.`` prefixes, ``strict=False``.
* ``classify``          - the loop body (:193-215): forward, ``nan_to_num``, sigmoid, ``>= is_wood``,
                          un-shift by ``local_shift[3b:3b+3]``; returns ``[sum N, 5]`` = x, y, z, pred, prob.
* ``classify_sharded``  - the same over ``torch.distributed``: voxel batches are partitioned over ranks
                          (``dist.partition_batches``), results gathered with ONE collective per call.
"""
from __future__ import annotations

import glob
import os
from collections import OrderedDict

import numpy as np
import torch

from .data import Batch, Data, DataLoader, serial_host_ops
from .dist import batch_cost, partition_batches


class VoxelDataset(torch.utils.data.Dataset):
    def __init__(self, voxels, reflectance_index: int = 3):
        if isinstance(voxels, (str, os.PathLike)):
            if not voxels:
                raise ValueError("The 'voxels' parameter cannot be empty.")
            self.keys = sorted(glob.glob(os.path.join(voxels, "*.pt")))
            self._mem = None
        else:
            self._mem = list(voxels)
            self.keys = list(range(len(self._mem)))
        self.reflectance_index = reflectance_index

    label_index = None        # column of the truth labels: ``evaluate.LabelledVoxelDataset`` sets it, and every item then carries ``y``

    def __len__(self):
        return len(self.keys)

    def raw(self, index):
        if self._mem is not None:
            return self._mem[index]
        kept = getattr(self, "_kept", None)
        if kept is not None and kept[index] is not None:
            return kept[index]
        return torch.load(self.keys[index])

    PRELOAD_BYTES = 8 << 30   # host memory preload() may keep (a 10 M-point plot's voxels are ~0.4 GB; 100 M+ points would be tens of GB)

    def preload(self, max_bytes: int | None = None):
        """Reads every voxel file once for its length (the reference reads each file twice: its sampler loads every voxel for its
        length, the loader loads it again - predicter.py:28-31,78-80) and KEEPS the tensors while they fit ``max_bytes`` of host
        memory (default ``PRELOAD_BYTES``); voxels beyond the budget are read again from disk when their batch is built (the
        reference's streaming behaviour).  Returns the voxel lengths, also kept as ``lengths``."""
        if self._mem is not None:
            self.lengths = [int(len(v)) for v in self._mem]
            return self.lengths
        budget = self.PRELOAD_BYTES if max_bytes is None else int(max_bytes)
        kept, lengths, used = [], [], 0
        for k in self.keys:
            v = torch.load(k)
            lengths.append(int(len(v)))
            nbytes = v.numel() * v.element_size() if isinstance(v, torch.Tensor) else 0
            if isinstance(v, torch.Tensor) and used + nbytes <= budget:
                kept.append(v)
                used += nbytes
            else:
                kept.append(None)
        self._kept, self.lengths = kept, lengths
        return self.lengths

    def __getitem__(self, index):
        pc = torch.as_tensor(self.raw(index))
        with serial_host_ops():   # a dozen small CPU operations: one intra-op thread (25 ms -> 1 ms per batch of 8 on the GPU hosts)
            pos = pc[:, :3].to(torch.float32)
            refl = pc[:, self.reflectance_index].to(torch.float32)
            shift = pos.mean(dim=0)
            pos = pos - shift
            sf = torch.sqrt((pos ** 2).sum(dim=1)).max()
            y = None if self.label_index is None else pc[:, self.label_index].to(torch.float32)
            bad = torch.isnan(pos).any(dim=1) | torch.isnan(refl)
            if bool(bad.any()):
                print(f"Encountered NaN values in sample at index {index}")
                pos, refl = pos[~bad], refl[~bad]
                y = None if y is None else y[~bad]
        if y is not None:
            return Data(pos=pos, reflectance=refl, y=y, local_shift=shift, sf=sf)
        return Data(pos=pos, reflectance=refl, local_shift=shift, sf=sf)


class BalancedBatchSampler(torch.utils.data.Sampler):
    def __init__(self, dataset, batch_size: int, reference: bool = False, seed: int = 0):
        self.dataset, self.batch_size, self.reference, self.seed = dataset, int(batch_size), reference, seed
        self.lengths = [len(dataset.raw(i)) for i in range(len(dataset))]
        dataset.lengths = self.lengths
        self.indices = np.argsort(self.lengths, kind="stable")

    def __iter__(self):
        n, half = len(self.indices), self.batch_size // 2
        short, long_ = self.indices[: n // 2].copy(), self.indices[n // 2:].copy()
        if self.reference:
            if half == 0:
                raise ValueError("range() arg 3 must not be zero")  # the reference's behaviour at batch_size 1
            np.random.shuffle(short)
            np.random.shuffle(long_)
            for i in range(0, len(short) - half + 1, half):
                if i + half <= len(long_):
                    batch = list(short[i:i + half]) + list(long_[i:i + half])
                    np.random.shuffle(batch)
                    yield [int(b) for b in batch]
            return
        rng = np.random.default_rng(self.seed)
        rng.shuffle(short)
        rng.shuffle(long_)
        hs, hl = max(half, 1) if self.batch_size > 1 else 0, self.batch_size - (max(half, 1) if self.batch_size > 1 else 0)
        i = j = 0
        while i < len(short) or j < len(long_):
            batch = list(short[i:i + hs]) + list(long_[j:j + hl])
            i, j = i + hs, j + hl
            if len(batch) < self.batch_size:  # top up from whichever half still has voxels
                need = self.batch_size - len(batch)
                extra_s = list(short[i:i + need]); i += len(extra_s)
                extra_l = list(long_[j:j + need - len(extra_s)]); j += len(extra_l)
                batch += extra_s + extra_l
            if batch:
                yield [int(b) for b in batch]

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.reference else -(-n // self.batch_size)


class PointBudgetSampler(torch.utils.data.Sampler):
    """Batches by a point budget instead of a voxel count: voxels are taken longest-first and packed greedily (first
    fit) into batches of at most ``max_points`` points / ``max_voxels`` voxels.  Covers every voxel, deterministic, and
    keeps every forward near the size the kernels are efficient at, whatever the voxel-size distribution (a plot
    voxelised at 2 m + 4 m has a median voxel of a few hundred points).  Not in the reference (its sampler fixes the
    voxel count and drops the remainder): batch composition only enters the result through the batch-global grid
    origin of ``voxel_grid``, exactly as it does there."""

    def __init__(self, lengths, max_points: int = 131072, max_voxels: int = 128):
        self.lengths = [int(n) for n in lengths]
        order = sorted(range(len(self.lengths)), key=lambda i: (-self.lengths[i], i))
        self.batches, room = [], []
        for i in order:
            n = self.lengths[i]
            for b, r in enumerate(room):
                if n <= r and len(self.batches[b]) < max_voxels:
                    self.batches[b].append(i)
                    room[b] -= n
                    break
            else:
                self.batches.append([i])
                room.append(max(0, max_points - n))

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def collate_device(voxels, reflectance_index: int = 3):
    """Feed step for voxels that already live on the GPU (e.g. from ``preprocessing.voxelise``): the per-voxel
    ``local_shift = mean(xyz)``, centring and ``sf = max ||p||`` of ``TestingDataset.__getitem__`` + PyG collation
    (predicter.py:78-94,177) for a whole batch in a handful of vectorised device ops and NO host synchronisation.
    Assumes NaN rows were already removed (the voxeliser does that).  The mean is a sequential per-segment sum on the
    device, so ``local_shift`` can differ from the reference's CPU mean in the last bits (a pure translation)."""
    dev = voxels[0].device
    n = [int(v.shape[0]) for v in voxels]
    B, total = len(voxels), sum(n)
    cat = torch.cat(voxels, 0)
    pos = cat[:, :3].to(torch.float32)
    refl = cat[:, reflectance_index].to(torch.float32).contiguous()
    lengths = torch.tensor(n, device=dev)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), lengths, output_size=total)
    shift = torch.segment_reduce(pos.contiguous(), "mean", lengths=lengths)
    pos = pos - shift[batch]
    sf = torch.segment_reduce(torch.sqrt((pos ** 2).sum(dim=1)), "max", lengths=lengths)
    ptr = torch.zeros(B + 1, dtype=torch.long)
    ptr[1:] = torch.cumsum(torch.tensor(n), 0)
    out = Batch(pos=pos.contiguous(), reflectance=refl, local_shift=shift.reshape(-1), sf=sf, batch=batch,
                ptr=ptr.to(dev, non_blocking=True))
    out.num_graphs = B
    return out


def load_model(path, model, device):
    ckpt = torch.load(path, map_location=device)
    sd = OrderedDict()
    for key, value in ckpt["model_state_dict"].items():
        sd[key[7:] if key.startswith("module.") else key] = value
    model.load_state_dict(sd, strict=False)
    return model


@torch.no_grad()
def classify_batch(model, data, is_wood: float, device):
    """One iteration of the reference loop; returns a float64 numpy array [n, 5]."""
    data = data.to(device)
    logits = torch.nan_to_num(model(data))
    probs = torch.sigmoid(logits).reshape(-1)
    preds = (probs >= is_wood).to(torch.int64)
    return _rows(data, preds, probs).cpu().numpy()


def _rows(data, preds, probs):
    """[n, 5] float64 = (un-shifted xyz, prediction, probability) as predicter.py:203-211 builds them: numpy's concatenate of
    float32 positions, int64 predictions and float32 probabilities is float64, and the shift is added to THAT array - the
    un-shifted coordinates are the float64 sums of two float32 values, not their float32 sums."""
    shift = data.local_shift.reshape(-1, 3)[data.batch.long()]
    xyz = data.pos[:, :3].to(torch.float64) + shift.to(torch.float64)
    return torch.cat([xyz, preds[:, None].to(torch.float64), probs[:, None].to(torch.float64)], dim=1)


def _consume(logits, data, is_wood: float):
    """The post-processing of one batch (predicter.py:197-211) on the device: [n, 5] = un-shifted xyz, prediction, probability."""
    probs = torch.sigmoid(torch.nan_to_num(logits)).reshape(-1)
    preds = (probs >= is_wood).to(torch.int64)
    return _rows(data, preds, probs)


def classify(model, loader, is_wood: float = 0.5, device="cuda", counts: list | None = None):
    """The reference's inference loop (predicter.py:193-213).  A model with a ``stream`` method (``pointstowood_amd.Net``) on a GPU
    gets the batches through its software pipeline (geometry of the next batch beside the features of the current ones, no
    device-to-host copy between batches); the rows and their order are those of one ``classify_batch`` per batch.
    ``counts`` (a list, optional) receives the row count of every batch."""
    if hasattr(model, "stream") and torch.device(device).type == "cuda":
        held, outs = [], []

        def feed():
            for data in loader:
                d = data.to(device, non_blocking=True)       # (pinned by the loader: the copy overlaps the forwards in flight)
                held.append(d)
                yield d
        with torch.no_grad():
            for logits in model.stream(feed()):
                outs.append(_consume(logits, held.pop(0), is_wood))
        if counts is not None:
            counts.extend(int(o.shape[0]) for o in outs)
        return torch.cat(outs).cpu().numpy() if outs else np.zeros((0, 5), dtype=np.float64)
    outs = [classify_batch(model, data, is_wood, device) for data in loader]
    if counts is not None:
        counts.extend(int(o.shape[0]) for o in outs)
    return np.vstack(outs) if outs else np.zeros((0, 5), dtype=np.float64)


def classify_voxels(model, dataset, is_wood: float = 0.5, device="cuda", batch_size: int = 8, reference_sampler: bool = False,
                    max_points: int = 262144, max_voxels: int = 256):
    """``predict.py --voxels`` on one GPU: every voxel of ``dataset`` through the model, rows as ``classify`` returns them
    ([n, 5] float64: un-shifted xyz, prediction, probability - predicter.py:193-213).

    Default: the voxels are read once (``VoxelDataset.preload``), packed into forwards of at most ``max_points`` points
    (``PointBudgetSampler``: every voxel exactly once, sizes the kernels are efficient at) and streamed through
    ``Net.stream`` - geometry of the next forward beside the features of the current ones, one device-to-host copy at the end.
    ``reference_sampler=True``: the reference's ``BalancedBatchSampler`` at ``batch_size`` voxels per forward (it draws from the
    global numpy RNG and drops the voxels of the last incomplete batch, as there), through the same pipeline."""
    batches = plan_batches(dataset, batch_size, reference_sampler, max_points, max_voxels)
    return classify(model, prefetch_batches(dataset, batches, pin=torch.device(device).type == "cuda"), is_wood, device)


def plan_batches(dataset, batch_size: int = 8, reference_sampler: bool = False, max_points: int = 262144, max_voxels: int = 256):
    """The forwards of a ``predict.py --voxels`` run as a list of voxel-index lists - ONE plan for one process and for every rank of a
    sharded run (it is deterministic, so every rank computes the same list and ``classify_sharded`` deals it out): logits depend
    on a batch's composition through the batch-global grid origin of ``voxel_grid``, so the same directory must give the same
    rows on 1 and on N GPUs.  Default: ``PointBudgetSampler`` (``batch_size`` is not used: forwards are sized in points);
    ``reference_sampler``: the reference's ``BalancedBatchSampler`` at ``batch_size`` voxels per forward (global numpy RNG - seed it
    identically on every rank -, remainder dropped, as there)."""
    if reference_sampler:
        return [list(b) for b in BalancedBatchSampler(dataset, batch_size, reference=True)]
    return [list(b) for b in PointBudgetSampler(dataset.preload(), max_points, max_voxels)]


def prefetch_batches(dataset, batches, pin: bool = True, workers: int = 1, ahead: int = 4):
    """The loader of ``classify_voxels``: yields ``Batch.from_data_list([dataset[i] for i in b])`` for every b of ``batches``, in
    order, built `ahead` batches ahead by a background thread and (``pin``) in pinned memory, so that the host-side feed - a dozen
    small tensor operations per voxel (predicter.py:78-94) - runs beside the forwards in flight instead of between them.  The
    dataset and the collation compute with ONE intra-op thread (``data.serial_host_ops``, restored after every call: the
    operations are a few thousand elements each, and with the process-wide thread count the reference's CLI sets - all cores,
    predict.py:79-84 - each of them costs a thread-team wake-up).  More than one worker thread does not pay: the per-voxel operations
    are too small to release the interpreter lock for long (measured: 0.43 s with 1 worker, 0.97 with 2, 6.1 with 8)."""
    import collections
    from concurrent.futures import ThreadPoolExecutor

    def build(b):
        with serial_host_ops():      # ... the pinned copies too: a parallel memcpy of a few MB wakes the whole OpenMP team
            out = Batch.from_data_list([dataset[i] for i in b])
            return out.pin_memory() if pin else out
    batches = list(batches)
    with ThreadPoolExecutor(max_workers=max(1, min(workers, len(batches)))) as pool:
        pending = collections.deque()
        it = iter(batches)
        for b in it:
            pending.append(pool.submit(build, b))
            if len(pending) > ahead + workers:
                break
        while pending:
            yield pending.popleft().result()
            nxt = next(it, None)
            if nxt is not None:
                pending.append(pool.submit(build, nxt))


def classify_sharded(model, dataset, batches, is_wood, device, dist):
    """``batches`` = list of voxel-index lists (identical on every rank).  Rank r classifies its share (LPT on the
    estimated FLOPs of every batch) and every rank receives all results, ordered by batch id: one all-reduce of the
    per-batch row counts (a voxel can lose rows to the NaN filter, which only its owner sees) and one all-gather of a
    padded buffer.  No rank touches a voxel it does not own."""
    world, rank = dist.get_world_size(), dist.get_rank()
    lengths = getattr(dataset, "lengths", None)
    costs = [sum(batch_cost(lengths[i]) if lengths is not None else 1.0 for i in b) for b in batches]
    plan = partition_batches(costs, world)
    # this rank's share through the same pipeline as one process (background feed -> Net.stream -> one D2H copy)
    rows_of, got = torch.zeros(len(batches), dtype=torch.int64), []
    on_gpu = torch.device(device).type == "cuda"
    mine = classify(model, prefetch_batches(dataset, [batches[bid] for bid in plan[rank]], pin=on_gpu), is_wood, device, counts=got)
    for bid, c in zip(plan[rank], got):
        rows_of[bid] = c
    local = torch.from_numpy(mine).to(device)
    rows_of = rows_of.to(device)
    dist.all_reduce(rows_of)                           # every batch has exactly one owner: the sum is its row count
    rows_of = [int(c) for c in rows_of.cpu()]
    counts = [sum(rows_of[b] for b in plan[r]) for r in range(world)]
    buf = torch.zeros((max(counts + [1]), 5), dtype=local.dtype, device=device)
    buf[: local.shape[0]] = local
    out = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)
    where = {}
    for r in range(world):
        off = 0
        for bid in plan[r]:
            where[bid] = (r, off, rows_of[bid])
            off += rows_of[bid]
    ordered = [out[where[b][0]][where[b][1]: where[b][1] + where[b][2]] for b in range(len(batches))]
    return torch.cat(ordered).cpu().numpy() if ordered else np.zeros((0, 5), dtype=np.float64)
