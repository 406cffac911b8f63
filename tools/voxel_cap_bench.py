#!/usr/bin/env python3
"""The voxeliser's ``max_pts`` cap on a dense plot: the per-voxel host route (``voxelise(generator=...)``: an index slice, a
``torch.multinomial``, a gather and a NaN filter per oversized voxel) beside the device cap (``voxelise(cap=DeviceCap(seed))``: one
``ops.cap_subset`` call and one gather per grid size).

    python tools/voxel_cap_bench.py [--repeat 10] [--commit <hash>] [--out profiles/voxel_cap_bench.json]

1. ``preprocessing.voxelise`` of a synthetic plot of ``--points`` points, uniform in a 16 m x 16 m x 8 m box (2 500 points per cubic
   metre at the default 5 120 000: every 2 m cell holds about 20 000 points, every 4 m cell about 160 000), grid sizes 2 m and 4 m,
   ``min_pts`` 128, ``max_pts`` 16 384, with reflectance: the two routes by a host clock from an idle device to a device
   synchronise - the host's waits are part of what the device cap removes.  How many voxels exceed ``max_pts`` is recorded per grid.
2. The operator alone on the 2 m grid's oversized runs: ``ops.cap_subset`` beside the loop of one ``torch.multinomial`` per run, by the
   same clock, and the operator by device events.

One process; two warm-up calls per route, then ``--repeat`` calls that alternate between the routes; median, minimum and maximum.  The
device cap is called faster only where the gain of the medians exceeds the larger of the two routes' min-to-max spreads; no ratio is
asserted: what is measured is what is written.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointstowood_amd import ops, preprocessing  # noqa: E402

SEED, GRIDS, MIN_PTS, MAX_PTS = 141190, (2.0, 4.0), 128, 16384
BOX = (16.0, 16.0, 8.0)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def host_clock(fn):
    """fn() from an idle device to an idle device, in host milliseconds"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def dense_plot(n, dev):
    g = torch.Generator(device=dev).manual_seed(SEED)
    xyz = torch.rand(n, 3, generator=g, device=dev) * torch.tensor(BOX, device=dev)
    return torch.cat([xyz, torch.randn(n, 1, generator=g, device=dev)], 1)


def verdict(r, a, b):
    spread = max(r[k]["ms_max"] - r[k]["ms_min"] for k in (a, b))
    gain = r[a]["ms_median"] - r[b]["ms_median"]
    return {"median_gain_ms": gain, "larger_spread_ms": spread, "gain_exceeds_spread": gain > spread}


def run_voxelise(pc, repeat):
    routes = {"host_route": lambda i: preprocessing.voxelise(pc, GRIDS, MIN_PTS, MAX_PTS, mode="xyz",
                                                             generator=torch.Generator(device=pc.device).manual_seed(i)),
              "device_cap": lambda i: preprocessing.voxelise(pc, GRIDS, MIN_PTS, MAX_PTS, mode="xyz",
                                                             cap=preprocessing.DeviceCap(SEED, counter=i))}
    times = {k: [] for k in routes}
    for i in range(2 + repeat):
        for name, fn in routes.items():                           # the routes alternate
            ms = host_clock(lambda: fn(i))
            if i >= 2:
                times[name].append(ms)
    r = {k: summary(v) for k, v in times.items()}
    per_grid = [[v.shape[0] for v in preprocessing.voxelise(pc, (g,), MIN_PTS, 1 << 30, mode="xyz")[0]] for g in GRIDS]
    capped, _ = routes["device_cap"](0)
    sizes = sum(per_grid, [])
    r.update(voxels=len(sizes), voxels_above_max_pts=sum(s > MAX_PTS for s in sizes), largest_voxel=max(sizes),
             voxels_above_max_pts_per_grid={str(g): sum(s > MAX_PTS for s in p) for g, p in zip(GRIDS, per_grid)},
             capped_voxels_have_max_pts_rows=all(c.shape[0] == min(s, MAX_PTS) for c, s in zip(capped, sizes)),
             clock="host clock around a voxelise that ends in torch.cuda.synchronize()", **verdict(r, "host_route", "device_cap"))
    return r


def run_operator(pc, repeat):
    order, starts, counts = preprocessing.HipBackend.grid_segments(pc[:, :3].contiguous(), GRIDS[0], MIN_PTS)
    over = counts > MAX_PTS
    starts, counts = starts[over].contiguous(), counts[over].contiguous()
    runs = list(zip(starts.tolist(), counts.tolist()))
    weight = pc[:, 3] - pc[:, 3].min() + 1e-8
    sorted_weight, n = weight[order].contiguous(), pc.shape[0]

    def loop(i):
        g = torch.Generator(device=pc.device).manual_seed(i)
        return [order[s:s + c][torch.multinomial(weight[order[s:s + c]], MAX_PTS, generator=g)] for s, c in runs]

    routes = {"multinomial_loop": loop,
              "cap_subset": lambda i: ops.cap_subset(n, starts, counts, MAX_PTS, SEED, counter=(0, i), weight=sorted_weight, row_id=order)}
    times = {"multinomial_loop": [], "cap_subset": [], "cap_subset_events": []}
    for i in range(2 + repeat):
        for name, fn in routes.items():
            ms = host_clock(lambda: fn(i))
            if i >= 2:
                times[name].append(ms)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        routes["cap_subset"](i)
        b.record()
        b.synchronize()
        if i >= 2:
            times["cap_subset_events"].append(a.elapsed_time(b))
    r = {k: summary(v) for k, v in times.items()}
    r.update(grid=GRIDS[0], rows=n, segments=len(runs), rows_in_segments=int(counts.sum()), k=MAX_PTS,
             **verdict(r, "multinomial_loop", "cap_subset"))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--points", type=int, default=5_120_000)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (recorded as given)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_cap_bench needs an MI355X: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    pc = dense_plot(a.points, dev)
    res = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "commit": a.commit, "repeat": a.repeat,
           "warmups": 2, "cpu": cpu_model(), "seed": SEED, "points": a.points, "box_m": BOX, "grid_sizes": GRIDS, "min_pts": MIN_PTS,
           "max_pts": MAX_PTS, "mode": "xyz", "reflectance": True}
    r = res["voxelise"] = run_voxelise(pc, a.repeat)
    for k in ("host_route", "device_cap"):
        print(f"voxelise, {k}: {r[k]['ms_median']:.1f} ms ({r[k]['ms_min']:.1f}..{r[k]['ms_max']:.1f})", flush=True)
    print(f"{r['voxels_above_max_pts']} of {r['voxels']} voxels above max_pts; gain {r['median_gain_ms']:.1f} ms, larger spread "
          f"{r['larger_spread_ms']:.1f} ms", flush=True)
    r = res["operator"] = run_operator(pc, a.repeat)
    for k in ("multinomial_loop", "cap_subset", "cap_subset_events"):
        print(f"{r['segments']} segments of the 2 m grid, {k}: {r[k]['ms_median']:.3f} ms ({r[k]['ms_min']:.3f}..{r[k]['ms_max']:.3f})",
              flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
