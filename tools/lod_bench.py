#!/usr/bin/env python3
"""Times the decode of N resident blocks at level of detail 0, 1 and 2 on the GPU.

    python tools/lod_bench.py --blocks 917 --batch 64 --chanstr 8,16,8,8 --ch 3 --reps 20 --warmup 3

What is timed is a whole call, latents on the device in, points and counts on the device out:

    lod 0            recon.reconstruct_points per slice of recon.eval_batches: Net.reconstruct + ops.threshold_points
    lod 1 / 2 fused  Net.reconstruct_lod + ops.head_points (nvf_head_occ_bits + nvf_points_from_bits)
    lod 1 / 2 plain  Net.reconstruct_lod(return_p=True) + ops.threshold_points: the head forward writes p, two more
                     kernels read it back

Each call is bracketed by device events and ends in a synchronise; the routes alternate inside every repetition, the
first --warmup repetitions are dropped and the median, minimum and maximum of the rest are reported in milliseconds.
The fused and the plain route are compared for equal points first (faster and different is not faster).  Weights and
latents are seeded random numbers: the time of these kernels does not depend on the values, only the number of points
written does, which the thresholds (medians of each level's probabilities) hold at half the voxels.
Prints one JSON line.  There is no CPU path: without a HIP device it exits with an error."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=917)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--chanstr", default="8,16,8,8")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lod_bench.py needs a HIP device: nothing here can be timed on a CPU")
    from nvfpcc_amd import network, ops
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    dev = torch.device("cuda")
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", a.ch, a.chanstr, verbose=False)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("kernel") or n.endswith(".b"):
                p.add_(0.03 * torch.randn(p.shape, generator=g))
    net = net.to(dev)
    lat = torch.round(2.0 * torch.randn(a.blocks, a.ch, 2, 2, 2, generator=g)).to(dev)
    idx = np.arange(a.blocks)
    origins = torch.from_numpy(np.stack([(idx // 1024) % 32, (idx // 32) % 32, idx % 32], 1) * 32).to(torch.int32).to(dev)
    heads = {lod: net.lod_head_params(lod) for lod in (1, 2)}
    chunks = [(lo, min(lo + a.batch, a.blocks)) for lo in range(0, a.blocks, a.batch)]

    with torch.no_grad():
        thh = {0: float(net.reconstruct(lat[:a.batch].contiguous(), 2).median())}
        for lod in (1, 2):
            thh[lod] = float(net.reconstruct_lod(lat[:a.batch].contiguous(), lod, return_p=True)[1].median())

    def lod0():
        return [ops.threshold_points(net.reconstruct(lat[lo:hi].contiguous(), 2), thh[0], origins[lo:hi]) for lo, hi in chunks]

    def fused(lod):
        w, b = heads[lod]
        return [ops.head_points(net.reconstruct_lod(lat[lo:hi].contiguous(), lod), w, b, thh[lod], origins[lo:hi], lod)
                for lo, hi in chunks]

    def plain(lod):
        return [ops.threshold_points(net.reconstruct_lod(lat[lo:hi].contiguous(), lod, return_p=True)[1], thh[lod],
                                     origins[lo:hi] >> lod) for lo, hi in chunks]

    routes = {"lod0": lod0, "lod1_fused": lambda: fused(1), "lod1_plain": lambda: plain(1),
              "lod2_fused": lambda: fused(2), "lod2_plain": lambda: plain(2)}
    points = {}
    with torch.no_grad():
        for lod in (1, 2):
            f, p = fused(lod), plain(lod)
            same = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(f, p))
            if not same:
                raise SystemExit(f"lod {lod}: the fused and the plain route give different points")
            points[f"lod{lod}"] = int(sum(x[0].shape[0] for x in f))
        points["lod0"] = int(sum(x[0].shape[0] for x in lod0()))
        times = {k: [] for k in routes}
        for rep in range(a.warmup + a.reps):
            for name, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
    out = {"tool": "lod_bench", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "batch": a.batch,
           "chanstr": a.chanstr, "reps": a.reps, "warmup": a.warmup, "points": points, "thresholds": thh,
           "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                  for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
