#!/usr/bin/env python3
"""Time of one whole thh_select.threshold_for_count call (three histogram passes + the digit choice on the device)
against what torch offers for the same job on the same tensor, in one process:

    python tools/thh_select_bench.py [--blocks 917,4096] [--repeats 20]

Fields: `uniform` (every key different: no equal keys to peel, the plain LDS adds carry the pass) and `saturated` (91 %
exact zeros, 6 % exact ones, the rest spread: what a trained decoder gives).  Baselines: torch.sort of the flattened
tensor (whole cloud) and torch.sort along dim 1 (per block), then one indexed read -- torch.kthvalue is timed too for
the per-block case (it takes one k for all rows).  Each figure: median, min and max of --repeats timed calls after 3
warm-up calls, wall clock around a device synchronise.  One JSON line per figure."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(kind, blocks, voxels=32768):
    g = torch.Generator(device="cuda").manual_seed(blocks)
    p = torch.rand((blocks, voxels), device="cuda", generator=g)
    if kind == "saturated":
        u = torch.rand((blocks, voxels), device="cuda", generator=g)
        p = torch.where(u < 0.91, torch.zeros_like(p), torch.where(u < 0.97, torch.ones_like(p), p))
    return p.contiguous()


def timed(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="917,4096")
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    from nvfpcc_amd import ops, thh_select as ts
    for blocks in [int(b) for b in a.blocks.split(",")]:
        for kind in ("uniform", "saturated"):
            p = make(kind, blocks)
            k_all = int(0.03 * p.numel())
            k_blk = torch.full((blocks,), int(0.03 * p.shape[1]), dtype=torch.int64, device="cuda")
            flat, kb0 = p.reshape(-1), int(0.03 * p.shape[1])
            jobs = {
                "hist_pass_count_only": lambda: ops.occ_hist(p, 21, 11),
                "select_whole_cloud": lambda: ts.threshold_for_count(p, k_all),
                "select_per_block": lambda: ts.threshold_for_count(p, k_blk),
                "torch_sort_whole_cloud": lambda: torch.sort(flat, descending=True).values[k_all - 1],
                "torch_sort_per_block": lambda: torch.sort(p, dim=1, descending=True).values[:, kb0 - 1],
                "torch_kthvalue_per_block": lambda: torch.kthvalue(p, p.shape[1] - kb0 + 1, dim=1).values,
            }
            want = torch.sort(flat, descending=True).values[k_all - 1]
            assert torch.equal(ts.kth_largest(p, k_all), want)
            for name, fn in jobs.items():
                print(json.dumps({"blocks": blocks, "field": kind, "what": name, **timed(fn, a.repeats)}), flush=True)
            del p, flat


if __name__ == "__main__":
    main()
