#!/usr/bin/env python3
"""Times the two ways from a host point array to the resident training tensors, on the same machine in one run:

  (a) files   octree_level5 + build_grids + the float64 `.npy` files + LoadedVoxelDataset + to_device
              (what get_octree.py, util_get_grids.py and `NVFPCC.py train` do between them), share by share;
  (b) device  preprocess.preprocess_device: one call, float32 tensors left on the device.

Wall clock around work that ends in a device synchronise.  (b): --warmup + --calls calls, median [min, max].
(a) takes tens of seconds a call, so it runs --host-calls times, without warm-up; the device was warmed by then
when --order device-first (the default).  The clouds are tools/rd_sweep.py's bumpy ellipsoid shells.  --bits 11 | 12
shifts them by (2^bits - 1024) / 2 per axis, to the middle of the deeper volume, where they cross its octant planes;
route (a) is 10-bit only, so only route (b) is timed then.

    python tools/preprocess_bench.py                              # the table + one JSON line
    python tools/preprocess_bench.py --bits 12                    # two more octree levels (D = 7), route (b) only
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/preprocess_bench.py --device-only --calls 5
    python tools/preprocess_bench.py --kernel-stats OUT/.../*_kernel_stats.csv      # the per-kernel split of (b)
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLOUDS = {"360k": (146.0, 2_500_000), "1M": (245.0, 6_000_000)}          # make_cloud(seed 1, radius, n_dir)


def med(v):
    return "%.4g [%.4g, %.4g]" % (float(np.median(v)), min(v), max(v))


def files_route(pts, dev, tmp):
    """One run of route (a) -> {share: seconds} with 'total'."""
    import torch
    from nvfpcc_amd import preprocess as pp
    from nvfpcc_amd.dataloader import LoadedVoxelDataset
    t = [time.perf_counter()]
    tick = lambda: t.append(time.perf_counter())
    origins, _ = pp.octree_level5(pts); tick()
    gt, dist = pp.build_grids(pts, origins, dev); tick()
    fid = os.path.join(tmp, "c")
    np.save(f"{fid}_l5_origins", origins.astype(np.float64))
    np.save(f"{fid}_l5_gt_grid", gt)
    np.save(f"{fid}_l5_dist", dist); tick()
    data = LoadedVoxelDataset(f"{fid}_l5_origins.npy", f"{fid}_l5_gt_grid.npy", f"{fid}_l5_dist.npy")
    g, d = data.to_device(dev)
    torch.cuda.synchronize(); tick()
    names = ("octree_level5", "build_grids", "npy_write", "load_to_device")
    out = {k: b - a for k, a, b in zip(names, t, t[1:])}
    out["total"] = t[-1] - t[0]
    return out


def device_route(pts, dev, bits=10):
    import torch
    from nvfpcc_amd import preprocess as pp
    t0 = time.perf_counter()
    pre = pp.preprocess_device(pts, dev, bits=bits)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, pre


def kernel_split(path):
    """rocprofv3's *_kernel_stats.csv -> rows (kernel, calls, total ms, share of all kernel time)."""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    print("| kernel | calls | total ms | share |\n|---|---|---|---|")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        if ns / total >= 0.001:
            print("| %s | %s | %.3f | %.1f %% |" % (r["Name"].split("(")[0][:60], r["Calls"], ns / 1e6, 100 * ns / total))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clouds", default="360k,1M")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--device-only", action="store_true", help="route (b) only (the run to put under rocprofv3)")
    ap.add_argument("--bits", type=int, choices=[10, 11, 12], default=10,
                    help="bits per axis: above 10 the cloud is shifted to the middle of the volume and only (b) runs")
    ap.add_argument("--kernel-stats", default=None, help="print the split of a rocprofv3 *_kernel_stats.csv and stop")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_split(args.kernel_stats)
    import torch
    from rd_sweep import make_cloud
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs a HIP device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"tool": "preprocess_bench", "bits": args.bits, "clouds": {}}
    device_only = args.device_only or args.bits > 10
    for name in args.clouds.split(","):
        radius, n_dir = CLOUDS[name]
        pts = make_cloud(1, radius, n_dir) + ((1 << args.bits) - 1024) // 2
        for _ in range(args.warmup):
            device_route(pts, dev, args.bits)
        times = []
        for _ in range(args.calls):
            dt, pre = device_route(pts, dev, args.bits)
            times.append(dt * 1e3)
        row = {"points": int(len(pts)), "blocks": int(pre.origins.shape[0]), "device_ms": times}
        print(f"[{name}] {len(pts)} points, {pre.origins.shape[0]} leaf blocks", flush=True)
        print(f"  (b) preprocess_device          {med(times)} ms", flush=True)
        del pre
        torch.cuda.empty_cache()
        if not device_only:
            runs = []
            for _ in range(args.host_calls):
                with tempfile.TemporaryDirectory() as tmp:
                    runs.append(files_route(pts, dev, tmp))
                torch.cuda.empty_cache()
            for k in ("octree_level5", "build_grids", "npy_write", "load_to_device", "total"):
                row["files_" + k + "_s"] = [r[k] for r in runs]
                print(f"  (a) {k:26s} {med([r[k] for r in runs])} s", flush=True)
            row["device_below_octree_level5"] = bool(max(times) / 1e3 < min(row["files_octree_level5_s"]))
        result["clouds"][name] = row
    print(json.dumps(result))


if __name__ == "__main__":
    main()
