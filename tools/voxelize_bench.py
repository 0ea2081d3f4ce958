#!/usr/bin/env python3
"""Times the voxeliser on the device (nvfpcc_amd.voxelize) next to its numpy restatement (tests/voxelize_ref.py).

    python tools/voxelize_bench.py --points 800000,3000000 --bits 10 --reps 10 --warmup 2

What is timed, for every point count:

    device_fit / device_given   a whole voxelize() call on float64 points already on the device, the lattice fitted or
                                given: bounds (fit only), quantise, torch.sort, unique and the read of the status record,
                                which ends the call in a synchronise
    numpy_fit / numpy_given     tests/voxelize_ref.voxelize on the same points on the host, with torch / numpy limited
                                to --threads threads (16 when absent; numpy's unique is one thread whatever is allowed)
    upload                      the float64 points host to device, with a synchronise: what a caller with a file pays
                                before device_*
    kernels                     nvf_vox_bounds, nvf_vox_quantize, torch.sort of the keys, nvf_vox_unique and
                                nvf_vox_dequantize each alone, bracketed by device events, and the bytes each moves
                                over that time

The routes alternate inside every repetition; the first --warmup repetitions are dropped and the median, minimum and
maximum of the rest are reported in milliseconds.  The cloud is a seeded surface sample: points on a sphere shell with
Gaussian thickness in a frame of its own, float32-rounded, a tenth of them repeated.  The device result is compared with
the reference's before anything is timed.  Prints one JSON line.  Not measured here: real scans, files with attributes
(reading and parsing a file is not in any row), a cold page cache."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n - n // 10, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = (1.7 + 0.002 * rng.normal(size=(len(d), 1))) * d * (1.0, 0.8, 1.3) + (12.5, -3.0, 140.0)
    x = np.concatenate([x, x[rng.integers(0, len(x), size=n - len(x))]])
    return x[rng.permutation(n)].astype(np.float32).astype(np.float64)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="800000,3000000")
    ap.add_argument("--bits", type=int, default=10, choices=[10, 11, 12])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxelize_bench.py needs a HIP device: nothing here can be timed on a CPU")
    torch.set_num_threads(a.threads)
    from nvfpcc_amd import ops, voxelize as vx
    from tests import voxelize_ref as R
    dev = torch.device("cuda:0")
    out = {"bits": a.bits, "reps": a.reps, "warmup": a.warmup, "threads": a.threads, "sizes": {}}

    def host_ms(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for n in (int(v) for v in a.points.split(",")):
        x = cloud(n)
        xd = torch.from_numpy(x).to(dev)
        ref = R.voxelize(x, a.bits)
        lat = vx.Lattice(*ref.lattice)
        got = vx.voxelize(xd, dev, bits=a.bits)
        assert got.lattice == lat and np.array_equal(got.points.cpu().numpy(), ref.points)
        assert np.array_equal(got.counts.cpu().numpy(), ref.counts) and got.max_err2 == ref.max_err2
        m = len(ref.points)
        routes = {
            "device_fit": lambda: host_ms(lambda: vx.voxelize(xd, dev, bits=a.bits)),
            "device_given": lambda: host_ms(lambda: vx.voxelize(xd, dev, lattice=lat)),
            "numpy_fit": lambda: host_ms(lambda: R.voxelize(x, a.bits)),
            "numpy_given": lambda: host_ms(lambda: R.voxelize(x, a.bits, ref.lattice)),
            "upload": lambda: host_ms(lambda: torch.from_numpy(x).to(dev)),
        }
        kernels = {k: [] for k in ("bounds", "quantize", "sort", "unique", "dequantize")}
        times = {k: [] for k in routes}
        for rep in range(a.warmup + a.reps):
            keep = rep >= a.warmup
            for name, fn in routes.items():
                ms = fn()
                if keep:
                    times[name].append(ms)
            t_b, _ = event_ms(lambda: lib_bounds(ops, xd))
            t_q, (_, keys, status) = event_ms(lambda: ops.vox_quantize(xd, lat.bits, lat.origin, lat.step, lat.inv))
            t_s, skeys = event_ms(lambda: torch.sort(keys).values)
            t_u, (pts, _) = event_ms(lambda: ops.vox_unique(skeys, lat.bits, status))
            t_d, _ = event_ms(lambda: ops.vox_dequantize(pts[:m], lat.origin, lat.step))
            if keep:
                for k, t in zip(kernels, (t_b, t_q, t_s, t_u, t_d)):
                    kernels[k].append(t)
        # bytes the algorithm needs: 24 in (bounds); 24 in, 12 + 8 out (quantise); 8 in, 4 cleared, 16 out per voxel (unique:
        # the keys are read twice, by the sums and by the emit pass); 12 in, 24 out per voxel (dequantise)
        need = {"bounds": 24 * n, "quantize": 44 * n, "unique": 20 * n + 16 * m, "dequantize": 36 * m}
        size = {"points": n, "voxels": m, **{k: stats(v) for k, v in times.items()}, "kernels": {}}
        for k, v in kernels.items():
            size["kernels"][k] = stats(v)
            if k in need:
                size["kernels"][k]["bytes"] = need[k]
                size["kernels"][k]["GB_per_s"] = round(need[k] / (statistics.median(v) * 1e-3) / 1e9, 1)
        size["speedup_fit"] = round(size["numpy_fit"]["median_ms"] / size["device_fit"]["median_ms"], 1)
        size["speedup_given"] = round(size["numpy_given"]["median_ms"] / size["device_given"]["median_ms"], 1)
        out["sizes"][str(n)] = size
    print(json.dumps(out))


def lib_bounds(ops, xd):
    """nvf_vox_bounds without the read of its record (ops.vox_bounds ends in one)."""
    from nvfpcc_amd._lib import lib, check
    bounds = torch.empty(ops.VOX_BOUNDS_WORDS, dtype=torch.int64, device=xd.device)
    work = torch.empty(ops.VOX_BOUNDS_WORK_WORDS, dtype=torch.int64, device=xd.device)
    check(lib().nvf_vox_bounds(xd.data_ptr(), xd.shape[0], bounds.data_ptr(), work.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "nvf_vox_bounds")
    return bounds


if __name__ == "__main__":
    main()
