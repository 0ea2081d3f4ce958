#!/usr/bin/env python3
"""Times the PLY readers and writers (nvfpcc_amd.ply_io) on the device against the host functions they stand in for.

    python tools/ply_io_bench.py [--sizes 100000 800000 3000000] [--bits 10 12] [--reps 10] [--out FILE.json]

Clouds are uniformly random points of `bits` bits per axis.  Every figure is a WHOLE call, wall clock, from the path
to the result and back: file access (a warm page cache: the file was just written), the copies in both directions and
the synchronisation included.  Each is the median of --reps calls (at least 10), and the routes of one pair alternate
call by call inside one run, so that they see the same machine:

    write   ply_io.write_ply(device)                 against  recon.write_ply_ascii
    read    ply_io.read_ply(device)                  against  preprocess.read_ply_xyz  and  pc_metrics.read_ply_points
    binary  ply_io.write_ply(fmt="binary") and ply_io.read_ply of that file, host and device destination

*_dev_passes_ms are device-event times of the passes alone on data that is already on the device: ops.ply_parse_xyz
(two line passes, torch's scan, the parse) and ops.ply_format_xyz (sizes, torch's scan, the read-back of the total, the
format).  Every route's result is checked against the cloud before it is timed.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nvfpcc_amd import ops, pc_metrics, ply_io, preprocess, recon  # noqa: E402


def alternating_ms(fns, reps):
    """Wall-clock medians (ms) of the calls of `fns`, taken in turn rep by rep; the device is idle at both ends."""
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[i].append(1e3 * (time.perf_counter() - t0))
    print("  medians of %d: %s ms" % (reps, ", ".join("%.1f" % np.median(ti) for ti in t)), file=sys.stderr, flush=True)
    return [float(np.median(ti)) for ti in t]


def event_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 800_000, 3_000_000])
    ap.add_argument("--bits", type=int, nargs="+", choices=(10, 11, 12), default=[10, 12])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.reps >= 10, "medians of at least 10 calls"
    dev = torch.device("cuda")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        host_ply, dev_ply, bin_ply = (os.path.join(tmp, f) for f in ("host.ply", "dev.ply", "bin.ply"))
        for bits in args.bits:
            for n in args.sizes:
                pts = np.random.default_rng(n + bits).integers(0, 1 << bits, size=(n, 3))
                row = {"n": n, "bits": bits}
                # the routes agree before anything is timed (and everything is warm afterwards)
                recon.write_ply_ascii(host_ply, pts)
                ply_io.write_ply(dev_ply, pts, device=dev)
                ply_io.write_ply(bin_ply, pts, fmt="binary")
                assert open(host_ply, "rb").read() == open(dev_ply, "rb").read()
                for got in (ply_io.read_ply(dev_ply, device=dev, fallback=False)[0].cpu().numpy(),
                            ply_io.read_ply(bin_ply, device=dev)[0].cpu().numpy(), ply_io.read_ply(bin_ply)[0],
                            preprocess.read_ply_xyz(host_ply), pc_metrics.read_ply_points(host_ply)[0]):
                    assert np.array_equal(got, pts)
                row["file_bytes"] = os.path.getsize(host_ply)
                row["write_device_ms"], row["write_host_ms"] = alternating_ms(
                    [lambda: ply_io.write_ply(dev_ply, pts, device=dev), lambda: recon.write_ply_ascii(host_ply, pts)],
                    args.reps)
                row["read_device_ms"], row["read_ply_xyz_ms"], row["read_ply_points_ms"] = alternating_ms(
                    [lambda: ply_io.read_ply(host_ply, device=dev, fallback=False),
                     lambda: preprocess.read_ply_xyz(host_ply), lambda: pc_metrics.read_ply_points(host_ply)], args.reps)
                row["write_binary_ms"], row["read_binary_host_ms"], row["read_binary_device_ms"] = alternating_ms(
                    [lambda: ply_io.write_ply(bin_ply, pts, fmt="binary"), lambda: ply_io.read_ply(bin_ply),
                     lambda: ply_io.read_ply(bin_ply, device=dev)], args.reps)
                raw = np.fromfile(host_ply, np.uint8)
                text = torch.from_numpy(raw).to(dev)[ply_io.parse_header(raw[:4096].tobytes()).body:]
                xyz = torch.from_numpy(pts.astype(np.int32)).to(dev)
                row["parse_dev_passes_ms"] = event_ms(lambda: ops.ply_parse_xyz(text, 0, n, 3, (0, 1, 2)), args.reps)
                row["format_dev_passes_ms"] = event_ms(lambda: ops.ply_format_xyz(xyz), args.reps)
                rows.append(row)
                print(json.dumps(row), flush=True)
    line = json.dumps({"reps": args.reps, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
