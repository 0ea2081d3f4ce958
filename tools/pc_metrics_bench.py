#!/usr/bin/env python3
"""Times the D1 / D2 geometry metrics (nvfpcc_amd.pc_metrics) on a longdress-sized cloud against scipy's cKDTree on
16 CPU threads, and one far-cluster worst case of the 1-NN search.

    python tools/pc_metrics_bench.py [--n-dir 1000000] [--reps 5] [--bits 10] [--index dense|sparse|both] [--out FILE.json]

Inputs: the bumpy-ellipsoid surface of tools/rd_sweep.make_cloud at ~0.8 M points (A, the reference) against a thinned
and jittered copy (B, the decoded stand-in).  GPU times are device events around whole geometry_psnr calls (index
build, searches, normals, sums and the host read-back of the sums) after one warm-up call; the CPU baseline builds the
two trees and queries both directions (D1), plus a 12-NN query and a batched numpy eigh for D2's normals.  Every
timing is the median of --reps runs (GPU: with the least and the greatest next to it as *_min / *_max).  The D1 values
of both sides are printed and must be equal (both are exact).

--bits 11 | 12 scales the shell by 2 | 4 about the volume centre (the far clusters keep their size and move apart
likewise).  --index picks the cell index of the search (default: the library's own choice, dense at 10 bits and sparse
above); `both` (10 bits only) times dense and sparse in one run, alternating them call by call, reports the sparse
figures under *_sparse keys and checks that the two results are equal.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rd_sweep import make_cloud  # noqa: E402
from nvfpcc_amd import pc_metrics  # noqa: E402


def perturbed(p, seed, top=1023):
    rng = np.random.default_rng(seed)
    q = p[rng.random(p.shape[0]) < 0.8]
    q = q + rng.integers(-1, 2, size=q.shape) * (rng.random((q.shape[0], 1)) < 0.3)
    return np.clip(q, 0, top)


def shell(seed, radius, n_dir, bits):
    """make_cloud's surface scaled by 2^(bits - 10) about the volume centre; make_cloud itself at 10 bits."""
    if bits == 10:
        return make_cloud(seed, radius, n_dir)
    scale = 1 << (bits - 10)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_dir, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    bump = 1.0 + 0.08 * np.sin(5 * d[:, 0]) * np.cos(4 * d[:, 1]) + 0.05 * np.sin(9 * d[:, 2])
    p = 512.0 * scale + d * bump[:, None] * np.array([radius, 0.85 * radius, 1.2 * radius]) * scale
    return np.unique(np.clip(np.round(p), 0, 1024 * scale - 1).astype(np.int64), axis=0)


def gpu_ms(fns, reps):
    """Times the calls of `fns` in turn, rep by rep, after one warm-up call each -> [(median, min, max, result)]."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t, r = [[] for _ in fns], [None] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r[i] = fn()
            e1.record()
            torch.cuda.synchronize()
            t[i].append(e0.elapsed_time(e1))
    return [(float(np.median(ti)), float(min(ti)), float(max(ti)), ri) for ti, ri in zip(t, r)]


def cpu_ms(fn, reps):
    t, r = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), r


def cpu_d1(a, b, workers):
    da = cKDTree(b).query(a, workers=workers)[0] ** 2
    db = cKDTree(a).query(b, workers=workers)[0] ** 2
    return max(np.round(da).sum() / a.shape[0], np.round(db).sum() / b.shape[0])


def cpu_normals(a, k, workers):
    _, idx = cKDTree(a).query(a, k=k, workers=workers)
    p = a[idx].astype(np.float64)
    c = p - p.mean(1, keepdims=True)
    return np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))[1][:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-dir", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--bits", type=int, choices=(10, 11, 12), default=10)
    ap.add_argument("--index", choices=("dense", "sparse", "both"), default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.bits == 10 or args.index in (None, "sparse"), "the dense index is 10-bit only"
    bits, scale = args.bits, 1 << (args.bits - 10)
    kinds = ["dense", "sparse"] if args.index == "both" else [args.index]
    a = shell(0, 450.0, args.n_dir, bits)
    b = perturbed(a, 1, 1024 * scale - 1)
    res = {"n_ref": int(a.shape[0]), "n_test": int(b.shape[0]), "bits": bits, "index": args.index}

    def timed(name, x, y, **kw):
        """Times geometry_psnr(x, y) under every index of `kinds` -> the first one's result."""
        runs = gpu_ms([lambda k=k: pc_metrics.geometry_psnr(x, y, bits=bits, index=k, **kw) for k in kinds], args.reps)
        for k, (med, lo, hi, r) in zip(kinds, runs):
            sfx = "_sparse" if k == "sparse" and len(kinds) == 2 else ""
            res[name + sfx], res[name + sfx + "_min"], res[name + sfx + "_max"] = med, lo, hi
            assert r == runs[0][3], (name, k)             # dense and sparse: the same dictionary
        return runs[0][3]

    g1 = timed("gpu_d1_ms", a, b, d2=False)
    g2 = timed("gpu_d1_d2_ms", a, b)
    res["cpu_d1_ms"], c1 = cpu_ms(lambda: cpu_d1(a, b, args.workers), args.reps)
    res["cpu_normals_ms"], _ = cpu_ms(lambda: cpu_normals(a, 12, args.workers), max(1, args.reps // 2))
    res["d1_mse_gpu"], res["d1_mse_cpu"], res["d2_mse_gpu"] = g1["d1_mse"], float(c1), g2["d2_mse"]
    res["d1_psnr"], res["d2_psnr"] = g2["d1_psnr"], g2["d2_psnr"]
    # far clusters: every query of one cluster ~ 1 200 voxels from the other
    fa = make_cloud(2, 60.0, 60_000) + 512 * (scale - 1) - 400 * scale
    fb = make_cloud(3, 60.0, 60_000) + 512 * (scale - 1) + 400 * scale
    res["far_n"] = [int(fa.shape[0]), int(fb.shape[0])]
    gf = timed("gpu_far_d1_ms", fa, fb, d2=False)
    res["cpu_far_d1_ms"], cf = cpu_ms(lambda: cpu_d1(fa, fb, args.workers), args.reps)
    res["far_d1_mse_gpu"], res["far_d1_mse_cpu"] = gf["d1_mse"], float(cf)
    assert res["d1_mse_gpu"] == res["d1_mse_cpu"] and res["far_d1_mse_gpu"] == res["far_d1_mse_cpu"], res
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
