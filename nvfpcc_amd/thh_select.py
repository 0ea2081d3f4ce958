"""Choosing the occupancy threshold at encode time, and carrying it in the pack.

The decoder's probabilities become points with `p > thh`.  This module finds thresholds from the probabilities
themselves, on the gfx950 kernels of csrc/occ_select.hip (C ABI: include/nvf_hip.h); there is no CPU fallback.

  key(p)                   the bit pattern of the float32 p: monotone on [0, 1], so the k-th largest probability is
                           the k-th largest key.  Three histogram passes (11 + 11 + 10 bits, top down, each
                           restricted to the prefix chosen so far) find it exactly.
  kth_largest(p, k)        v_k, over the whole cloud (k an int) or per block (k an int tensor [B]).
  threshold_for_count      t = nextafter(v_k, -inf): `p > t` keeps every voxel with p >= v_k.  Voxels that TIE at v_k
                           are all kept (no index tie-break), so the set can be larger than k; the result is a plain
                           threshold and the raster-order compaction of ops.threshold_points applies unchanged.
  curve(p, gt, d2, cands)  decoded point count, true positives and the decoded-to-original squared-error sum at every
                           candidate threshold, from ONE histogram pass whose bin edges are the candidates.  Integers.
  choose(mode, ...)        the three encoder modes of `NVFPCC.py --thh_mode`: count, block-count, d1.

Memory: the selection needs all probabilities at once, N_leaf x 128 KiB of float32 (120 MB at 917 blocks, 537 MB at
4096); `check_resident` refuses above MAX_RESIDENT_BYTES = 4 GiB, which is what the 32768 leaf blocks of a full
1024^3 volume take.  The d1 mode also keeps the integer squared-distance grid (same size) and the occupancy bytes.
"""
import math
import struct

import numpy as np
import torch

PASSES = ((21, 11), (10, 11), (0, 10))          # (shift, nbits) of the three digits, top down
MAX_RESIDENT_BYTES = 4 << 30
MODES = ("count", "block-count", "d1")
MODE_IDS = {"count": 1, "block-count": 2, "d1": 3}
D2_EXACT_BOUND = 1 << 22                        # see d2_from_dist
WINDOW = (2.0 / 3.0, 3.0 / 2.0)                 # the rule of thumb tools/rd_sweep.py states: decoded / input points
SHORTLIST = 16


# ---------------------------------------------------------------- host arithmetic (device-agnostic torch / numpy)
def choose_digit(hist, k):
    """One radix step of a k-th LARGEST search.  hist int64 [R, bins], k int64 [R] with 1 <= k <= hist.sum(1).
    -> (digit [R]: the bin holding the k-th largest key, k_rest [R]: its rank among the keys of that bin)."""
    bins = hist.shape[1]
    desc = hist.flip(1).cumsum(1)                               # desc[:, j] = keys with digit >= bins - 1 - j
    j = torch.searchsorted(desc, k[:, None].contiguous()).squeeze(1).clamp(max=bins - 1)   # first j with desc >= k
    above = torch.where(j > 0, desc.gather(1, (j - 1).clamp(min=0)[:, None]).squeeze(1), torch.zeros_like(k))
    return bins - 1 - j, k - above


def threshold_below(v):
    """nextafter(v, -inf) in float32: `p > t` is `p >= v` (v = 0 gives the smallest negative float)."""
    v = torch.as_tensor(v, dtype=torch.float32)
    return torch.nextafter(v, torch.full_like(v, -math.inf))


def fold_curve(count, sum_d2=None, count_gt=None):
    """Edge histograms [B, E + 1] (or already summed [E + 1]) -> per-candidate totals [E]: the voxels with
    p > edges[i] are the bins above i.  Returns {"count", "sse", "tp"} of int64 (a rider not given: None)."""
    def fold(h):
        if h is None:
            return None
        h = torch.as_tensor(h).long()
        h = h.sum(0) if h.dim() == 2 else h
        return h.flip(0).cumsum(0).flip(0)[1:].contiguous()
    return {"count": fold(count), "sse": fold(sum_d2), "tp": fold(count_gt)}


def d2_from_dist(dist):
    """The integer squared distances behind a distance grid (dist = sqrt of an integer, float32 or float64).

    Exact for every integer n < 2^22: a correctly rounded float32 sqrt is off by at most 2^-24 relative, so its
    float64 square is within n (2^-23 + 2^-48) < 0.5 of n and rounds back to n (float64 inputs are closer still).
    Squared distances of this codec are at most 3 * 1023^2 = 3139587 < 2^22, and nvf_nearest_dist2 searches the block
    itself and the blocks within two steps, so what it stores is far below that.  Raises above the bound."""
    t = dist if isinstance(dist, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dist))
    r = torch.round(t.double() ** 2)
    if r.numel() and (not bool(torch.isfinite(r).all()) or float(r.max()) >= D2_EXACT_BOUND):
        raise ValueError(f"distance grid holds values whose square is not below {D2_EXACT_BOUND}: not a codec grid")
    return r.to(torch.int32)


def encode_block_counts(k):
    """Per-block point counts -> raw little-endian uint16, 2 bytes per block (a 32^3 block holds at most 32768)."""
    k = np.asarray(k.cpu() if isinstance(k, torch.Tensor) else k).astype(np.int64).reshape(-1)
    if k.size and (k.min() < 0 or k.max() > 0xFFFF):
        raise ValueError("block counts must fit 16 bits")
    return k.astype("<u2").tobytes()


def decode_block_counts(data):
    return np.frombuffer(data, dtype="<u2").astype(np.int64)


def write_thh_pack(mode, t=None, block_counts=None):
    """The `thh_pack` entry of pack.pk: one mode byte, then the fp32 threshold (count, d1) or the uint16 counts
    (block-count).  Its length times 8 is the side information the encoder adds to Gross bpp."""
    if mode not in MODE_IDS:
        raise ValueError(f"unknown threshold mode {mode!r}")
    if mode == "block-count":
        return bytes([MODE_IDS[mode]]) + encode_block_counts(block_counts)
    return bytes([MODE_IDS[mode]]) + struct.pack("<f", float(t))


def read_thh_pack(data):
    """-> (mode, fp32 threshold as a Python float | int64 numpy counts)."""
    data = bytes(data)
    names = {v: k for k, v in MODE_IDS.items()}
    if len(data) < 1 or data[0] not in names:
        raise ValueError("thh_pack: unknown mode byte")
    mode = names[data[0]]
    if mode == "block-count":
        if (len(data) - 1) % 2:
            raise ValueError("thh_pack: block-count payload must hold 2 bytes per block")
        return mode, decode_block_counts(data[1:])
    if len(data) != 5:
        raise ValueError("thh_pack: expected one float32")
    return mode, struct.unpack("<f", data[1:])[0]


def threshold_line(mode, t=None, block_counts=None, thresholds=None):
    """The `[Threshold]` line encode and decode both print."""
    if mode == "block-count":
        k = np.asarray(block_counts, np.int64)
        th = np.asarray(thresholds, np.float32)
        return ("[Threshold] mode: block-count blocks: %d points asked: %d t_min: %.9g t_max: %.9g"
                % (k.size, int(k.sum()), float(th.min()), float(th.max())))
    return "[Threshold] mode: %s t: %.9g" % (mode, float(np.float32(t)))


def shortlist_counts(n_points, n_voxels):
    """Up to SHORTLIST evenly spaced point counts between 2/3 and 3/2 of the input's count."""
    lo, hi = math.ceil(WINDOW[0] * n_points), math.floor(WINDOW[1] * n_points)
    lo, hi = max(lo, 1), min(hi, n_voxels)
    if n_points <= 0 or hi < lo:
        return []
    return sorted(set(int(round(v)) for v in np.linspace(lo, hi, SHORTLIST)))


def check_resident(n_blocks, voxels=32768):
    need = int(n_blocks) * int(voxels) * 4
    if need > MAX_RESIDENT_BYTES:
        raise RuntimeError(f"threshold selection keeps all probabilities resident: {n_blocks} blocks need "
                           f"{need / 2 ** 20:.0f} MiB, over the budget of {MAX_RESIDENT_BYTES >> 20} MiB; "
                           f"use --thh_mode fixed")
    return need


# ---------------------------------------------------------------- device side
def _rows(p):
    from . import ops
    ops._f32(p)
    if p.dim() < 2 or p.shape[0] == 0:
        raise ValueError("p must be [blocks, ...] with at least one block")
    return p.reshape(p.shape[0], -1)


def _raise_bad(bad):
    n = int(bad.sum().item())
    if n:
        raise ValueError(f"{n} probabilities are NaN or outside [0, 1]")


def kth_largest(p, k):
    """The exact k-th largest float32 of p [B, ...]: over all blocks when k is an int (0-dim tensor back), per block
    when k is an integer tensor [B] ([B] back).  k == 0 gives +inf (nothing is >= it), k at or above the number of
    voxels gives the minimum.  Three histogram passes; the digit choice stays on the device, one sync at the end."""
    from . import ops
    p2 = _rows(p)
    B, V = p2.shape
    whole = not isinstance(k, torch.Tensor)
    if whole:
        k0 = torch.tensor([int(k)], dtype=torch.int64, device=p.device)
        n = B * V
    else:
        if k.shape != (B,) or k.dtype.is_floating_point:
            raise ValueError(f"per-block k must be an integer tensor of shape ({B},)")
        k0 = k.to(device=p.device, dtype=torch.int64)
        n = V
    if whole and int(k) < 0:
        raise ValueError("k must not be negative")
    kk = k0.clamp(1, n)
    key = torch.zeros_like(kk)
    prefix, bad0 = None, None
    for shift, nbits in PASSES:
        count, _, _, bad = ops.occ_hist(p2, shift, nbits, prefix)
        bad0 = bad if bad0 is None else bad0
        hist = count.long()
        if whole:
            hist = hist.sum(0, keepdim=True)
        digit, kk = choose_digit(hist, kk)
        key = (key << nbits) | digit
        prefix = key.to(torch.int32).expand(B).contiguous()
    _raise_bad(bad0)
    if not whole and bool((k0 < 0).any().item()):
        raise ValueError("k must not be negative")
    v = key.to(torch.int32).view(torch.float32)
    v = torch.where(k0 == 0, torch.full_like(v, math.inf), v)
    return v[0] if whole else v


def threshold_for_count(p, k):
    """The float32 t with {p > t} = {p >= v_k}: at least k voxels (more when values tie at v_k), none for k = 0."""
    return threshold_below(kth_largest(p, k))


def curve(p, gt, d2, candidates):
    """At every candidate threshold (ascending float32 values): {"count": decoded points, "tp": of them occupied in
    gt, "sse": sum of d2 over them} as int64 numpy arrays.  gt uint8 / d2 int32 hold one value per voxel of p; either
    may be None (its entry is then None).  One pass of nvf_occ_hist_edges over p, exact at every candidate."""
    from . import ops
    p2 = _rows(p)
    cand = np.asarray(candidates, np.float32).reshape(-1)
    if cand.size == 0 or np.any(np.diff(cand) < 0) or not np.all(np.isfinite(cand)):
        raise ValueError("candidates must be a non-empty ascending list of finite thresholds")
    edges = torch.from_numpy(cand).to(p.device)
    count, sum_d2, count_gt, bad = ops.occ_hist(p2, d2=None if d2 is None else d2.reshape(p2.shape),
                                                gt=None if gt is None else gt.reshape(p2.shape), edges=edges)
    _raise_bad(bad)
    out = fold_curve(count, sum_d2, count_gt)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def original_points(gt, origins):
    """The original cloud from the ground-truth grids: non-zero voxels + block origin, int64 numpy [n, 3] in the
    (block, raster) order ops.threshold_points emits."""
    idx = torch.nonzero(gt.reshape(gt.shape[0], *gt.shape[-3:]))
    org = torch.as_tensor(np.asarray(origins)).to(device=idx.device, dtype=torch.int64)
    return (idx[:, 1:] + org[idx[:, 0]]).cpu().numpy()


def choose(mode, p, origins=None, n_points=None, block_counts=None, gt=None, d2=None):
    """The encoder's threshold for p [B, 1, D, D, D] (all blocks resident).

      count        t = threshold_for_count(p, n_points) over the whole cloud.
      block-count  t_b = threshold_for_count(p, block_counts) per block (a float32 tensor [B]).
      d1           the candidate of the shortlist with the highest symmetric D1 PSNR against the original cloud
                   (gt + origins); needs gt uint8, d2 int32 (d2_from_dist) and origins.  Equal PSNR goes to the count
                   nearest n_points.  The decoded-to-original error is as exact as the distance grid: the grids of
                   preprocess.build_grids hold the distance to the nearest point of the whole cloud, synth.make_blocks
                   only that inside the block.  With no candidate inside the 2/3..3/2 window it falls back to count.

    Returns {"mode": the mode that decided, "t": float | tensor [B], "note": str | None, "candidates": list of
    {"t", "count", "psnr"} (d1 only)}."""
    from . import ops, pc_metrics
    if mode not in MODES:
        raise ValueError(f"unknown threshold mode {mode!r}")
    check_resident(p.shape[0], p[0].numel())
    if mode == "block-count":
        k = torch.as_tensor(np.asarray(block_counts)).to(device=p.device, dtype=torch.int64)
        return {"mode": mode, "t": threshold_for_count(p, k), "note": None, "candidates": []}
    n_points = int(n_points)
    if mode == "count":
        return {"mode": mode, "t": float(threshold_for_count(p, n_points).item()), "note": None, "candidates": []}
    ks = shortlist_counts(n_points, p.numel())
    cands = []
    if ks:
        ts = torch.stack([threshold_for_count(p, k) for k in ks]).cpu().numpy()
        ts = np.unique(ts[np.isfinite(ts)])
        cur = curve(p, gt, d2, ts)
        orig = original_points(gt, origins)
        lo, hi = WINDOW[0] * n_points, WINDOW[1] * n_points
        for t, cnt, sse in zip(ts.tolist(), cur["count"].tolist(), cur["sse"].tolist()):
            if cnt == 0 or not lo <= cnt <= hi or orig.shape[0] == 0:
                continue
            pts, _ = ops.threshold_points(p, float(t), None if origins is None else torch.as_tensor(np.asarray(origins)))
            back = int(pc_metrics.nearest(orig, pts.cpu().numpy(), device=p.device)[1].sum())
            mse = max(sse / cnt, back / orig.shape[0])
            cands.append({"t": float(t), "count": int(cnt), "psnr": pc_metrics.psnr(mse, 1023.0)})
    if not cands:
        r = choose("count", p, n_points=n_points)
        r["note"] = "d1: no candidate threshold decodes between 2/3 and 3/2 of the input's points; using count"
        return r
    best = min(cands, key=lambda c: (-c["psnr"], abs(c["count"] - n_points), c["t"]))
    return {"mode": mode, "t": best["t"], "note": None, "candidates": cands}
