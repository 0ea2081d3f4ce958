"""Plain numpy restatement of nvfpcc_amd/thh_select.py (sort based), for the tests."""
import numpy as np


def keys(p):
    """The sort key of float32 probabilities: the bit pattern, -0.0 folded onto +0.0."""
    k = np.ascontiguousarray(p, np.float32).view(np.uint32).astype(np.int64)
    return np.where(k == 0x80000000, 0, k)


def digit_hist(p, shift, nbits, prefix=None, d2=None, gt=None):
    """(count, sum_d2, count_gt, bad) of one block p [voxels], as nvf_occ_hist defines them."""
    k = keys(p.reshape(-1))
    ok = k <= 0x3F800000
    bad = int((~ok).sum())
    if prefix is not None and shift + nbits < 32:
        ok = ok & ((k >> (shift + nbits)) == int(prefix))
    d = ((k >> shift) & ((1 << nbits) - 1))[ok]
    n = 1 << nbits
    count = np.bincount(d, minlength=n).astype(np.int64)
    s = None if d2 is None else _int_bincount(d, d2.reshape(-1)[ok], n)
    g = None if gt is None else _int_bincount(d, (gt.reshape(-1)[ok] != 0).astype(np.int64), n)
    return count, s, g, bad


def _int_bincount(idx, w, n):
    out = np.zeros(n, np.int64)
    np.add.at(out, idx, w.astype(np.int64))
    return out


def kth_largest(p, k):
    """k-th largest float32 of the flattened p; +inf for k == 0, the minimum for k >= size."""
    v = np.sort(np.ascontiguousarray(p, np.float32).reshape(-1))[::-1]
    if k == 0:
        return np.float32(np.inf)
    return np.float32(v[min(int(k), v.size) - 1])


def threshold_for_count(p, k):
    return np.nextafter(kth_largest(p, k), np.float32(-np.inf), dtype=np.float32)


def kth_largest_blocks(p, ks):
    return np.array([kth_largest(p[b], int(k)) for b, k in enumerate(ks)], np.float32)


def threshold_for_count_blocks(p, ks):
    return np.nextafter(kth_largest_blocks(p, ks), np.float32(-np.inf), dtype=np.float32)


def curve(p, gt, d2, candidates):
    """count / tp / sse at every candidate threshold, by direct selection."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1)
    out = {"count": [], "tp": [], "sse": []}
    for t in np.asarray(candidates, np.float32):
        sel = p > t
        out["count"].append(int(sel.sum()))
        out["tp"].append(None if gt is None else int((gt.reshape(-1)[sel] != 0).sum()))
        out["sse"].append(None if d2 is None else int(d2.reshape(-1)[sel].astype(np.int64).sum()))
    return out
