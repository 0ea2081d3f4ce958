"""numpy reference of the motion-compensated reference words (include/nvf_hip.h "scalable lossless geometry,
motion-compensated reference", csrc/occ_motion.hip), by a dense volume per block and nothing else:

    Ref(q) = 1 when the reference cloud holds q, q in [0, 2^26)^3, else 0
    R'_b(v) = Ref(o_b + v - d_b), v in [0, 32)^3

Occupancies travel as bool [nb, 32768] in raster order (v0, v1, v2) here and as words (H.words_of) on the device."""
import itertools

import numpy as np

from tests import occ_hier_ref as H

VOX = H.VOX
COORD = 1 << 26
MAX_RADIUS = 8


def in_range(points):
    points = np.asarray(points, np.int64).reshape(-1, 3)
    return points[((points >= 0) & (points < COORD)).all(1)]


def volume(points, lo, n):
    """Ref over the cube [lo, lo + n)^3 (lo int [3]) as bool [n, n, n]; points already in_range."""
    rel = points - np.asarray(lo, np.int64)
    rel = rel[((rel >= 0) & (rel < n)).all(1)]
    out = np.zeros((n, n, n), bool)
    out[tuple(rel.T)] = True
    return out


def compensated(points, origins, mv):
    """points int [M, 3], origins int [nb, 3], mv int [nb, 3] -> R' bool [nb, 32768]."""
    points = in_range(points)
    origins, mv = np.asarray(origins, np.int64).reshape(-1, 3), np.asarray(mv, np.int64).reshape(-1, 3)
    assert origins.shape == mv.shape and np.abs(mv).max(initial=0) <= MAX_RADIUS
    return np.stack([volume(points, o - d, 32).reshape(VOX) for o, d in zip(origins, mv)])


def vectors(r):
    """Every vector of the cube [-r, r]^3 in lexicographic order."""
    return list(itertools.product(range(-r, r + 1), repeat=3))


def costs(gt_block, points, origin, r):
    """The Hamming distance of one block (bool [32768]) to its window under every vector of vectors(r) -> int [n]."""
    g = np.asarray(gt_block).astype(bool).reshape(32, 32, 32)
    w = volume(points, np.asarray(origin, np.int64) - r, 32 + 2 * r)       # w[i] = Ref(o - r + i)
    return np.asarray([np.count_nonzero(g ^ w[r - d0:r - d0 + 32, r - d1:r - d1 + 32, r - d2:r - d2 + 32])
                       for d0, d1, d2 in vectors(r)])


def search(gt, points, origins, r):
    """gt bool [nb, 32768] -> (mv int [nb, 3], cost int [nb, 2] = (the winner's distance, the distance at 0)): the smallest
    distance, then the smaller d0^2 + d1^2 + d2^2, then the lexicographically smaller (d0, d1, d2)."""
    assert 1 <= r <= MAX_RADIUS
    points = in_range(points)
    origins = np.asarray(origins, np.int64).reshape(-1, 3)
    vs = vectors(r)
    mv, cost = [], []
    for g, o in zip(np.asarray(gt).reshape(-1, VOX), origins):
        c = costs(g, points, o, r)
        best = min(range(len(vs)), key=lambda i: (int(c[i]), sum(x * x for x in vs[i]), vs[i]))
        mv.append(vs[best])
        cost.append((int(c[best]), int(c[vs.index((0, 0, 0))])))
    return np.asarray(mv, np.int64).reshape(-1, 3), np.asarray(cost, np.int64).reshape(-1, 2)


def cloud_of(gt, origins):
    """bool [nb, 32768] on the blocks at origins -> points int64 [M, 3] in (block, raster) order."""
    nz = np.argwhere(np.asarray(gt).reshape(-1, 32, 32, 32))
    return nz[:, 1:] + np.asarray(origins, np.int64)[nz[:, 0]]
