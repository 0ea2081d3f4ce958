"""The numpy restatement of the voxeliser's definition (nvfpcc_amd/voxelize.py): what the kernels of
csrc/voxelize.hip are held to.  numpy's elementwise float64 operations round one at a time, as the definition asks."""
import collections

import numpy as np

RefVoxelized = collections.namedtuple("RefVoxelized", "points counts lattice n_in sum_err2 max_err2")
RefLattice = collections.namedtuple("RefLattice", "bits origin step")


def fit(points, bits):
    """(bits, origin, step) of the finite points of float64 [P, 3]."""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    x = x[np.all(np.isfinite(x), 1)]
    lo, hi = x.min(0), x.max(0)
    extent = float(np.max(hi - lo))
    step = extent / float((1 << bits) - 1) if extent > 0.0 else 1.0
    return RefLattice(bits, tuple((lo + 0.0).tolist()), step)


def classify(points, lattice):
    """-> (nonfinite bool [P], outside bool [P], v = u + 0.5 float64 [P, 3])."""
    x = np.asarray(points, np.float64).reshape(-1, 3)
    o, inv = np.asarray(lattice.origin, np.float64), 1.0 / np.float64(lattice.step)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x - o
        u = t * inv
        v = u + 0.5
    nonfinite = ~np.all(np.isfinite(x), 1)
    outside = ~nonfinite & ~np.all((v >= 0.0) & (v < float(1 << lattice.bits)), 1)
    return nonfinite, outside, v


def quantize(points, lattice):
    """q int64 [P, 3] of points that are all inside."""
    nonfinite, outside, v = classify(points, lattice)
    assert not nonfinite.any() and not outside.any()
    return np.floor(v).astype(np.int64)


def to_source(q, lattice, level=0):
    o, s = np.asarray(lattice.origin, np.float64), np.float64(lattice.step) * np.float64(2.0 ** level)
    p = np.asarray(q, np.int64).astype(np.float64) * s
    return o + p


def voxelize(points, bits=10, lattice=None):
    x = np.asarray(points, np.float64).reshape(-1, 3)
    lattice = fit(x, bits) if lattice is None else RefLattice(*lattice)
    q = quantize(x, lattice)
    b = lattice.bits
    key = (q[:, 0] << (2 * b)) | (q[:, 1] << b) | q[:, 2]
    ukey, counts = np.unique(key, return_counts=True)
    mask = (1 << b) - 1
    pts = np.stack([(ukey >> (2 * b)) & mask, (ukey >> b) & mask, ukey & mask], 1)
    d = x - to_source(q, lattice)
    e = d * d
    e2 = (e[:, 0] + e[:, 1]) + e[:, 2]
    return RefVoxelized(pts.astype(np.int32), counts.astype(np.int32), lattice, x.shape[0], float(e2.sum()), float(e2.max()))
