"""Geometry PSNR of a decoded point cloud against its reference: MPEG's D1 (point-to-point) and D2 (point-to-plane),
as pc_error defines them, on the gfx950 kernels of csrc/pc_metrics.hip and csrc/pc_sparse.hip (C ABI: include/nvf_hip.h).

Definitions.  A is the reference cloud (the original), B the test cloud (decoded).  Both hold integer coordinates in
[0, 2^bits), bits = 10 (the default), 11 or 12; anything else (non-integer or out-of-range coordinates, an empty
cloud) raises ValueError.  Points are taken as given: duplicates are not removed.

  nn_Y(p)       the point of Y with the least squared distance to p; ties go to the lowest index in Y's INPUT order.
                Squared distances are exact int32 (at most 3 * 4095^2 < 2^31).
  D1(X->Y)      mean_i |x_i - nn_Y(x_i)|^2
  D2(X->Y)      mean_i ((nn_Y(x_i) - x_i) . n_X[i])^2     (pc_error's c2p: the error projected on the query's normal)
  normals of A  the PLY's nx ny nz when given, otherwise PCA: the eigenvector of the smallest eigenvalue of the
                covariance of the k nearest points of A (the point itself included, ordered by (squared distance,
                input index), which is deterministic on integer grids where ties are everywhere); k = 12 by default,
                3 <= k <= 32.
  normals of B  n_B[i] = n_A[nn_A(b_i)] (pc_error averages over the points of A that have b_i as nearest neighbour;
                this simplified transfer makes D2(B->A) exactly the error projected on the normal at the reference point).
  symmetric     mse = max(A->B, B->A);  PSNR = 10 log10(3 peak^2 / mse), peak = 2^bits - 1 by default (the convention
                of NVFPCC's PSNR1); inf when mse == 0.  Per direction also the Hausdorff value max_i |x_i - nn_Y(x_i)|^2.

D1 equals pc_error's for clouds without duplicate points.  D2 uses pc_error's formula, but the normals of B are
transferred in the simplified way above, so D2 is not promised to match pc_error to the bit.

Index.  `index="dense"` buckets a cloud into a dense grid of 8-voxel cells over the 1024^3 volume (10 bits only);
`index="sparse"` keeps the occupied cells only, under 64- and 512-voxel parents (any bits; its memory follows the
points, not the volume).  Both give the same answers, bit for bit.  index=None means dense at 10 bits and sparse above.

The search, the normal estimation and the sums run on the GPU; there is no CPU fallback (as for every op, _lib.py).
"""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import lib, check, NvfPcSparseIndex, CONSTANTS

ROOT = 1024                # the default domain: bits = 10
CELLS = CONSTANTS["NVF_PC_CELLS"]           # the dense index
BITS = (10, 11, 12)        # bits per axis the metrics reach


def _check_index(bits, index):
    """-> True for the sparse index; ValueError on a bits / index pair there is no index for."""
    if bits not in BITS:
        raise ValueError(f"bits must be one of {BITS}, got {bits}")
    if index not in (None, "dense", "sparse"):
        raise ValueError(f"index must be None, 'dense' or 'sparse', got {index!r}")
    if index == "dense" and bits != 10:
        raise ValueError(f"index='dense' covers 10 bits per axis only, not {bits}: use index='sparse'")
    return index == "sparse" or (index is None and bits != 10)


def _points(a, what, bits=10):
    """-> int64 [n, 3] numpy, or ValueError."""
    root = 1 << bits
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{what}: expected an [n, 3] array of coordinates, got shape {a.shape}")
    if a.shape[0] == 0:
        raise ValueError(f"{what}: the cloud is empty")
    if a.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f"{what}: too many points")
    if not np.issubdtype(a.dtype, np.integer):
        if not np.issubdtype(a.dtype, np.floating) or not np.all(np.isfinite(a)) or np.any(a != np.round(a)):
            raise ValueError(f"{what}: coordinates must be integers")
    if a.min() < 0 or a.max() >= root:
        raise ValueError(f"{what}: coordinates must lie in [0, {root})")
    return a.astype(np.int64)


class _Cloud:
    """A cloud (checked by _points) on the device: xyz int32 [n, 3] in input order, the sorted cloud int32 [n, 4] (x, y, z, input index) in
    cell-key order and the cell offsets int32 [CELLS + 1] (the index layout of include/nvf_hip.h)."""

    def __init__(self, points, device):
        pts = torch.from_numpy(points).to(device=device, dtype=torch.int32)
        self.n = pts.shape[0]
        self.xyz = pts.contiguous()
        c = pts >> 3
        key = ((((c[:, 0] >> 3) << 8) | ((c[:, 1] >> 3) << 4) | (c[:, 2] >> 3)) << 9) | \
            ((c[:, 0] & 7) << 6) | ((c[:, 1] & 7) << 3) | (c[:, 2] & 7)
        order = torch.sort(key, stable=True).indices
        ids = torch.arange(self.n, device=device, dtype=torch.int32)
        self.sorted = torch.cat([pts, ids[:, None]], 1)[order].contiguous()
        self.start = torch.zeros(CELLS + 1, dtype=torch.int32, device=device)
        self.start[1:] = torch.cumsum(torch.bincount(key.long(), minlength=CELLS), 0)


def _key9(v):
    return ((v[:, 0] & 7) << 6) | ((v[:, 1] & 7) << 3) | (v[:, 2] & 7)


class _SparseCloud:
    """A cloud on the device under the sparse index of include/nvf_hip.h (NvfPcSparseIndex): xyz and the sorted cloud
    as in _Cloud but in the nested key order, start int32 [M + 1] over the M occupied cells, and for the S occupied
    super-cells mask int64 [S, 8] (the bits of uint64 words) and first int32 [S]; super_table and hyper_table are dense
    over the super- and hyper-cells of the 2^bits volume.  The sort and the two run-length scans are torch's, the
    records and tables are filled by nvf_pc_sparse_build."""

    def __init__(self, points, device, bits):
        pts = torch.from_numpy(points).to(device=device, dtype=torch.int32)
        self.n, self.bits = pts.shape[0], bits
        self.xyz = pts.contiguous()
        hb = bits - 9
        h = pts >> 9
        key = ((((h[:, 0] << (2 * hb)) | (h[:, 1] << hb) | h[:, 2]) << 18) | (_key9(pts >> 6) << 9) | _key9(pts >> 3))
        skey, order = torch.sort(key, stable=True)
        ids = torch.arange(self.n, device=device, dtype=torch.int32)
        self.sorted = torch.cat([pts, ids[:, None]], 1)[order].contiguous()
        cell_key, counts = torch.unique_consecutive(skey, return_counts=True)
        supers, cell_super = torch.unique_consecutive(cell_key >> 9, return_inverse=True)
        m, s = cell_key.numel(), supers.numel()
        self.start = torch.zeros(m + 1, dtype=torch.int32, device=device)
        self.start[1:] = torch.cumsum(counts, 0)
        self.mask = torch.empty((s, 8), dtype=torch.int64, device=device)
        self.first = torch.empty(s, dtype=torch.int32, device=device)
        self.super_table = torch.empty(1 << (3 * (bits - 6)), dtype=torch.int32, device=device)
        self.hyper_table = torch.empty(1 << (3 * hb), dtype=torch.int32, device=device)
        self.index = NvfPcSparseIndex(self.sorted.data_ptr(), self.start.data_ptr(), self.mask.data_ptr(),
                                      self.first.data_ptr(), self.super_table.data_ptr(), self.hyper_table.data_ptr(),
                                      self.n, m, s, bits)
        check(lib().nvf_pc_sparse_build(C.byref(self.index), cell_key.to(torch.int32).contiguous().data_ptr(),
                                        cell_super.to(torch.int32).contiguous().data_ptr(), _stream()),
              "nvf_pc_sparse_build")


def _cloud(points, device, bits, sparse):
    return _SparseCloud(points, device, bits) if sparse else _Cloud(points, device)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("nvfpcc_amd.pc_metrics needs a HIP device: there is no CPU fallback")
    return dev


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nearest(q, t):
    """(input index int32 [q.n], d2 int32 [q.n]) of nn_t for every point of q, on the device."""
    idx = torch.empty(q.n, dtype=torch.int32, device=q.xyz.device)
    d2 = torch.empty_like(idx)
    if isinstance(t, _SparseCloud):
        check(lib().nvf_pc_nearest_sparse(q.sorted.data_ptr(), q.n, C.byref(t.index), idx.data_ptr(), d2.data_ptr(),
                                          _stream()), "nvf_pc_nearest_sparse")
        return idx, d2
    check(lib().nvf_pc_nearest(q.sorted.data_ptr(), q.n, t.sorted.data_ptr(), t.start.data_ptr(), t.n,
                               idx.data_ptr(), d2.data_ptr(), _stream()), "nvf_pc_nearest")
    return idx, d2


def _check_knn(k, n):
    if int(k) != k or not 3 <= k <= 32:
        raise ValueError(f"knn must be an integer in [3, 32], got {k}")
    if n < k:
        raise ValueError(f"normal estimation with knn = {k} needs at least {k} points, the cloud has {n}")


def _normals(c, k, want_knn=False):
    nrm = torch.empty((c.n, 3), dtype=torch.float32, device=c.xyz.device)
    knn = torch.empty((c.n, k), dtype=torch.int32, device=c.xyz.device) if want_knn else None
    if isinstance(c, _SparseCloud):
        check(lib().nvf_pc_knn_normals_sparse(C.byref(c.index), c.xyz.data_ptr(), int(k), nrm.data_ptr(),
                                              None if knn is None else knn.data_ptr(), _stream()),
              "nvf_pc_knn_normals_sparse")
        return nrm, knn
    check(lib().nvf_pc_knn_normals(c.sorted.data_ptr(), c.start.data_ptr(), c.xyz.data_ptr(), c.n, int(k),
                                   nrm.data_ptr(), None if knn is None else knn.data_ptr(), _stream()),
          "nvf_pc_knn_normals")
    return nrm, knn


def _sums(q, t, nn_idx, normals, normals_of_target):
    """(D1 sum, max d2, D2 sum or None) of the direction q -> t."""
    dev = q.xyz.device
    ws = torch.empty(max(int(lib().nvf_pc_workspace_bytes(q.n, t.n)), 8), dtype=torch.uint8, device=dev)
    sums = torch.empty(2, dtype=torch.int64, device=dev)
    d2 = torch.empty(1, dtype=torch.float64, device=dev)
    check(lib().nvf_pc_error_sums(q.xyz.data_ptr(), q.n, t.xyz.data_ptr(), nn_idx.data_ptr(),
                                  None if normals is None else normals.data_ptr(), int(normals_of_target),
                                  sums.data_ptr(), d2.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "nvf_pc_error_sums")
    s = sums.cpu().tolist()
    return s[0], s[1], (None if normals is None else float(d2.item()))


def psnr(mse, peak=1023.0):
    return math.inf if mse == 0 else 10.0 * math.log10(3.0 * peak * peak / mse)


def nearest(query, target, device="cuda", bits=10, index=None):
    """(input index of nn_target, squared distance) for every query point: int64 numpy arrays [n_query]."""
    sparse = _check_index(bits, index)
    query, target = _points(query, "query", bits), _points(target, "target", bits)
    dev = _device(device)
    idx, d2 = _nearest(_cloud(query, dev, bits, sparse), _cloud(target, dev, bits, sparse))
    return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.int64)


def estimate_normals(points, k=12, device="cuda", return_knn=False, bits=10, index=None):
    """PCA unit normals float32 [n, 3] of the cloud (and, with return_knn, its k-NN sets int64 [n, k])."""
    sparse = _check_index(bits, index)
    points = _points(points, "points", bits)
    _check_knn(k, points.shape[0])
    dev = _device(device)
    nrm, knn = _normals(_cloud(points, dev, bits, sparse), int(k), return_knn)
    return (nrm.cpu().numpy(), knn.cpu().numpy().astype(np.int64)) if return_knn else nrm.cpu().numpy()


def geometry_psnr(ref, test, peak=None, ref_normals=None, knn=12, d2=True, device="cuda", bits=10, index=None):
    """D1 / D2 geometry PSNR of `test` (B) against `ref` (A); see the module docstring for the definitions.
    Coordinates lie in [0, 2^bits); peak=None means 2^bits - 1.

    Returns {"d1_mse", "d1_psnr", "d2_mse", "d2_psnr", "hausdorff_d2", "n_ref", "n_test"} for the symmetric values,
    plus the same keys (without the counts) under "ref_to_test" (A->B, pc_error's mse1) and "test_to_ref" (B->A,
    mse2).  With d2=False the D2 entries are None and no normals are computed."""
    sparse = _check_index(bits, index)
    ref, test = _points(ref, "ref", bits), _points(test, "test", bits)
    if peak is None:
        peak = (1 << bits) - 1
    if not float(peak) > 0 or not math.isfinite(float(peak)):
        raise ValueError(f"peak must be positive, got {peak}")
    n = None
    if d2 and ref_normals is not None:
        n = np.asarray(ref_normals, np.float32)
        if n.shape != ref.shape or not np.all(np.isfinite(n)):
            raise ValueError(f"ref_normals: expected finite [{ref.shape[0]}, 3] values, got shape {n.shape}")
    elif d2:
        _check_knn(knn, ref.shape[0])
    dev = _device(device)
    A, B = _cloud(ref, dev, bits, sparse), _cloud(test, dev, bits, sparse)
    nA = None
    if d2:
        nA = torch.from_numpy(np.ascontiguousarray(n)).to(dev) if n is not None else _normals(A, int(knn))[0]
    ab_idx, _ = _nearest(A, B)
    ba_idx, _ = _nearest(B, A)
    dirs = {}
    for name, q, t, nn, of_target in (("ref_to_test", A, B, ab_idx, 0), ("test_to_ref", B, A, ba_idx, 1)):
        s1, mx, s2 = _sums(q, t, nn, nA, of_target)
        d1_mse, d2_mse = s1 / q.n, (None if s2 is None else s2 / q.n)
        dirs[name] = {"d1_mse": d1_mse, "d1_psnr": psnr(d1_mse, peak),
                      "d2_mse": d2_mse, "d2_psnr": None if d2_mse is None else psnr(d2_mse, peak),
                      "hausdorff_d2": mx}
    a, b = dirs["ref_to_test"], dirs["test_to_ref"]
    d1_mse = max(a["d1_mse"], b["d1_mse"])
    d2_mse = None if nA is None else max(a["d2_mse"], b["d2_mse"])
    return {"d1_mse": d1_mse, "d1_psnr": psnr(d1_mse, peak),
            "d2_mse": d2_mse, "d2_psnr": None if d2_mse is None else psnr(d2_mse, peak),
            "hausdorff_d2": max(a["hausdorff_d2"], b["hausdorff_d2"]),
            "n_ref": A.n, "n_test": B.n, **dirs}


def read_ply_points(path):
    """(xyz int64 [n, 3], normals float64 [n, 3] or None) of an ASCII PLY, by the header's property names: x, y and z
    need not be the first columns; nx ny nz are returned when all three are present.  Binary PLY raises ValueError.
    nvfpcc_amd.ply_io.read_ply reads both formats, and ASCII on the device."""
    with open(path, "rb") as f:
        raw = f.read()
    if not raw.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file")
    end = raw.find(b"end_header")
    if end < 0:
        raise ValueError(f"{path}: PLY header has no end_header")
    body_start = raw.find(b"\n", end)
    header = raw[:end].decode("ascii", "replace").splitlines()
    elements = []           # [name, count, [property names]]
    fmt = None
    for line in header:
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1] if len(w) > 1 else None
        elif w[0] == "element" and len(w) == 3:
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements:
            elements[-1][2].append(w[-1])
    if fmt != "ascii":
        raise ValueError(f"{path}: only ASCII PLY is supported (format {fmt})")
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: PLY has no vertex element")
    vi = names.index("vertex")
    _, n, props = elements[vi]
    for axis in ("x", "y", "z"):
        if axis not in props:
            raise ValueError(f"{path}: vertex element has no '{axis}' property")
    lines = raw[body_start + 1:].decode("ascii").splitlines() if body_start >= 0 else []
    skip = sum(e[1] for e in elements[:vi])
    rows = [ln.split() for ln in lines[skip:skip + n]]
    if len(rows) < n or any(len(r) < len(props) for r in rows):
        raise ValueError(f"{path}: PLY holds fewer vertex values than its header declares")
    vals = np.asarray([r[:len(props)] for r in rows], np.float64).reshape(n, len(props))
    col = {p: i for i, p in enumerate(props)}
    xyz = vals[:, [col["x"], col["y"], col["z"]]]
    if not np.all(np.isfinite(xyz)) or np.any(xyz != np.round(xyz)):
        raise ValueError(f"{path}: coordinates must be integers")
    normals = vals[:, [col["nx"], col["ny"], col["nz"]]] if all(p in col for p in ("nx", "ny", "nz")) else None
    return xyz.astype(np.int64), normals
