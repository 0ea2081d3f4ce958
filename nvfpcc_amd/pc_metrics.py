"""Geometry PSNR of a decoded point cloud against its reference: MPEG's D1 (point-to-point) and D2 (point-to-plane),
as pc_error defines them, on the gfx950 kernels of csrc/pc_metrics.hip (C ABI: include/nvf_hip.h).

Definitions.  A is the reference cloud (the original), B the test cloud (decoded).  Both hold integer coordinates in
[0, 1024), the codec's domain; anything else (non-integer or out-of-range coordinates, an empty cloud) raises
ValueError.  Points are taken as given: duplicates are not removed.

  nn_Y(p)       the point of Y with the least squared distance to p; ties go to the lowest index in Y's INPUT order.
                Squared distances are exact int32 (at most 3 * 1023^2 < 2^31).
  D1(X->Y)      mean_i |x_i - nn_Y(x_i)|^2
  D2(X->Y)      mean_i ((nn_Y(x_i) - x_i) . n_X[i])^2     (pc_error's c2p: the error projected on the query's normal)
  normals of A  the PLY's nx ny nz when given, otherwise PCA: the eigenvector of the smallest eigenvalue of the
                covariance of the k nearest points of A (the point itself included, ordered by (squared distance,
                input index), which is deterministic on integer grids where ties are everywhere); k = 12 by default,
                3 <= k <= 32.
  normals of B  n_B[i] = n_A[nn_A(b_i)] (pc_error averages over the points of A that have b_i as nearest neighbour;
                this simplified transfer makes D2(B->A) exactly the error projected on the normal at the reference point).
  symmetric     mse = max(A->B, B->A);  PSNR = 10 log10(3 peak^2 / mse), peak = 1023 by default (the convention of
                NVFPCC's PSNR1); inf when mse == 0.  Per direction also the Hausdorff value max_i |x_i - nn_Y(x_i)|^2.

D1 equals pc_error's for clouds without duplicate points.  D2 uses pc_error's formula, but the normals of B are
transferred in the simplified way above, so D2 is not promised to match pc_error to the bit.

The search, the normal estimation and the sums run on the GPU; there is no CPU fallback (as for every op, _lib.py).
"""
import math

import numpy as np
import torch

from ._lib import lib, check

ROOT = 1024
CELLS = 128 ** 3           # NVF_PC_CELLS


def _points(a, what):
    """-> int64 [n, 3] numpy, or ValueError."""
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
    if a.min() < 0 or a.max() >= ROOT:
        raise ValueError(f"{what}: coordinates must lie in [0, {ROOT})")
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


def nearest(query, target, device="cuda"):
    """(input index of nn_target, squared distance) for every query point: int64 numpy arrays [n_query]."""
    query, target = _points(query, "query"), _points(target, "target")
    dev = _device(device)
    idx, d2 = _nearest(_Cloud(query, dev), _Cloud(target, dev))
    return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.int64)


def estimate_normals(points, k=12, device="cuda", return_knn=False):
    """PCA unit normals float32 [n, 3] of the cloud (and, with return_knn, its k-NN sets int64 [n, k])."""
    points = _points(points, "points")
    _check_knn(k, points.shape[0])
    dev = _device(device)
    nrm, knn = _normals(_Cloud(points, dev), int(k), return_knn)
    return (nrm.cpu().numpy(), knn.cpu().numpy().astype(np.int64)) if return_knn else nrm.cpu().numpy()


def geometry_psnr(ref, test, peak=1023, ref_normals=None, knn=12, d2=True, device="cuda"):
    """D1 / D2 geometry PSNR of `test` (B) against `ref` (A); see the module docstring for the definitions.

    Returns {"d1_mse", "d1_psnr", "d2_mse", "d2_psnr", "hausdorff_d2", "n_ref", "n_test"} for the symmetric values,
    plus the same keys (without the counts) under "ref_to_test" (A->B, pc_error's mse1) and "test_to_ref" (B->A,
    mse2).  With d2=False the D2 entries are None and no normals are computed."""
    ref, test = _points(ref, "ref"), _points(test, "test")
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
    A, B = _Cloud(ref, dev), _Cloud(test, dev)
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
    need not be the first columns; nx ny nz are returned when all three are present.  Binary PLY raises ValueError."""
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
