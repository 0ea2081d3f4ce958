"""CPU oracle of nvfpcc_amd.pc_metrics (scipy cKDTree + numpy), with the same definitions and tie-break: neighbours
ordered by (exact integer squared distance, input index)."""
import math

import numpy as np
from scipy.spatial import cKDTree


def ordered_neighbours(query, target, k):
    """(idx, d2) int64 [n, k]: the k points of `target` first in (d2, input index) order for every query point.
    The tree is asked for more neighbours until every tie at the k-th distance is inside the answer."""
    q, t = np.asarray(query, np.int64), np.asarray(target, np.int64)
    tree = cKDTree(t)
    out_i = np.empty((q.shape[0], k), np.int64)
    out_d = np.empty((q.shape[0], k), np.int64)
    todo = np.arange(q.shape[0])
    m = min(t.shape[0], k + 8)
    while todo.size:
        _, idx = tree.query(q[todo], k=m)
        idx = idx.reshape(todo.size, m)
        d2 = ((t[idx] - q[todo][:, None, :]) ** 2).sum(-1)
        order = np.lexsort((idx, d2), axis=-1)
        idx, d2 = np.take_along_axis(idx, order, 1), np.take_along_axis(d2, order, 1)
        done = (d2[:, -1] > d2[:, k - 1]) | (m == t.shape[0])
        out_i[todo[done]], out_d[todo[done]] = idx[done, :k], d2[done, :k]
        todo = todo[~done]
        m = min(t.shape[0], 2 * m)
    return out_i, out_d


def nearest(query, target):
    """(idx, d2) of nn_target, ties to the lowest index."""
    i, d = ordered_neighbours(query, target, 1)
    return i[:, 0], d[:, 0]


def pca_normals(points, knn_idx):
    """Unit eigenvectors of the smallest eigenvalue (numpy eigh) of each neighbourhood, and the relative gap
    (lambda_1 - lambda_0) / lambda_2 between the two smallest eigenvalues."""
    p = np.asarray(points, np.float64)[knn_idx]                     # [n, k, 3]
    c = p - p.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))
    gap = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)
    return v[:, :, 0], gap


def psnr(mse, peak=1023.0):
    return math.inf if mse == 0 else 10.0 * math.log10(3.0 * peak * peak / mse)


def geometry_psnr(ref, test, ref_normals, peak=1023.0):
    """Symmetric and per-direction D1 / D2 with the given normals of the reference (float64 math throughout)."""
    a, b = np.asarray(ref, np.int64), np.asarray(test, np.int64)
    na = np.asarray(ref_normals, np.float64)
    ab, _ = nearest(a, b)
    ba, _ = nearest(b, a)
    ea, eb = b[ab] - a, a[ba] - b
    d1a, d1b = (ea ** 2).sum(1), (eb ** 2).sum(1)
    d2a = ((ea * na).sum(1) ** 2).mean()
    d2b = ((eb * na[ba]).sum(1) ** 2).mean()
    r = {"ref_to_test": {"d1_mse": d1a.sum() / a.shape[0], "d2_mse": d2a, "hausdorff_d2": int(d1a.max())},
         "test_to_ref": {"d1_mse": d1b.sum() / b.shape[0], "d2_mse": d2b, "hausdorff_d2": int(d1b.max())}}
    for v in r.values():
        v["d1_psnr"], v["d2_psnr"] = psnr(v["d1_mse"], peak), psnr(v["d2_mse"], peak)
    x, y = r["ref_to_test"], r["test_to_ref"]
    r.update(d1_mse=max(x["d1_mse"], y["d1_mse"]), d2_mse=max(x["d2_mse"], y["d2_mse"]),
             hausdorff_d2=max(x["hausdorff_d2"], y["hausdorff_d2"]), n_ref=a.shape[0], n_test=b.shape[0])
    r["d1_psnr"], r["d2_psnr"] = psnr(r["d1_mse"], peak), psnr(r["d2_mse"], peak)
    return r
