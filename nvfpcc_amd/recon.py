"""Occupancy grids -> point cloud (reconstruction half of encode()/decode(), NVFPCC.py:501-554, 624-650).

The reference thresholds with MinkowskiEngine (to_sparse + pruning) one block at a time and writes the
PLY through open3d; here the decoder runs batched (bit-identical to batch 1 by construction of the
kernels), a ballot-compaction kernel emits origin + (z, y, x) in raster order, and the PLY writer is ours.
"""
import numpy as np
import torch

from . import ops


def eval_batches(net, latents, batch, lod=0, q=2, return_p=False):
    """The eval forward over latents [N,ch,2,2,2], at most max(batch, 1) blocks a call: yields (lo, hi, out) with out =
    net.reconstruct(latents[lo:hi], q) at lod 0 and net.reconstruct_lod(latents[lo:hi], lod, q, return_p) at lod 1 | 2.
    Nothing is gathered or moved, and gradients are the caller's business."""
    batch = max(int(batch), 1)
    for lo in range(0, latents.shape[0], batch):
        hi = min(lo + batch, latents.shape[0])
        x = latents[lo:hi].contiguous()
        yield lo, hi, net.reconstruct_lod(x, lod, q, return_p) if lod else net.reconstruct(x, q)


@torch.no_grad()
def reconstruct_points(net, latents, origins, thh, batch=64, q=2, block_counts=None, thh_out=None):
    """latents [N,ch,2,2,2] (already rounded) on the device -> (int64 [n,3] points, per-block counts).

    Voxel coordinate order inside a block is (d0, d1, d2) of the 32^3 grid, the order
    torch.nonzero(out[b, 0] > thh) yields; points = coords + origins[b] (NVFPCC.py:535-538, 635-637).

    Per-block thresholds (optional): thh may be a float32 tensor [N], one threshold per block; or block_counts (int
    [N]) asks for them from the probabilities themselves -- block b keeps its block_counts[b] most probable voxels,
    ties included (thh_select.threshold_for_count; thh is then ignored).  thh_out, a list, receives the per-block
    thresholds used, batch by batch."""
    dev = latents.device
    origins = torch.as_tensor(np.asarray(origins)).to(torch.int32)
    if block_counts is not None:
        from .thh_select import threshold_for_count
        block_counts = torch.as_tensor(np.asarray(block_counts)).to(device=dev, dtype=torch.int64)
    elif isinstance(thh, torch.Tensor):
        thh = thh.to(device=dev, dtype=torch.float32)
    pts, counts = [], []
    for lo, hi, out in eval_batches(net, latents, batch, q=q):
        t = thh
        if block_counts is not None:
            t = threshold_for_count(out, block_counts[lo:hi])
        elif isinstance(thh, torch.Tensor):
            t = thh[lo:hi].contiguous()
        if thh_out is not None and isinstance(t, torch.Tensor):
            thh_out.append(t)
        p, c = ops.threshold_points(out, t, origins[lo:hi].to(dev))
        pts.append(p.cpu())
        counts.append(c.cpu())
    return torch.cat(pts, 0).long().numpy(), torch.cat(counts, 0).numpy()


@torch.no_grad()
def reconstruct_points_lod(net, latents, origins, lod, thh, batch=64, q=2):
    """reconstruct_points at a coarser level of detail: lod 1 = the 16^3 head (conv1_cls), lod 2 = the 8^3 head
    (conv0_cls).  The trunk stops at the activation the head reads (Net.reconstruct_lod) and ops.head_points turns it
    into points on the lattice of `bits - lod` bits per axis: (origins[b] >> lod) + (z, y, x) of the coarse grid, in
    (block, z, y, x) order.  thh: a float, or a float32 tensor [N] (one per block).
    -> (int64 [n,3] points, per-block counts)."""
    dev = latents.device
    origins = torch.as_tensor(np.asarray(origins)).to(torch.int32)
    if isinstance(thh, torch.Tensor):
        thh = thh.to(device=dev, dtype=torch.float32)
    w_fwd, bias = net.lod_head_params(lod)
    pts, counts = [], []
    for lo, hi, x in eval_batches(net, latents, batch, lod, q):
        t = thh[lo:hi].contiguous() if isinstance(thh, torch.Tensor) else thh
        p, c = ops.head_points(x, w_fwd, bias, t, origins[lo:hi].to(dev), lod)
        pts.append(p.cpu())
        counts.append(c.cpu())
    return torch.cat(pts, 0).long().numpy(), torch.cat(counts, 0).numpy()


def reduce_to_lattice(points, lod):
    """A cloud on the lattice of a coarser level: every coordinate >> lod, duplicates removed (rows sorted, as
    numpy.unique gives them).  Normals and other columns do not survive the reduction: pass the xyz columns."""
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("reduce_to_lattice takes [n, 3] coordinates")
    pts = np.round(pts).astype(np.int64)
    if pts.size and pts.min() < 0:
        raise ValueError("coordinates must not be negative")
    return np.unique(pts >> int(lod), axis=0)


def write_ply_ascii(path, points):
    """ASCII PLY with double x/y/z, the layout open3d writes for write_ascii=True (NVFPCC.py:554, 650)."""
    pts = np.round(np.asarray(points, np.float64))
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment Created by nvfpcc_amd\n")
        f.write(f"element vertex {pts.shape[0]}\nproperty double x\nproperty double y\nproperty double z\nend_header\n")
        for x, y, z in pts:
            f.write(f"{x:.0f} {y:.0f} {z:.0f}\n")


def read_ply_ascii(path):
    with open(path) as f:
        n = 0
        for line in f:
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            if line.strip() == "end_header":
                break
        if n == 0:
            return np.zeros((0, 3), np.float64)
        return np.loadtxt(f, dtype=np.float64).reshape(n, -1)[:, :3]
