"""The `lossless_mv_pack` entry of pack.pk: one integer motion vector per leaf block, for a version-4 `lossless_lod_pack`
(lossless_inter_pack.py) whose reference words were built with block motion compensation.  include/nvf_hip.h, "scalable
lossless geometry, motion-compensated reference", is the contract of the kernels (csrc/occ_motion.hip).

The version-4 coder only ever sees R, the reference words of this frame's blocks, and carries their digest.  Here R is
R': block b with origin o_b and vector d_b reads R'_b(v) = Ref(o_b + v - d_b), v in [0, 32)^3, where Ref is the reference
cloud (1 at its points inside [0, 2^26)^3, 0 everywhere else).  With every vector 0 this is reference_words' R whenever
the reference's points all lie under the frame's blocks.  The coder, its kernels and its bytes are untouched; a decoder
that applies other vectors stops at the version-4 digest check.  Layout, little-endian:

    byte 0          version (1)
    byte 1          radius r of the search, 1..8: every |component| <= r
    bytes 2..5      uint32 N, the block count
    then            ceil(N / 8) bytes: bit b (little bit order) set when block b's vector is not 0
    then            per set bit, ascending: three int8 (d0, d1, d2), axes in the order of the points' columns

The host half (size, write, read) needs no device.
"""
import numpy as np
import torch

VERSION = 1
MAX_RADIUS = 8
_NAME = "lossless_mv_pack"
_HEADER = 6


def size(n_blocks, moved):
    """Bytes of a pack of n_blocks blocks of which `moved` have a vector other than 0."""
    return _HEADER + (int(n_blocks) + 7) // 8 + 3 * int(moved)


def _radius(radius):
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"{_NAME}: radius {radius!r} outside 1..{MAX_RADIUS}")
    return int(radius)


def write(radius, mv):
    """radius 1..8, mv int [N, 3] (numpy or torch), every |component| <= radius -> bytes."""
    radius = _radius(radius)
    if isinstance(mv, torch.Tensor):
        mv = mv.detach().cpu().numpy()
    mv = np.asarray(mv)
    if mv.ndim != 2 or mv.shape[1] != 3 or mv.shape[0] < 1 or mv.shape[0] >= 1 << 32 or mv.dtype.kind not in "iu":
        raise ValueError(f"{_NAME}: the vectors are integers [N, 3], N >= 1")
    mv = mv.astype(np.int64)
    if np.abs(mv).max() > radius:
        b = int(np.argmax(np.abs(mv).max(1) > radius))
        raise ValueError(f"{_NAME}: block {b}'s vector {tuple(mv[b].tolist())} has a component beyond +-{radius}")
    moved = (mv != 0).any(1)
    return bytes([VERSION, radius]) + int(mv.shape[0]).to_bytes(4, "little") + \
        np.packbits(moved, bitorder="little").tobytes() + mv[moved].astype(np.int8).tobytes()


def read(data, n_blocks=None):
    """bytes -> {'radius', 'n_blocks', 'mv' int32 [N, 3]}.  ValueError, naming the fault, on a wrong version, a radius
    outside 1..8, a block count other than n_blocks, truncation, trailing bytes, bitmap bits at or above N, a listed
    vector that is 0 and a component beyond +-radius."""
    data = bytes(data)
    if not data:
        raise ValueError(f"{_NAME}: empty")
    if data[0] != VERSION:
        raise ValueError(f"{_NAME}: version {data[0]}, this reader knows {VERSION}")
    if len(data) < _HEADER:
        raise ValueError(f"{_NAME}: truncated header")
    radius, N = data[1], int.from_bytes(data[2:6], "little")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"{_NAME}: radius {radius} outside 1..{MAX_RADIUS}")
    if N < 1:
        raise ValueError(f"{_NAME}: no blocks")
    if n_blocks is not None and N != int(n_blocks):
        raise ValueError(f"{_NAME}: codes {N} blocks, the pack holds {int(n_blocks)}")
    nbitmap = (N + 7) // 8
    if len(data) < _HEADER + nbitmap:
        raise ValueError(f"{_NAME}: truncated bitmap")
    bits = np.unpackbits(np.frombuffer(data, np.uint8, nbitmap, _HEADER), bitorder="little").astype(bool)
    if bits[N:].any():
        raise ValueError(f"{_NAME}: the bitmap sets bit {N + int(np.argmax(bits[N:]))}, at or above the {N} blocks")
    moved = np.flatnonzero(bits[:N])
    want = size(N, moved.size)
    if len(data) < want:
        raise ValueError(f"{_NAME}: truncated vectors: the bitmap names {moved.size}, {(len(data) - _HEADER - nbitmap) // 3} follow whole")
    if len(data) > want:
        raise ValueError(f"{_NAME}: {len(data) - want} trailing bytes behind the {moved.size} vectors")
    vec = np.frombuffer(data, np.int8, 3 * moved.size, _HEADER + nbitmap).reshape(-1, 3).astype(np.int32)
    zero = ~(vec != 0).any(1)
    if zero.any():
        raise ValueError(f"{_NAME}: block {int(moved[np.argmax(zero)])} is listed with the vector 0")
    far = np.abs(vec).max(1, initial=0) > radius
    if far.any():
        i = int(np.argmax(far))
        raise ValueError(f"{_NAME}: block {int(moved[i])}'s vector {tuple(vec[i].tolist())} has a component beyond "
                         f"+-{radius}")
    mv = np.zeros((N, 3), np.int32)
    mv[moved] = vec
    return {"radius": radius, "n_blocks": N, "mv": mv}


def mv_line(radius, mv, n_bytes):
    """The [LosslessLoD] line of encode --lossless_mv."""
    mv = np.asarray(mv.cpu() if isinstance(mv, torch.Tensor) else mv)
    return '[LosslessLoD] motion: radius %d moved: %d of %d blocks bytes: %d' % (
        radius, int((mv != 0).any(1).sum()), mv.shape[0], n_bytes)


# ---------------------------------------------------------------- device half
def _device_int32(a, device):
    """int [n, 3], numpy or torch -> int32 on the device; what no int32 holds lies beyond any block either way."""
    a = (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).reshape(-1, 3).to(device)
    if a.dtype != torch.int32:
        big = 1 << 30
        a = a.to(torch.int64).clamp(-big, big).to(torch.int32)
    return a.contiguous()


def reference_blocks(points, device=None):
    """The reference cloud `points` (int [M, 3]) on its own blocks, on the device: (ref_own, ref_keys) of
    ops.occ_ref_blocks.  Build it once for search and compensated_words of one frame."""
    from . import ops
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) else torch.device("cuda")
    return ops.occ_ref_blocks(_device_int32(points, device))


def _reference(points, device):
    return points if isinstance(points, tuple) else reference_blocks(points, device)


def frame_words(gt, span=4096):
    """The frame's own words for search: gt float [N, 32768] (or [N, 1, 32, 32, 32]) on the device, non-zero = occupied
    -> int64 [N, 512], gt_words[0] of ops.occ_hier_pyramid with the ground truth as its own field, `span` blocks a call."""
    from . import ops
    chunks = (gt[lo:lo + span].contiguous() for lo in range(0, gt.shape[0], span))
    return torch.cat([ops.occ_hier_pyramid(g, g)["gt_words"][0] for g in chunks], 0)


def compensated_words(points, origins, mv, device=None):
    """R': the reference cloud `points` (int [M, 3], or the pair reference_blocks made of it) fetched under the vectors
    mv (int [N, 3], |component| <= 8) for the blocks at `origins` (int [N, 3]) -> words int64 [N, 512] on the device, in
    the format of lossless_inter_pack.reference_words.  ValueError on a vector beyond +-8."""
    from . import ops
    ref_own, ref_keys = _reference(points, device)
    dev = ref_own.device
    org, mv = _device_int32(origins, dev), _device_int32(mv, dev)
    if mv.shape != org.shape:
        raise ValueError(f"{_NAME}: {mv.shape[0]} vectors for {org.shape[0]} blocks")
    out, bad = [], 0
    for lo in range(0, org.shape[0], ops.OCC_HIER_MAX_BATCH):
        words, status = ops.occ_mv_words(ref_own, ref_keys, org[lo:lo + ops.OCC_HIER_MAX_BATCH],
                                         mv[lo:lo + ops.OCC_HIER_MAX_BATCH])
        out.append(words)
        bad += int(status.item())
    if bad:
        raise ValueError(f"{_NAME}: {bad} vectors have a component beyond +-{MAX_RADIUS}")
    return out[0] if len(out) == 1 else torch.cat(out, 0)


def search(gt_words0, points, origins, radius, device=None):
    """The vectors of the frame whose own words are gt_words0 (int64 [N, 512] on the device: gt_words[0] of
    ops.occ_hier_pyramid) against the reference cloud `points` (or its reference_blocks pair): the exhaustive Hamming
    search of `radius` -> (mv int32 [N, 3], cost int32 [N, 2] = (the winner's distance, the distance at 0)), on the device."""
    from . import ops
    radius = _radius(radius)
    ref_own, ref_keys = _reference(points, gt_words0.device if device is None else device)
    org = _device_int32(origins, ref_own.device)
    if gt_words0.shape[0] != org.shape[0]:
        raise ValueError(f"{_NAME}: words of {gt_words0.shape[0]} blocks, {org.shape[0]} origins")
    got = [ops.occ_mv_search(gt_words0[lo:lo + ops.OCC_HIER_MAX_BATCH].contiguous(), ref_own, ref_keys,
                             org[lo:lo + ops.OCC_HIER_MAX_BATCH], radius)
           for lo in range(0, org.shape[0], ops.OCC_HIER_MAX_BATCH)]
    return tuple(g[0] if len(got) == 1 else torch.cat(g, 0) for g in zip(*got))
