"""Pre-processing of a voxelised point cloud (10 bits per axis; 11 and 12 on the device route) into the three `*_l5_*.npy` files the trainer reads
(SURVEY.md section 8, row f2):

  * level-5 octree partition: the 32^3 leaf cubes in the reference's depth-first child order
    (child index = [x >= mid] + 2 [y >= mid] + 4 [z >= mid], get_octree.cpp:354-411, 598-611, 787-795) and the
    breadth-first child-occupancy bit string down to level 5 (:574-595, 797-800);
  * per-cube occupancy and distance grids: dist = Euclidean distance of every voxel of every cube to the
    nearest input point, gt_grid = (dist == 0), axes (x, y, z) (util_get_grids.py:19-46) -- the distances come
    from the gfx950 kernel nvf_nearest_dist2 instead of 30 M KD-tree queries in a Python loop.

`preprocess_device` does both on the device (csrc/pp_device.hip, 10 to 12 bits per axis) and leaves the float32 grids there for the trainer;
`write_octree_pack` / `read_octree_pack` carry the partition in pack.pk as octree bytes instead of raw origins.
"""
import numpy as np
import torch

from ._lib import lib, check, CONSTANTS

LEAF = 32
ROOT = 1024
BITS = (10, 11, 12)             # bits per axis; the leaves are the cells of level D = bits - 5


def _depth(bits):
    """D = bits - 5, the octree level of the 32^3 leaf blocks."""
    if isinstance(bits, bool) or bits not in BITS:
        raise ValueError(f"bits must be one of {BITS}, not {bits!r}")
    return int(bits) - 5


def read_ply_xyz(path):
    """Integer x y z of an ASCII PLY (extra per-vertex properties are ignored), get_octree.cpp:751-778."""
    with open(path) as f:
        n = 0
        for line in f:
            if line.startswith("element vertex"):
                n = int(line.split()[2])
            if line.strip() == "end_header":
                break
        pts = np.loadtxt(f, max_rows=n, usecols=(0, 1, 2), ndmin=2)
    return np.asarray(pts, np.int64)


def _child_path_key(cells, levels):
    """Sort key = the sequence of child indices from the root: x is the least significant bit of a level."""
    key = np.zeros(cells.shape[0], np.int64)
    for lv in range(levels):
        bit = levels - 1 - lv
        idx = ((cells[:, 0] >> bit) & 1) | (((cells[:, 1] >> bit) & 1) << 1) | (((cells[:, 2] >> bit) & 1) << 2)
        key = key * 8 + idx
    return key


def octree_level5(points):
    """Returns (origins int64 [N,3] in the reference's traversal order, subtree bit string)."""
    pts = np.asarray(points, np.int64)
    if pts.min() < 0 or pts.max() >= ROOT:
        raise ValueError("coordinates must lie in [0, 1024)")
    cells = np.unique(pts // LEAF, axis=0)                      # level-5 cells, 32 per axis
    order = np.argsort(_child_path_key(cells, 5), kind="stable")
    origins = cells[order] * LEAF
    # breadth-first occupancy: for every node of level 0..5, eight bits for its children
    bits = []
    for level in range(0, 6):
        size = ROOT >> level                                      # node edge at this level
        nodes = np.unique(pts // size, axis=0)
        nodes = nodes[np.argsort(_child_path_key(nodes, level), kind="stable")] if level else nodes
        kids = np.unique(pts // (size // 2), axis=0)
        occupied = set(map(tuple, kids.tolist()))
        for nx, ny, nz in nodes.tolist():
            for i in range(8):
                c = (2 * nx + (i & 1), 2 * ny + ((i >> 1) & 1), 2 * nz + ((i >> 2) & 1))
                bits.append("1" if c in occupied else "0")
    return origins, "".join(bits)


def octree_partition(points, bits=10):
    """octree_level5 for a cloud of `bits` bits per axis: (origins int64 [N,3] of the 32^3 leaves in traversal order,
    the breadth-first bit string of levels 0..D, D = bits - 5).  octree_partition(p, 10) equals octree_level5(p)."""
    depth = _depth(bits)
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    levels = octree_level_bytes(pts, bits)
    cells = np.unique(pts // LEAF, axis=0)
    origins = cells[np.argsort(_child_path_key(cells, depth), kind="stable")] * LEAF
    return origins, subtree_from_level_bytes(levels)


def write_origins_txt(path, origins):
    with open(path, "w") as f:
        for x, y, z in np.asarray(origins, np.int64).tolist():
            f.write(f"{x},{y},{z}\n")


def _neighbour_lists(origins):
    cells = (np.asarray(origins, np.int64) // LEAF)
    index = {tuple(c): i for i, c in enumerate(cells.tolist())}
    off, idx = [0], []
    steps = [(dx, dy, dz) for dx in range(-2, 3) for dy in range(-2, 3) for dz in range(-2, 3)]
    steps.sort(key=lambda s: s[0] * s[0] + s[1] * s[1] + s[2] * s[2])     # nearest blocks first: tight bounds early
    for cx, cy, cz in cells.tolist():
        for dx, dy, dz in steps:
            j = index.get((cx + dx, cy + dy, cz + dz))
            if j is not None:
                idx.append(j)
        off.append(len(idx))
    return np.asarray(off, np.int32), np.asarray(idx, np.int32)


def build_grids(points, origins, device="cuda"):
    """(gt_grid uint8 [N,1,32,32,32], dist float64 [N,1,32,32,32]) of util_get_grids.py:41-46, on the GPU."""
    pts = np.asarray(points, np.int64)
    origins = np.asarray(origins, np.int64)
    n = origins.shape[0]
    cell_of = {tuple(c): i for i, c in enumerate((origins // LEAF).tolist())}
    blk = np.fromiter((cell_of[tuple(c)] for c in (pts // LEAF).tolist()), np.int64, pts.shape[0])
    order = np.argsort(blk, kind="stable")
    spts = pts[order].astype(np.int32)
    blk_off = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(blk, minlength=n), out=blk_off[1:])
    nb_off, nb_idx = _neighbour_lists(origins)
    dev = torch.device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pts, d_off, d_org, d_nbo, d_nbi = t(spts), t(blk_off), t(origins.astype(np.int32)), t(nb_off), t(nb_idx)
    d2 = torch.empty((n, LEAF, LEAF, LEAF), dtype=torch.int32, device=dev)
    check(lib().nvf_nearest_dist2(d_pts.data_ptr(), d_off.data_ptr(), d_org.data_ptr(), d_nbo.data_ptr(),
                                  d_nbi.data_ptr(), d2.data_ptr(), n, torch.cuda.current_stream().cuda_stream),
          "nvf_nearest_dist2")
    d2 = d2.cpu().numpy().astype(np.float64).reshape(n, 1, LEAF, LEAF, LEAF)
    dist = np.sqrt(d2)
    return (dist == 0).astype(np.uint8), dist


def preprocess(ply_path, level=5, device="cuda"):
    """`get_octree` + `util_get_grids.py` in one call; writes the reference's five output files."""
    if level != 5:
        raise NotImplementedError("the codec is built around level-5 (32^3) leaf cubes")
    fid = ply_path.split("/")[-1][:-4]
    pts = read_ply_xyz(ply_path)
    origins, subtree = octree_level5(pts)
    write_origins_txt(f"{fid}_l5_origins.txt", origins)
    with open(f"{fid}_l5_subtree.txt", "w") as f:
        f.write(subtree)
    gt, dist = build_grids(pts, origins, device)
    np.save(f"{fid}_l5_origins", origins.astype(np.float64))       # np.loadtxt gives float64 (util_get_grids.py:16-17)
    np.save(f"{fid}_l5_gt_grid", gt)
    np.save(f"{fid}_l5_dist", dist)
    return origins, gt, dist


# ---------------------------------------------------------------- the octree as bytes (host side, <= a few thousand nodes)
# A node's eight children are one byte (bit i = child i = character i of the reference's string); the nodes of a level
# in traversal order are the cells of that level in ascending Morton code (x in the lowest bit of each level).
OCTREE_PACK_LEVELS = 5          # levels 0..4: the children of level 4 are the leaf cubes


def _morton(cells, levels):
    return _child_path_key(np.asarray(cells, np.int64), levels)


def _unmorton(codes, levels):
    codes = np.asarray(codes, np.int64)
    out = np.zeros((codes.shape[0], 3), np.int64)
    for bit in range(levels):
        for axis in range(3):
            out[:, axis] |= ((codes >> (3 * bit + axis)) & 1) << bit
    return out


def octree_level_bytes(points, bits=10):
    """The child-occupancy bytes of levels 0..D (D = bits - 5: 0..5 at 10 bits), breadth first, one `bytes` per level:
    what octree_level5's string holds, eight characters to the byte."""
    depth = _depth(bits)
    pts = np.asarray(points, np.int64).reshape(-1, 3)
    if pts.shape[0] == 0:
        raise ValueError("empty cloud")
    if pts.min() < 0 or pts.max() >= 1 << bits:
        raise ValueError(f"coordinates must lie in [0, {1 << bits})")
    codes = np.unique(_morton(pts >> 4, depth + 1))              # occupied 16^3 cells, one level below the leaves
    levels = []
    for _ in range(depth + 1):
        parents, inverse = np.unique(codes >> 3, return_inverse=True)
        b = np.zeros(parents.shape[0], np.uint8)
        np.bitwise_or.at(b, inverse, (1 << (codes & 7)).astype(np.uint8))
        levels.append(b.tobytes())
        codes = parents
    return levels[::-1]


def subtree_from_level_bytes(levels):
    """Per-level bytes -> the reference's `*_l5_subtree.txt` string."""
    return "".join("".join(map(str, np.unpackbits(np.frombuffer(b, np.uint8), bitorder="little").tolist()))
                   for b in levels)


PACK_DEPTHS = (5, 6, 7)         # the header byte: 5 for 10 bits per axis, 6 for 11, 7 for 12


def write_octree_pack(levels, depth=None):
    """The `octree_pack` entry of pack.pk: one header byte (the number D of levels that follow: 5, 6 or 7) + the bytes
    of levels 0..D-1.  `levels` is what octree_level_bytes returns (D + 1 entries, the last is not carried) or its
    first D entries with `depth` = D; five entries without `depth` are levels 0..4.  Its length times 8 is the side
    information the encoder adds to Gross bpp."""
    if depth is None:
        depth = max(len(levels) - 1, OCTREE_PACK_LEVELS)
    if depth not in PACK_DEPTHS:
        raise ValueError(f"octree_pack carries {PACK_DEPTHS} levels, not {depth}")
    levels = [bytes(b) for b in levels[:depth]]
    if len(levels) != depth:
        raise ValueError(f"octree_pack needs the bytes of levels 0..{depth - 1}")
    return bytes([depth]) + b"".join(levels)


def read_octree_pack(data):
    """octree_pack -> origins int64 [N,3] of the leaf cubes in the reference's traversal order.  Every node byte is
    read exactly once; a stream that is short, long, or holds a node without children raises ValueError."""
    data = np.frombuffer(bytes(data), np.uint8)
    if data.size < 1 or int(data[0]) not in PACK_DEPTHS:
        raise ValueError("octree_pack: unknown header byte")
    depth = int(data[0])
    codes, at = np.zeros(1, np.int64), 1
    for level in range(depth):
        n = codes.shape[0]
        if at + n > data.size:
            raise ValueError(f"octree_pack: truncated at level {level}")
        b = data[at:at + n]
        at += n
        if not b.all():
            raise ValueError(f"octree_pack: a node of level {level} has no children")
        kids = np.unpackbits(b[:, None], axis=1, bitorder="little").astype(bool)      # [n, 8], column i = child i
        codes = (codes[:, None] * 8 + np.arange(8))[kids]                            # row-major: ascending code
    if at != data.size:
        raise ValueError("octree_pack: bytes left over after the last level")
    return _unmorton(codes, depth) * LEAF


def octree_pack_from_origins(origins, bits=10):
    """The pack of a partition given by its leaf origins (the file-based encoder has nothing else)."""
    depth = _depth(bits)
    return write_octree_pack(octree_level_bytes(np.asarray(origins, np.int64), bits)[:depth], depth)


# ---------------------------------------------------------------- the whole pre-processing on the device
META_INTS = CONSTANTS["NVF_PP_META_INTS"]    # [0] N, [1] rejected points, [2..9] bytes of level 0..7, [10] nb_off[N], [11] voxels
WORK_WORDS = CONSTANTS["NVF_PP_WORK_WORDS"]


class DevicePreprocess:
    """What preprocess_device leaves on the device.  origins int32 [N,3] (traversal order), blk_off int32 [N+1],
    points int32 [P,3] sorted by block, (nb_off, nb_idx) the candidate lists, gt / dist float32 [N,1,32,32,32],
    n_points = occupied voxels, bits = bits per axis.  octree_bytes (D + 1 = bits - 4 `bytes`, level 0..D; level L
    starts at byte level_starts[L] of oct_dev) and subtree are fetched when first asked."""

    def __init__(self, origins, blk_off, points, nb_off, nb_idx, gt, dist, n_points, oct_dev, level_counts,
                 level_starts, bits=10):
        self.origins, self.blk_off, self.points, self.nb_off, self.nb_idx = origins, blk_off, points, nb_off, nb_idx
        self.gt, self.dist, self.n_points, self.bits = gt, dist, int(n_points), int(bits)
        self._oct_dev, self._level_counts = oct_dev, [int(c) for c in level_counts]
        self._level_starts = [int(s) for s in level_starts]
        self._octree_bytes = self._subtree = None

    @property
    def octree_bytes(self):
        if self._octree_bytes is None:
            raw = self._oct_dev.cpu().numpy().tobytes()
            self._octree_bytes = tuple(raw[s:s + c] for s, c in zip(self._level_starts, self._level_counts))
        return self._octree_bytes

    @property
    def subtree(self):
        if self._subtree is None:
            self._subtree = subtree_from_level_bytes(self.octree_bytes)
        return self._subtree

    def octree_pack(self):
        return write_octree_pack(self.octree_bytes)


def grids_from_d2(d2, in_place=False):
    """int32 squared distances -> (gt, dist) float32 of the same shape: dist = sqrtf(d2), gt = (d2 == 0).  in_place:
    dist takes d2's memory (d2 is gone afterwards)."""
    if not d2.is_cuda or not d2.is_contiguous() or d2.dtype != torch.int32:
        raise RuntimeError("grids_from_d2 needs a contiguous int32 tensor on the HIP device")
    dist = d2.view(torch.float32) if in_place else torch.empty(d2.shape, dtype=torch.float32, device=d2.device)
    gt = torch.empty(d2.shape, dtype=torch.float32, device=d2.device)
    if d2.numel():
        check(lib().nvf_pp_grids(d2.data_ptr(), dist.data_ptr(), gt.data_ptr(), d2.numel(),
                                 torch.cuda.current_stream().cuda_stream), "nvf_pp_grids")
    return gt, dist


def preprocess_device(points, device="cuda", bits=10):
    """octree_partition + build_grids on the device: integer points [P,3] (numpy or tensor, coordinates of `bits` bits,
    duplicates allowed) -> DevicePreprocess.  The host reads one 64-byte record (N, the count of rejected points, the
    list sizes); nothing that scales with P or with the voxels crosses the bus after the points went up.  The kernels
    are those of csrc/pp_device.hip at the leaf level D = bits - 5: sort keys are int32 at 10 bits and int64 above, and
    every buffer is sized from min(8^L, P), the most nodes level L can have."""
    depth = _depth(bits)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("preprocess_device runs on the HIP device only; there is no CPU fallback")
    t = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points))
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError("points must be an integer array of shape [P, 3]")
    npts = t.shape[0]
    if npts == 0:
        raise ValueError("empty cloud")
    if npts >= 1 << 30:
        raise ValueError("too many points")
    t = t.to(dev)
    if t.dtype != torch.int32:
        t = t.to(torch.int64).clamp(-1, 1 << bits).to(torch.int32)          # out of range stays out of range in 32 bits
    t = t.contiguous()
    caps = [min(8 ** lv, npts) for lv in range(depth + 1)]
    starts = [sum(caps[:lv]) for lv in range(depth + 1)]
    cap, words = caps[depth], 8 ** depth // 32
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream().cuda_stream
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        keys = torch.empty(npts, dtype=torch.int32 if bits == 10 else torch.int64, device=dev)
        bitmap, meta, work = i32(8 * words), i32(META_INTS), i32(WORK_WORDS)
        origins, tab, nb_off, blk_off = i32(cap, 3), i32(2 * words), i32(cap + 1), i32(cap + 1)
        oct_dev = torch.empty(sum(caps), dtype=torch.uint8, device=dev)
        spts = i32(npts, 3)
        L = lib()
        check(L.nvf_pp_keys(t.data_ptr(), npts, bits, keys.data_ptr(), bitmap.data_ptr(), meta.data_ptr(), st),
              "nvf_pp_keys")
        skeys = torch.sort(keys).values                          # plumbing: equal keys are equal points
        check(L.nvf_pp_tree(bitmap.data_ptr(), bits, npts, origins.data_ptr(), tab.data_ptr(), oct_dev.data_ptr(),
                            nb_off.data_ptr(), work.data_ptr(), meta.data_ptr(), st), "nvf_pp_tree")
        check(L.nvf_pp_blocks(skeys.data_ptr(), npts, bits, tab.data_ptr(), meta.data_ptr(), spts.data_ptr(),
                              blk_off.data_ptr(), st), "nvf_pp_blocks")
        m = meta.cpu().tolist()                                  # the one host sync of the call
        n, bad, level_counts, nb_total, voxels = m[0], m[1], m[2:depth + 3], m[10], m[11]
        if bad:
            raise ValueError(f"coordinates must lie in [0, {1 << bits}): {bad} points do not")
        origins, nb_off, blk_off = origins[:n], nb_off[:n + 1], blk_off[:n + 1]
        nb_idx = i32(nb_total)
        check(L.nvf_pp_neighbours(origins.data_ptr(), bits, tab.data_ptr(), nb_off.data_ptr(), nb_idx.data_ptr(), n, st),
              "nvf_pp_neighbours")
        d2 = i32(n, 1, LEAF, LEAF, LEAF)
        check(L.nvf_nearest_dist2(spts.data_ptr(), blk_off.data_ptr(), origins.data_ptr(), nb_off.data_ptr(),
                                  nb_idx.data_ptr(), d2.data_ptr(), n, st), "nvf_nearest_dist2")
        gt, dist = grids_from_d2(d2, in_place=True)
    return DevicePreprocess(origins, blk_off, spts, nb_off, nb_idx, gt, dist, voxels, oct_dev, level_counts, starts,
                            bits=bits)
