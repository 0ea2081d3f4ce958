"""A group of frames (GoF) under one shared decoder: frame names, the dataset of several clouds, and the framing of
a pack that holds several frames under one `net_weight_pack`.

The decoder's weights are most of a pack; a sequence's frames show the same surfaces.  One decoder is fitted to all
blocks of F frames (the training step works over independent 32^3 blocks and does not care which cloud a block came
from), its bits are divided by the points of all frames, and each frame pays only for its own latents and side packs.

    {'net_weight_pack': <as in a plain pack, once>,
     'gof_pack': version 1 | uint16 F | uint32 first frame number | F x (uint32 leaf blocks, uint32 points),
     'frames': [frame_pack_0, ..., frame_pack_{F-1}]}

A frame_pack is the plain pack of that frame without its first key, and `extract` puts the key back: a frame inside a
group is coded by the same code, to the same bytes, as that frame coded alone under the same weights.  Nothing here
touches the device besides the tensors a dataset is handed.
"""
import contextlib
import io
import os
import re
import struct

import numpy as np
import torch

from .dataloader import LoadedVoxelDataset

VERSION = 1
_HEAD = struct.Struct('<BHI')       # version, F, first frame number
_FRAME = struct.Struct('<II')       # leaf blocks, points
_CONVERSION = re.compile(r'%(0\d+)?d')


def frame_names(pattern, start, count, needs=None):
    """The `count` file names `pattern % n`, n = start .. start + count - 1.  `pattern` holds exactly one integer
    conversion (%d or %0<n>d) and no other '%'.  Every frame's files must exist: the name itself, or what `needs(name)`
    lists (the `*_l5_*.npy` triple of a cloud that is not read itself).  ValueError names the pattern, or the first file
    that is missing."""
    if not isinstance(pattern, str) or len(_CONVERSION.findall(pattern)) != 1 or _CONVERSION.sub('', pattern).count('%'):
        raise ValueError(f"{pattern!r} is no frame pattern: it must hold exactly one %d or %0<n>d and no other '%'")
    if int(count) < 1:
        raise ValueError(f"{pattern!r}: a group holds at least one frame, not {count}")
    if int(start) < 0:
        raise ValueError(f"{pattern!r}: the first frame number is {start}, below 0")
    names = [pattern % n for n in range(int(start), int(start) + int(count))]
    for name in names:
        for fn in ([name] if needs is None else needs(name)):
            if not os.path.isfile(fn):
                raise ValueError(f"{fn}: no such file (frame {name} of {pattern!r})")
    return names


def npy_triple(name):
    """The three `*_l5_*.npy` files next to a cloud's name, in the order LoadedVoxelDataset takes them."""
    return [f'{name[:-4]}_l5_{k}.npy' for k in ('origins', 'gt_grid', 'dist')]


class GofDataset(torch.utils.data.Dataset):
    """The blocks of several frames as one dataset with the interface train() uses.  Blocks are frame-major and keep,
    inside a frame, the order of that frame's own dataset; N_leaf and N are the sums.  frame_ranges (int64 [F + 1] block
    offsets) and frame_points ([F]) say where each frame lies; frame(k) is a view of frame k."""
    MAGIC = LoadedVoxelDataset.MAGIC

    def __init__(self, frames, shuffle=True, pres=None):
        super().__init__()
        frames = list(frames)
        if not frames:
            raise ValueError("a group holds at least one frame")
        self.shuffle = shuffle
        self.pres = list(pres) if pres is not None else [None] * len(frames)
        leaves = [int(f.N_leaf) for f in frames]
        self.frame_ranges = np.concatenate([[0], np.cumsum(leaves)]).astype(np.int64)
        self.frame_points = np.asarray([f.N for f in frames])
        self.N_leaf = int(self.frame_ranges[-1])
        self.N = self.frame_points.sum()
        one = len(frames) == 1
        self.origins = frames[0].origins if one else np.concatenate([f.origins for f in frames], 0)
        if all("_resident" in f.__dict__ for f in frames):      # device-resident frames: one tensor pair, cut into views
            gts, dists = zip(*[f._resident for f in frames])
            self._resident = (gts[0], dists[0]) if one else (torch.cat(gts, 0), torch.cat(dists, 0))
            if not one:
                for k, pre in enumerate(self.pres):             # the frames' own grids become views of the group's
                    lo, hi = self.frame_ranges[k:k + 2]
                    frames[k]._resident = (self._resident[0][lo:hi], self._resident[1][lo:hi])
                    if pre is not None:
                        pre.gt, pre.dist = frames[k]._resident
        else:
            self._host = frames if not one else None
            if one:
                self.gt_grid, self.dist = frames[0].gt_grid, frames[0].dist
        print(f"[data] {self.N_leaf} leaf blocks, {self.N} points")

    def __getattr__(self, name):
        # reached only when the attribute is missing: gt_grid / dist are built on first use
        if name in ("gt_grid", "dist"):
            if "_resident" in self.__dict__:
                t = self._resident[0 if name == "gt_grid" else 1]
                value = t.cpu().numpy().astype(np.uint8) if name == "gt_grid" else t.cpu().numpy()
            elif self.__dict__.get("_host"):
                value = np.concatenate([getattr(f, name) for f in self._host], 0)
                for k, f in enumerate(self._host):              # one copy on the host: the frames keep views of it
                    f.__dict__[name] = value[self.frame_ranges[k]:self.frame_ranges[k + 1]]
            else:
                raise AttributeError(name)
            self.__dict__[name] = value
            return value
        raise AttributeError(name)

    def frame(self, k):
        """Dataset view of frame k: slices of the group's arrays along dim 0, no copy; `pre` is that frame's
        DevicePreprocess when it has one."""
        if not 0 <= k < len(self.frame_points):
            raise ValueError(f"frame {k} of a group of {len(self.frame_points)}")
        lo, hi = int(self.frame_ranges[k]), int(self.frame_ranges[k + 1])
        v = LoadedVoxelDataset.__new__(LoadedVoxelDataset)
        torch.utils.data.Dataset.__init__(v)
        v.shuffle = self.shuffle
        v.origins = self.origins[lo:hi]
        v.N_leaf = hi - lo
        v.N = self.frame_points[k]
        v.pre = self.pres[k]
        if "_resident" in self.__dict__:
            v._resident = (self._resident[0][lo:hi], self._resident[1][lo:hi])
        else:
            v.gt_grid, v.dist = self.gt_grid[lo:hi], self.dist[lo:hi]
        return v

    permute = LoadedVoxelDataset.permute
    __getitem__ = LoadedVoxelDataset.__getitem__
    get_all = LoadedVoxelDataset.get_all
    to_device = LoadedVoxelDataset.to_device
    epoch_order = LoadedVoxelDataset.epoch_order

    def __len__(self):
        return self.N_leaf


def quiet(fn, *args, **kw):
    """fn(*args, **kw) with its printed lines dropped: a frame's own [data] line belongs to the frame coded alone."""
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def write_gof_pack(start, n_leaf, n_points):
    """gof_pack bytes: version | uint16 F | uint32 first frame number | F x (uint32 leaf blocks, uint32 points)."""
    n_leaf, n_points = [int(x) for x in n_leaf], [int(x) for x in n_points]
    if len(n_leaf) != len(n_points) or not 1 <= len(n_leaf) <= 0xFFFF:
        raise ValueError(f"gof_pack: {len(n_leaf)} leaf counts and {len(n_points)} point counts; a group holds 1 to 65535 frames")
    if not 0 <= int(start) <= 0xFFFFFFFF or any(not 0 <= x <= 0xFFFFFFFF for x in n_leaf + n_points):
        raise ValueError("gof_pack: a frame number or a count does not fit 32 bits")
    return _HEAD.pack(VERSION, len(n_leaf), int(start)) + b''.join(_FRAME.pack(a, b) for a, b in zip(n_leaf, n_points))


def read_gof_pack(data):
    """-> {'start': first frame number, 'n_leaf': [F], 'n_points': [F]}.  ValueError with its reason on a wrong version,
    a wrong length or F == 0."""
    data = bytes(data)
    if len(data) < _HEAD.size:
        raise ValueError(f"gof_pack: {len(data)} bytes are shorter than the {_HEAD.size}-byte header")
    version, F, start = _HEAD.unpack_from(data)
    if version != VERSION:
        raise ValueError(f"gof_pack: version {version}, this decoder reads version {VERSION}")
    if F == 0:
        raise ValueError("gof_pack: a group of 0 frames")
    if len(data) != _HEAD.size + _FRAME.size * F:
        raise ValueError(f"gof_pack: {len(data)} bytes, {F} frames take {_HEAD.size + _FRAME.size * F}")
    rows = [_FRAME.unpack_from(data, _HEAD.size + _FRAME.size * k) for k in range(F)]
    return {'start': start, 'n_leaf': [r[0] for r in rows], 'n_points': [r[1] for r in rows]}


def frame_leaves(frame_pack):
    """Leaf blocks a frame pack says it holds: the rows of its origins, or the leaves of its octree_pack."""
    if 'octree_pack' in frame_pack:
        from .preprocess import read_octree_pack
        return int(read_octree_pack(frame_pack['octree_pack']).shape[0])
    return int(len(frame_pack['origins']))


def extract(total_pack, k):
    """Frame k of a group as a plain pack: {'net_weight_pack': W, **frames[k]}.  Reads nothing of another frame.
    ValueError when k is out of range or the frame's leaf count disagrees with gof_pack."""
    info = read_gof_pack(total_pack['gof_pack'])
    frames = total_pack['frames']
    F = len(info['n_leaf'])
    if len(frames) != F:
        raise ValueError(f"gof_pack names {F} frames, the pack holds {len(frames)}")
    if not isinstance(k, (int, np.integer)) or not 0 <= k < F:
        raise ValueError(f"frame index {k} outside the group's 0 .. {F - 1}")
    n = frame_leaves(frames[k])
    if n != info['n_leaf'][k]:
        raise ValueError(f"frame index {k} holds {n} leaf blocks, gof_pack says {info['n_leaf'][k]}")
    return {'net_weight_pack': total_pack['net_weight_pack'], **frames[k]}


SIDE_KEYS = ('thh_pack', 'octree_pack', 'lod_pack', 'lossless_pack', 'lossless_lod_pack', 'vox_pack')


def frame_bits(frame_pack):
    """(latent bits, side bits) of a frame pack, with the terms of the plain encoder's Gross bpp line."""
    latent = 8 * len(frame_pack['latent_pack']['latent_byte_stream'])
    return latent, sum(8 * len(frame_pack.get(k, b'')) for k in SIDE_KEYS)


def account(total_pack):
    """The group's bits from its pack: {'frames', 'points', 'weight_bits', 'latent_bits', 'side_bits', 'gof_bits',
    'own_bpp': [F] (latent + side bits of a frame over its points), 'gross_bpp'}; gross = (weights + latents + sides +
    gof_pack) / points."""
    info = read_gof_pack(total_pack['gof_pack'])
    bits = [frame_bits(f) for f in total_pack['frames']]
    points = int(sum(info['n_points']))
    # (a latents-only group, nvfpcc_amd.pframe: its 33-byte ref_pack stands where the weights' stream would)
    w = 8 * (len(total_pack['net_weight_pack']['bit_stream']) if 'net_weight_pack' in total_pack else len(total_pack['ref_pack']))
    lat, side, g = sum(b[0] for b in bits), sum(b[1] for b in bits), 8 * len(total_pack['gof_pack'])
    return {'frames': len(bits), 'points': points, 'weight_bits': w, 'latent_bits': lat, 'side_bits': side, 'gof_bits': g,
            'own_bpp': [(b[0] + b[1]) / float(n) for b, n in zip(bits, info['n_points'])],
            'gross_bpp': (w + lat + side + g) / float(points)}


def frame_line(number, points, blocks, latent_bits, side_bits):
    return '[Frame %04d] points: %d blocks: %d latent bytes: %d side bytes: %d own bpp: %.4f' % (
        number, points, blocks, latent_bits // 8, side_bits // 8, (latent_bits + side_bits) / float(points))


def gof_lines(total_pack):
    """The two closing lines of encode --gof."""
    a = account(total_pack)
    return ['[GoF] frames: %d points: %d weight bytes: %d latent bytes: %d side bytes: %d' % (
        a['frames'], a['points'], a['weight_bits'] // 8, a['latent_bits'] // 8, a['side_bits'] // 8),
        '[Latent code] Gross bpp: %.4f' % a['gross_bpp']]
