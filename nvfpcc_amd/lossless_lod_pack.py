"""The `lossless_lod_pack` entry of pack.pk: the true occupancy of every leaf block coded coarse to fine, exact at 8^3,
16^3 and 32^3 from one stream.  A second, independent side pack next to `lossless_pack` (lossless_pack.py), with the
same decoder field, context function, table rule and rANS coder; include/nvf_hip.h, "scalable lossless geometry", is
the contract of the kernels (csrc/occ_hier.hip).

Pyramid of a block, from p (float32 [32^3], the eval forward's bits) with exact float comparisons only: P0 = p;
P1[c] = the maximum of the 8 children of 16^3 cell c, folded in child order as m = c0, m = (cj > m) ? cj : m;
K1[c] = min(3, children with p > 0.5); P2, K2 likewise from P1.  The children of cell (Z, Y, X) are (2Z + dz, 2Y + dy,
2X + dx), in order j = 4 dz + 2 dy + dx.  A NaN or a value outside [0, 1] anywhere in p is an input error (-0.0 counts
as +0.0): the encoder raises before it codes.

Contexts, 3 x 4 x 256 = 3072: ctx = (level * 4 + k) * 256 + occ_ctx(P_level[cell]), occ_ctx being lossless_pack's
function of the float32 bits; k = K2[c] for an 8^3 cell (level 2), K1[c] for a 16^3 cell (level 1), K1[parent(v)] for
a voxel (level 0).

Symbols of a group of G consecutive blocks, three sections in this order: section 2 = block by block all 512 cells of
the 8^3 grid in raster order; section 1 = block by block, for every OCCUPIED 8^3 cell in raster order, its 8 children in
order j; section 0 = the same from the occupied 16^3 cells to the voxels.  Occupied at a coarse level = the max-pool of
the ground truth; everything under an empty parent is known and costs no symbol.  Each section is padded to a multiple
of 64 with idle slots; symbol i of a padded section belongs to lane i % 64 at that section's step i / 64; an idle lane
neither codes nor renormalises.

Coder: lossless_pack's binary rANS exactly (64-bit states from 2^31, 32-bit words, 16-bit frequencies, symbol 1 =
(start 0, freq f1), the words of a step in ascending lane order for the decoder), ONE stream per group: the 64 states
run through sections 2, 1, 0 without a flush; the encoder walks section 0, then 1, then 2, each backwards.  A decoder
that stops after section 2 or 1 has read a prefix of the group's words and holds the exact max-pool: the input reduced
to bits - 2 or bits - 1 bits per axis.  A block emits at most 512 + 4096 + 32768 = 37376 words.

Table: lossless_pack's rule over the coded symbols only, in exact integers; a context without symbols is 32768 and never
used.  Layout, little-endian:

    byte 0          version (VERSION)
    bytes 1..2      uint16 G: blocks per group (the last group may be shorter)
    bytes 3..6      uint32 block count N
    bytes 7..8      uint16 context count (3072)
    then            384 bytes: bit c % 8 of byte c / 8 is set when context c has at least one symbol
    then            uint16 f1 of every context present, ascending, each in [1, 65535]
    then            uint32 word count of each of the ceil(N / G) groups
    then per group  64 uint64 states, then its uint32 words in the order the decoder reads them

The host half of this module needs no device; encode_occupancy / decode_occupancy run the forward and the kernels.
"""
import struct

import numpy as np
import torch

from .lossless_pack import MAX_GROUP, SPAN_GROUPS, _forward, _span, check_status as _check_status, ideal_bits, n_groups

VERSION = 1
CONTEXTS = 3072
GROUP = 64
BLOCK_WORDS = 512 + 4096 + 32768
_HEADER = struct.Struct("<BHIH")
_BITMAP = CONTEXTS // 8
_NAME = "lossless_lod_pack"


def table_from_counts(cnt, occ):
    """Per context the coded symbols and the occupied ones -> (f1 as a list of Python integers, used as a list of
    bools): clamp((2 * 65536 * occ + cnt) // (2 * cnt), 1, 65535), and 32768, unused, for a context without symbols."""
    cnt, occ = [int(v) for v in cnt], [int(v) for v in occ]
    if len(cnt) != CONTEXTS or len(occ) != CONTEXTS or any(o < 0 or o > c for c, o in zip(cnt, occ)):
        raise ValueError(f"{_NAME}: the counts are {CONTEXTS} pairs with 0 <= occupied <= symbols")
    f1 = [32768 if c == 0 else min(max((2 * 65536 * o + c) // (2 * c), 1), 65535) for c, o in zip(cnt, occ)]
    return f1, [c > 0 for c in cnt]


def size(n_blocks, group, n_words, n_used):
    """Bytes of a pack of n_blocks blocks in groups of `group`, n_words words in all, n_used contexts present."""
    return _HEADER.size + _BITMAP + 2 * int(n_used) + n_groups(n_blocks, group) * (4 + 64 * 8) + 4 * int(n_words)


def write(group, n_blocks, f1, used, states, words):
    """f1: the frequencies of the contexts present, ascending (or all 3072, of which those are taken); used: bool
    [3072]; states: uint64 [groups, 64] (or int64 holding them); words: one uint32 array per group -> bytes."""
    group, n_blocks = int(group), int(n_blocks)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"{_NAME}: group {group} outside [1, {MAX_GROUP}]")
    if not 1 <= n_blocks < 1 << 32:
        raise ValueError(f"{_NAME}: block count {n_blocks}")
    used = np.asarray(used).reshape(-1)
    if used.shape != (CONTEXTS,):
        raise ValueError(f"{_NAME}: the bitmap has {CONTEXTS} contexts")
    used = used.astype(bool)
    f1 = np.asarray(f1, np.int64).reshape(-1)
    if f1.size == CONTEXTS and int(used.sum()) != CONTEXTS:
        f1 = f1[used]
    if f1.size != int(used.sum()):
        raise ValueError(f"{_NAME}: the bitmap names {int(used.sum())} contexts, {f1.size} frequencies given")
    if f1.size and (f1.min() < 1 or f1.max() > 65535):
        raise ValueError(f"{_NAME}: the table's frequencies are in [1, 65535]")
    ng = n_groups(n_blocks, group)
    states = np.ascontiguousarray(states).view(np.uint64) if np.asarray(states).dtype == np.int64 else np.asarray(states, np.uint64)
    if states.shape != (ng, 64) or len(words) != ng:
        raise ValueError(f"{_NAME}: {n_blocks} blocks in groups of {group} are {ng} groups of 64 states")
    words = [np.ascontiguousarray(w).view(np.uint32) if np.asarray(w).dtype == np.int32 else np.asarray(w, np.uint32)
             for w in words]
    for g, w in enumerate(words):
        if w.ndim != 1 or w.size > min(group, n_blocks - g * group) * BLOCK_WORDS:
            raise ValueError(f"{_NAME}: group {g} holds more words than it has symbols")
    parts = [_HEADER.pack(VERSION, group, n_blocks, CONTEXTS), np.packbits(used, bitorder="little").tobytes(),
             f1.astype("<u2").tobytes(), np.asarray([w.size for w in words], "<u4").tobytes()]
    for g in range(ng):
        parts += [states[g].astype("<u8").tobytes(), words[g].astype("<u4").tobytes()]
    return b"".join(parts)


def read(data, n_blocks=None):
    """bytes -> {'group', 'n_blocks', 'f1' int64 [3072] (32768 where absent), 'used' bool [3072], 'nwords' int64
    [groups], 'states' uint64 [groups, 64], 'words' uint32 [total] (the groups' words back to back)}.  ValueError,
    naming the fault, on a wrong version, a truncated header, a group size or context count out of range, a bitmap
    that names more frequencies than follow, a frequency of 0, a word count no group can have, a block count other than
    `n_blocks`, and a payload that is shorter or longer than its counts say."""
    data = bytes(data)
    if len(data) < 1:
        raise ValueError(f"{_NAME}: empty")
    if data[0] != VERSION:
        raise ValueError(f"{_NAME}: version {data[0]}, this reader knows {VERSION}")
    if len(data) < _HEADER.size:
        raise ValueError(f"{_NAME}: truncated header")
    _, group, nb, nctx = _HEADER.unpack_from(data)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"{_NAME}: group size {group} outside [1, {MAX_GROUP}]")
    if nb < 1:
        raise ValueError(f"{_NAME}: no blocks")
    if n_blocks is not None and nb != int(n_blocks):
        raise ValueError(f"{_NAME}: codes {nb} blocks, the pack holds {int(n_blocks)}")
    if nctx != CONTEXTS:
        raise ValueError(f"{_NAME}: {nctx} contexts, this reader knows {CONTEXTS}")
    ng = n_groups(nb, group)
    at = _HEADER.size
    if len(data) < at + _BITMAP:
        raise ValueError(f"{_NAME}: truncated bitmap")
    used = np.unpackbits(np.frombuffer(data, np.uint8, _BITMAP, at), bitorder="little").astype(bool)
    at += _BITMAP
    n_used = int(used.sum())
    if len(data) < at + 2 * n_used + 4 * ng:
        raise ValueError(f"{_NAME}: the bitmap names {n_used} contexts and {ng} word counts follow them, "
                         f"{len(data) - at} bytes are left")
    present = np.frombuffer(data, "<u2", n_used, at).astype(np.int64)
    at += 2 * n_used
    if n_used and present.min() < 1:
        raise ValueError(f"{_NAME}: a frequency of 0 in the table")
    f1 = np.full(CONTEXTS, 32768, np.int64)
    f1[used] = present
    nwords = np.frombuffer(data, "<u4", ng, at).astype(np.int64)
    at += 4 * ng
    for g in range(ng):
        if nwords[g] > min(group, nb - g * group) * BLOCK_WORDS:
            raise ValueError(f"{_NAME}: group {g} claims {int(nwords[g])} words, more than it has symbols")
    need = size(nb, group, int(nwords.sum()), n_used)
    if len(data) != need:
        raise ValueError(f"{_NAME}: {len(data)} bytes, {need} expected for {nb} blocks, {n_used} contexts and "
                         f"{int(nwords.sum())} words")
    states, words = np.empty((ng, 64), np.uint64), []
    for g in range(ng):
        states[g] = np.frombuffer(data, "<u8", 64, at)
        at += 512
        words.append(np.frombuffer(data, "<u4", int(nwords[g]), at).astype(np.uint32))
        at += 4 * int(nwords[g])
    return {"group": group, "n_blocks": nb, "f1": f1, "used": used, "nwords": nwords, "states": states,
            "words": np.concatenate(words) if words else np.zeros(0, np.uint32)}


def lossless_lod_line(n_bytes, n_points, ideal, n_used, n_symbols, group):
    """The `[LosslessLoD]` line of encode."""
    return "[LosslessLoD] bytes: %d bpp: %.4f ideal bpp: %.4f contexts: %d symbols: %d group: %d" % (
        n_bytes, 8.0 * n_bytes / n_points, ideal / n_points, n_used, n_symbols, group)


def check_status(status):
    """ValueError naming the first group whose decoder status is not 0."""
    try:
        _check_status(status)
    except ValueError as e:
        raise ValueError(str(e).replace("lossless_pack:", _NAME + ":", 1)) from None


# ---------------------------------------------------------------- device half
@torch.no_grad()
def encode_occupancy(net, latents, gt, batch=64, group=GROUP, span_groups=SPAN_GROUPS):
    """latents [N, ch, 2, 2, 2] (rounded, on the device) and gt float32 [N, 1, 32, 32, 32] (non-zero = occupied) ->
    (lossless_lod_pack bytes, {'ideal_bits', 'f1', 'used', 'cnt', 'occ', 'contexts' (present), 'symbols' (coded),
    'gt_words': the ground truth's occupancy words int64 [N, 512], [N, 64], [N, 8] of levels 0, 1, 2 on the device}).
    The forward runs twice -- once for the table, once for the coder -- in calls of `batch` blocks, and the coder takes
    `span_groups` whole groups per launch (lossless_pack._span): memory follows the batch and the span, not the cloud.
    ValueError when a probability is NaN or outside [0, 1]."""
    from . import ops
    N, batch, group = latents.shape[0], max(int(batch), 1), int(group)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"{_NAME}: group {group} outside [1, {MAX_GROUP}]")
    if gt.shape[0] != N:
        raise ValueError(f"{_NAME}: {N} latents and {gt.shape[0]} blocks of ground truth")
    span = _span(batch, group, span_groups)
    cnt = occ = bad = None
    for lo in range(0, N, span):
        hi = min(lo + span, N)
        pyr = ops.occ_hier_pyramid(_forward(net, latents, lo, hi, batch), gt[lo:hi].contiguous(), bad)
        bad = pyr["bad"]
        cnt, occ = ops.occ_hier_hist(pyr, cnt, occ)
    if int(bad.item()):
        raise ValueError(f"{_NAME}: {int(bad.item())} probabilities are NaN or outside [0, 1]")
    cnt, occ = (t.cpu().numpy().view(np.uint64) for t in (cnt, occ))
    f1, used = table_from_counts(cnt, occ)
    f1_dev = torch.tensor(f1, dtype=torch.int32, device=latents.device)
    states, words, gt_words = [], [], []
    for lo in range(0, N, span):
        hi = min(lo + span, N)
        pyr = ops.occ_hier_pyramid(_forward(net, latents, lo, hi, batch), gt[lo:hi].contiguous())
        s, w = ops.occ_hier_encode(pyr, f1_dev, group)
        states.append(s.cpu().numpy())
        words += [x.cpu().numpy() for x in w]
        gt_words.append(pyr["gt_words"])
    pack = write(group, N, f1, used, np.concatenate(states, 0), words)
    return pack, {"ideal_bits": ideal_bits(f1, cnt, occ), "f1": f1, "used": used, "cnt": cnt, "occ": occ,
                  "contexts": int(sum(used)), "symbols": int(sum(int(c) for c in cnt)),
                  "gt_words": tuple(torch.cat([g[lv] for g in gt_words], 0) for lv in range(3))}


@torch.no_grad()
def decode_occupancy(net, latents, data, level=0, batch=64, span_groups=SPAN_GROUPS):
    """lossless_lod_pack bytes -> (occupancy words int64 [N, 512 >> 3 * level] on the device: bit k of word w of a
    block = its cell 64 w + k of the (32 >> level)^3 grid in raster order; counts int32 [N]).  level 0 is the input's
    occupancy, levels 1 and 2 its exact 2^3 and 4^3 max-pool, from a prefix of every group's words.  ValueError on a
    malformed pack (read), on one that codes another number of blocks than `latents` has, and on a stream whose decoder
    ends in a non-zero status: a read past the end of a group's words and, at level 0, a final state that is not 2^31
    or words left over."""
    from . import ops
    if level not in (0, 1, 2):
        raise ValueError(f"{_NAME}: level {level!r}, the stream holds levels 0, 1 and 2")
    side = read(data, latents.shape[0])
    N, group, dev = side["n_blocks"], side["group"], latents.device
    span = _span(max(int(batch), 1), group, span_groups)
    f1_dev = torch.from_numpy(side["f1"].astype(np.int32)).to(dev)
    states = torch.from_numpy(side["states"].view(np.int64)).to(dev)
    words = torch.from_numpy(side["words"].view(np.int32)).to(dev)
    nwords = torch.from_numpy(side["nwords"].astype(np.int32)).to(dev)
    off = np.concatenate([[0], np.cumsum(side["nwords"])])
    out_w, out_c, out_s = [], [], []
    for lo in range(0, N, span):
        hi = min(lo + span, N)
        g0, g1 = lo // group, n_groups(hi, group)
        pyr = ops.occ_hier_pyramid(_forward(net, latents, lo, hi, batch))
        w, c, s, _ = ops.occ_hier_decode(pyr, f1_dev, states[g0:g1].contiguous(), words[int(off[g0]):int(off[g1])].contiguous(),
                                         nwords[g0:g1].contiguous(), group, level)
        out_w.append(w)
        out_c.append(c)
        out_s.append(s)
    check_status(torch.cat(out_s).cpu().numpy())
    return torch.cat(out_w, 0), torch.cat(out_c, 0)


@torch.no_grad()
def points_from_words(words, counts, origins, level=0, batch=64):
    """Occupancy words of a level + counts -> int64 [n, 3] points (origin >> level) + (z, y, x) in (block, raster) order
    (numpy): the lattice of decode --lod."""
    from . import ops
    from .lossless_pack import points_from_words as points32
    if level == 0:
        return points32(words, counts, origins, batch)
    dev = words.device
    origins = torch.as_tensor(np.asarray(origins)).to(torch.int32)
    pts = []
    for lo in range(0, words.shape[0], batch):
        hi = min(lo + batch, words.shape[0])
        pts.append(ops.points_from_bits(words[lo:hi].contiguous(), counts[lo:hi].contiguous(),
                                        origins[lo:hi].to(dev).contiguous(), 32 >> level, level).cpu())
    return torch.cat(pts, 0).long().numpy()
