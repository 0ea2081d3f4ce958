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

The framing, the span loops, the table rule and points_from_words are lossless_pack's; this module holds the table
section (bitmap + present frequencies) and the coder calls.  The host half needs no device; encode_occupancy /
decode_occupancy run the forward and the kernels.
"""
import numpy as np
import torch

from . import lossless_pack as _lp
from .lossless_pack import SPAN_GROUPS, ideal_bits, points_from_words  # noqa: F401  (points_from_words: this pack's too)

VERSION = 1
CONTEXTS = 3072
GROUP = 64
BLOCK_WORDS = 512 + 4096 + 32768
_BITMAP = CONTEXTS // 8
_NAME = "lossless_lod_pack"
_KIND = _lp.Kind(_NAME, VERSION, CONTEXTS, BLOCK_WORDS)


def table_from_counts(cnt, occ):
    """Per context the coded symbols and the occupied ones -> (f1 as a list of Python integers, used as a list of
    bools): lossless_pack's rule (table_rule); a context without symbols is 32768 and unused."""
    return _lp.table_rule(_KIND, "symbols", cnt, occ)


def size(n_blocks, group, n_words, n_used):
    """Bytes of a pack of n_blocks blocks in groups of `group`, n_words words in all, n_used contexts present."""
    return _lp.frame_size(_BITMAP + 2 * int(n_used), n_blocks, group, n_words)


def write(group, n_blocks, f1, used, states, words):
    """f1: the frequencies of the contexts present, ascending (or all 3072, of which those are taken); used: bool
    [3072]; states: uint64 [groups, 64] (or int64 holding them); words: one uint32 array per group -> bytes."""
    group, n_blocks = _lp.frame_counts(_KIND, group, n_blocks)
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
    table = np.packbits(used, bitorder="little").tobytes() + f1.astype("<u2").tobytes()
    return _lp.frame_write(_KIND, group, n_blocks, table, states, words)


def _read_table(data, at, tail):
    if len(data) < at + _BITMAP:
        raise ValueError(f"{_NAME}: truncated bitmap")
    used = np.unpackbits(np.frombuffer(data, np.uint8, _BITMAP, at), bitorder="little").astype(bool)
    at += _BITMAP
    n_used = int(used.sum())
    if len(data) < at + 2 * n_used + tail:
        raise ValueError(f"{_NAME}: the bitmap names {n_used} contexts and {tail // 4} word counts follow them, "
                         f"{len(data) - at} bytes are left")
    present = np.frombuffer(data, "<u2", n_used, at).astype(np.int64)
    if n_used and present.min() < 1:
        raise ValueError(f"{_NAME}: a frequency of 0 in the table")
    f1 = np.full(CONTEXTS, 32768, np.int64)
    f1[used] = present
    return at + 2 * n_used, {"f1": f1, "used": used}, f", {n_used} contexts"


def read(data, n_blocks=None):
    """bytes -> {'group', 'n_blocks', 'f1' int64 [3072] (32768 where absent), 'used' bool [3072], 'nwords' int64
    [groups], 'states' uint64 [groups, 64], 'words' uint32 [total] (the groups' words back to back)}.  ValueError,
    naming the fault, on a wrong version, a truncated header, a group size or context count out of range, a bitmap
    that names more frequencies than follow, a frequency of 0, a word count no group can have, a block count other than
    `n_blocks`, and a payload that is shorter or longer than its counts say."""
    return _lp.frame_read(_KIND, _read_table, data, n_blocks)


def lossless_lod_line(n_bytes, n_points, ideal, n_used, n_symbols, group):
    """The `[LosslessLoD]` line of encode."""
    return "[LosslessLoD] bytes: %d bpp: %.4f ideal bpp: %.4f contexts: %d symbols: %d group: %d" % (
        n_bytes, 8.0 * n_bytes / n_points, ideal / n_points, n_used, n_symbols, group)


def check_status(status):
    """ValueError naming the first group whose decoder status is not 0."""
    _lp.check_status(status, _NAME)


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
    N, batch, group, span = _lp.span_args(_KIND, latents, gt, batch, group, span_groups)
    cnt = occ = bad = None
    for p, g in _lp.spans(net, latents, gt, batch, span):
        pyr = ops.occ_hier_pyramid(p, g, bad)
        bad = pyr["bad"]
        cnt, occ = ops.occ_hier_hist(pyr, cnt, occ)
    if int(bad.item()):
        raise ValueError(f"{_NAME}: {int(bad.item())} probabilities are NaN or outside [0, 1]")
    cnt, occ = (t.cpu().numpy().view(np.uint64) for t in (cnt, occ))
    f1, used = table_from_counts(cnt, occ)
    f1_dev = torch.tensor(f1, dtype=torch.int32, device=latents.device)

    def code(p, g):
        pyr = ops.occ_hier_pyramid(p, g)
        return (*ops.occ_hier_encode(pyr, f1_dev, group), pyr["gt_words"])
    states, words, gt_words = _lp.encode_spans(net, latents, gt, batch, span, code)
    pack = write(group, N, f1, used, states, words)
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
    return _lp.decode_spans(_KIND, net, latents, read(data, latents.shape[0]), batch, span_groups,
                            lambda p, *stream: ops.occ_hier_decode(ops.occ_hier_pyramid(p), *stream, level)[:3])
