"""The second layout of the `lossless_lod_pack` entry of pack.pk (version 3): lossless_lod_pack.py's stream with the
voxels coded under their parents' neighbours.  Pyramid, sections, symbol order, idle slots, coder, group framing and
status rules are lossless_lod_pack's, and so are the contexts of sections 2 and 1, (level * 4 + k) * 256 + occ_ctx(P):
1024..3071.  include/nvf_hip.h, "scalable lossless geometry, neighbour contexts", is the contract of the kernels.

Context of a voxel v = (z, y, x) of section 0.  Its parent is P = (z >> 1, y >> 1, x >> 1) on the 16^3 grid; s_a = +1
where v's coordinate on axis a is odd, else -1; O(q) is the level-1 occupancy of cell q of the SAME block and 0 outside
[0, 16)^3 -- the ground truth's max-pool at the encoder, what section 1 produced at the decoder, which therefore holds
it before the first voxel.  Then

    F = O(P + s_z e_z) + O(P + s_y e_y) + O(P + s_x e_x)        the three face neighbours on v's side of P
    E = the same sum over the three two-axis offsets, C = O at the three-axis offset
    n = (F * 4 + E) * 2 + C                                     in [0, 32)
    ctx = 3072 + (n * 4 + k) * 256 + occ_ctx(p[v])              k = K1[P]

35840 contexts, of which 0..1023 are never used.  Table: lossless_pack's rule over the coded symbols.  Layout,
little-endian, the frame of lossless_pack:

    byte 0          version (3)
    bytes 1..2      uint16 G, bytes 3..6 uint32 block count N, bytes 7..8 uint16 context count (35840)
    then            384 bytes: the bitmap over the 3072 SLOTS (level, k, occ_ctx) = (level * 4 + k) * 256 + occ_ctx; a
                    level-0 slot (0..1023) is set when a context of any n of it has a symbol
    then            per level-0 slot present, ascending: uint32 mask, bit n set when context 3072 + n * 1024 + slot has
                    a symbol; never 0
    then            uint16 f1 of every context present, in ascending context order, each in [1, 65535]
    then            the word counts, and per group 64 states and its words, as lossless_lod_pack

so the table follows the contexts in use, not the 35840.  `module_of` tells the two layouts apart by byte 0.  The host
half needs no device.
"""
import sys

import numpy as np
import torch

from . import lossless_lod_pack as _llp
from . import lossless_pack as _lp
from .lossless_lod_pack import GROUP, check_status, lossless_lod_line  # noqa: F401  (this layout's too)
from .lossless_pack import SPAN_GROUPS, ideal_bits, points_from_words  # noqa: F401

VERSION = 3
SLOTS = 3072
CONTEXTS = SLOTS + 32 * 1024
BLOCK_WORDS = _llp.BLOCK_WORDS
_BITMAP = SLOTS // 8
_NAME = "lossless_lod_pack"
_KIND = _lp.Kind(_NAME, VERSION, CONTEXTS, BLOCK_WORDS)


def module_of(data):
    """The module that reads the lossless_lod_pack bytes `data`, by their version byte; ValueError naming any other."""
    data = bytes(data[:1])
    if not data:
        raise ValueError(f"{_NAME}: empty")
    if data[0] == _llp.VERSION:
        return _llp
    if data[0] == VERSION:
        return sys.modules[__name__]
    raise ValueError(f"{_NAME}: version {data[0]}, the readers know {_llp.VERSION} (field contexts) and {VERSION} "
                     f"(neighbour contexts)")


def table_from_counts(cnt, occ):
    """Per context the coded symbols and the occupied ones -> (f1 int64 [35840], used bool [35840]): lossless_pack's
    rule (table_rule) in Python integers over the contexts that have symbols -- a few hundred of the 35840 --, 32768
    and unused for the rest."""
    cnt, occ = np.asarray(cnt).reshape(-1), np.asarray(occ).reshape(-1)
    if cnt.shape != (CONTEXTS,) or occ.shape != (CONTEXTS,) or (occ[cnt == 0] != 0).any():
        raise ValueError(f"{_NAME}: the counts are {CONTEXTS} pairs with 0 <= occupied <= symbols")
    used = cnt != 0
    f1 = np.full(CONTEXTS, 32768, np.int64)
    f1[used] = _lp.table_rule(_KIND._replace(contexts=int(used.sum())), "symbols", cnt[used].tolist(), occ[used].tolist())[0]
    return f1, used


def size(n_blocks, group, n_words, n_used, n_slots0):
    """Bytes of a pack of n_blocks blocks in groups of `group`, n_words words in all, n_used contexts present, n_slots0
    of the 1024 level-0 slots among them."""
    return _lp.frame_size(_BITMAP + 4 * int(n_slots0) + 2 * int(n_used), n_blocks, group, n_words)


def write(group, n_blocks, f1, used, states, words):
    """f1: the frequencies of the contexts present, ascending (or all 35840, of which those are taken); used: bool
    [35840]; states: uint64 [groups, 64] (or int64 holding them); words: one uint32 array per group -> bytes."""
    group, n_blocks = _lp.frame_counts(_KIND, group, n_blocks)
    used = np.asarray(used).reshape(-1)
    if used.shape != (CONTEXTS,):
        raise ValueError(f"{_NAME}: the neighbour table has {CONTEXTS} contexts")
    used = used.astype(bool)
    if used[:1024].any():
        raise ValueError(f"{_NAME}: contexts 0..1023 belong to no level of the neighbour table")
    f1 = np.asarray(f1, np.int64).reshape(-1)
    if f1.size == CONTEXTS and int(used.sum()) != CONTEXTS:
        f1 = f1[used]
    if f1.size != int(used.sum()):
        raise ValueError(f"{_NAME}: the table names {int(used.sum())} contexts, {f1.size} frequencies given")
    if f1.size and (f1.min() < 1 or f1.max() > 65535):
        raise ValueError(f"{_NAME}: the table's frequencies are in [1, 65535]")
    by_n = used[SLOTS:].reshape(32, 1024)
    slots = np.concatenate([by_n.any(0), used[1024:SLOTS]])
    masks = (by_n.astype(np.uint64) << np.arange(32, dtype=np.uint64)[:, None]).sum(0)[slots[:1024]]
    table = np.packbits(slots, bitorder="little").tobytes() + masks.astype("<u4").tobytes() + f1.astype("<u2").tobytes()
    return _lp.frame_write(_KIND, group, n_blocks, table, states, words)


def _read_table(data, at, tail):
    if len(data) < at + _BITMAP:
        raise ValueError(f"{_NAME}: truncated bitmap")
    slots = np.unpackbits(np.frombuffer(data, np.uint8, _BITMAP, at), bitorder="little").astype(bool)
    at += _BITMAP
    slots0 = np.flatnonzero(slots[:1024])
    if len(data) < at + 4 * slots0.size:
        raise ValueError(f"{_NAME}: the bitmap names {slots0.size} level-0 slots, {(len(data) - at) // 4} masks follow")
    masks = np.frombuffer(data, "<u4", slots0.size, at).astype(np.int64)
    at += 4 * slots0.size
    if slots0.size and masks.min() == 0:
        raise ValueError(f"{_NAME}: a neighbour mask of 0 for slot {int(slots0[np.argmin(masks)])}")
    used = np.zeros(CONTEXTS, bool)
    used[1024:SLOTS] = slots[1024:]
    used[SLOTS:].reshape(32, 1024)[:, slots0] = (masks[None, :] >> np.arange(32)[:, None]) & 1
    n_used = int(used.sum())
    if len(data) < at + 2 * n_used + tail:
        raise ValueError(f"{_NAME}: the bitmap and the masks name {n_used} contexts and {tail // 4} word counts follow "
                         f"them, {len(data) - at} bytes are left")
    present = np.frombuffer(data, "<u2", n_used, at).astype(np.int64)
    if n_used and present.min() < 1:
        raise ValueError(f"{_NAME}: a frequency of 0 in the table")
    f1 = np.full(CONTEXTS, 32768, np.int64)
    f1[used] = present
    return at + 2 * n_used, {"f1": f1, "used": used}, f", {n_used} contexts"


def read(data, n_blocks=None):
    """bytes -> {'group', 'n_blocks', 'f1' int64 [35840] (32768 where absent), 'used' bool [35840], 'nwords', 'states',
    'words'} as lossless_lod_pack.read.  ValueError, naming the fault, on everything that reader rejects, on masks cut
    short and on a mask of 0.  The masks are positional -- one per level-0 slot the bitmap names --, so the bytes cannot
    hold a mask for a slot of another level; `write` refuses a table that would need one (contexts 0..1023)."""
    return _lp.frame_read(_KIND, _read_table, data, n_blocks)


# ---------------------------------------------------------------- device half
@torch.no_grad()
def encode_occupancy(net, latents, gt, batch=64, group=GROUP, span_groups=SPAN_GROUPS):
    """lossless_lod_pack.encode_occupancy under the neighbour contexts: the same arguments, the same results (f1, used,
    cnt, occ as arrays over 35840 contexts, and 'slots0': the level-0 slots present), version-3 bytes."""
    from . import ops
    N, batch, group, span = _lp.span_args(_KIND, latents, gt, batch, group, span_groups)
    cnt = occ = bad = None
    for p, g in _lp.spans(net, latents, gt, batch, span):
        pyr = ops.occ_hier_pyramid(p, g, bad)
        bad = pyr["bad"]
        cnt, occ = ops.occ_nbr_hist(pyr, cnt, occ)
    if int(bad.item()):
        raise ValueError(f"{_NAME}: {int(bad.item())} probabilities are NaN or outside [0, 1]")
    cnt, occ = (t.cpu().numpy().view(np.uint64) for t in (cnt, occ))
    f1, used = table_from_counts(cnt, occ)
    f1_dev = torch.from_numpy(f1.astype(np.int32)).to(latents.device)

    def code(p, g):
        pyr = ops.occ_hier_pyramid(p, g)
        return (*ops.occ_nbr_encode(pyr, f1_dev, group), pyr["gt_words"])
    states, words, gt_words = _lp.encode_spans(net, latents, gt, batch, span, code)
    pack = write(group, N, f1, used, states, words)
    return pack, {"ideal_bits": ideal_bits(f1[used], cnt[used], occ[used]), "f1": f1, "used": used, "cnt": cnt,
                  "occ": occ, "contexts": int(used.sum()), "symbols": int(cnt.sum()),
                  "slots0": int(used[SLOTS:].reshape(32, 1024).any(0).sum()),
                  "gt_words": tuple(torch.cat([g[lv] for g in gt_words], 0) for lv in range(3))}


@torch.no_grad()
def decode_occupancy(net, latents, data, level=0, batch=64, span_groups=SPAN_GROUPS):
    """lossless_lod_pack.decode_occupancy for version-3 bytes: the same arguments, results and errors."""
    from . import ops
    if level not in (0, 1, 2):
        raise ValueError(f"{_NAME}: level {level!r}, the stream holds levels 0, 1 and 2")
    return _lp.decode_spans(_KIND, net, latents, read(data, latents.shape[0]), batch, span_groups,
                            lambda p, *stream: ops.occ_nbr_decode(ops.occ_hier_pyramid(p), *stream, level)[:3])
