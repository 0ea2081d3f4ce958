"""The third layout of the `lossless_lod_pack` entry of pack.pk (version 4): lossless_lod_pack.py's stream with the
voxels coded under a REFERENCE cloud that encoder and decoder both hold -- normally the previous frame's decoded
output, lossless or lossy; nothing about how it was made enters the format -- and under their parents' neighbours.
Pyramid, sections, symbol order, idle slots, coder, group framing and status rules are lossless_lod_pack's, and so are
the contexts of sections 2 and 1, (level * 4 + k) * 256 + occ_ctx(P): 1024..3071.  include/nvf_hip.h, "scalable lossless
geometry, inter contexts", is the contract of the kernels.

R, the reference words: the reference cloud rasterised onto THIS frame's leaf blocks (reference_words), int64 [N, 512]
in the format of gt_words[0].  R(q) is the reference occupancy of voxel q of the SAME block, 0 outside [0, 32)^3.
Context of a voxel v = (z, y, x) of section 0:

    a = R(v), f = the sum of R over the six face neighbours of v
    r = 2 if a else (1 if f > 0 else 0)                         the temporal class
    F, E, C = lossless_nbr_pack's counts around the parent      s = (F * 2 + (E > 0)) * 2 + C in [0, 16)
    t = r * 16 + s                                              in [0, 48)
    ctx = 3072 + (t * 4 + k) * 256 + occ_ctx(p[v])              k = K1[parent]

52224 contexts, of which 0..1023 are never used.  Table: lossless_pack's rule over the coded symbols.  Layout,
little-endian, the frame of lossless_pack:

    byte 0          version (4)
    bytes 1..2      uint16 G, bytes 3..6 uint32 block count N, bytes 7..8 uint16 context count (52224)
    then            32 bytes: digest(R), SHA-256 over the words' little-endian bytes
    then            384 bytes: the bitmap over the 3072 SLOTS, as lossless_nbr_pack; a level-0 slot (0..1023) is set
                    when a context of any t of it has a symbol
    then            per level-0 slot present, ascending: uint64 mask, bit t set when context 3072 + t * 1024 + slot has
                    a symbol; never 0, bits 48..63 are 0
    then            uint16 f1 of every context present, in ascending context order, each in [1, 65535]
    then            the word counts, and per group 64 states and its words, as lossless_lod_pack

decode_occupancy compares the digest before anything else: a wrong reference never decodes to a wrong cloud silently.
`module_of` tells the three layouts apart by byte 0.  The host half needs no device.
"""
import hashlib
import sys

import numpy as np
import torch

from . import lossless_lod_pack as _llp
from . import lossless_nbr_pack as _nbr
from . import lossless_pack as _lp
from .lossless_lod_pack import GROUP, check_status, lossless_lod_line  # noqa: F401  (this layout's too)
from .lossless_pack import SPAN_GROUPS, ideal_bits, points_from_words  # noqa: F401

VERSION = 4
SLOTS = 3072
CLASSES = 48
CONTEXTS = SLOTS + CLASSES * 1024
BLOCK_WORDS = _llp.BLOCK_WORDS
DIGEST = 32
_BITMAP = SLOTS // 8
_NAME = "lossless_lod_pack"
_KIND = _lp.Kind(_NAME, VERSION, CONTEXTS, BLOCK_WORDS)


def module_of(data):
    """The module that reads the lossless_lod_pack bytes `data`, by their version byte: this one for 4, else what
    lossless_nbr_pack.module_of says (1, 3, or ValueError naming the version)."""
    if bytes(data[:1]) == bytes([VERSION]):
        return sys.modules[__name__]
    return _nbr.module_of(data)


def digest(words):
    """SHA-256 over the reference words' little-endian bytes: int64 / uint64 [N, 512], numpy or torch -> 32 bytes."""
    if isinstance(words, torch.Tensor):
        words = words.detach().cpu().numpy()
    words = np.ascontiguousarray(words)
    if words.dtype not in (np.int64, np.uint64) or words.ndim != 2 or words.shape[1] != 512:
        raise ValueError(f"{_NAME}: the reference words are 64-bit [N, 512]")
    return hashlib.sha256(words.view(np.uint64).astype("<u8").tobytes()).digest()


def reference_words(points, origins, device=None):
    """The reference cloud `points` (int [M, 3]) rasterised onto the blocks at `origins` (int [N, 3]) on the device:
    -> (words int64 [N, 512] on the device, dropped: the points under no block).  A point q sets the bit of voxel
    q & 31 (per axis, raster order) in the block whose origin is q & ~31; duplicates are harmless."""
    from . import ops
    if device is None:
        device = points.device if isinstance(points, torch.Tensor) else torch.device("cuda")
    pts = torch.as_tensor(np.asarray(points.cpu() if isinstance(points, torch.Tensor) else points)).reshape(-1, 3)
    big = 1 << 30
    pts = pts.to(torch.int64).clamp(-big, big).to(torch.int32).to(device).contiguous()     # beyond any block either way
    org = torch.as_tensor(np.asarray(origins.cpu() if isinstance(origins, torch.Tensor) else origins)).reshape(-1, 3)
    words, dropped = ops.occ_ref_words(pts, org.to(torch.int32).to(device).contiguous())
    return words, int(dropped.item())


def table_from_counts(cnt, occ):
    """Per context the coded symbols and the occupied ones -> (f1 int64 [52224], used bool [52224]): lossless_pack's
    rule (table_rule) in Python integers over the contexts that have symbols, 32768 and unused for the rest."""
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
    return _lp.frame_size(DIGEST + _BITMAP + 8 * int(n_slots0) + 2 * int(n_used), n_blocks, group, n_words)


def write(group, n_blocks, ref_digest, f1, used, states, words):
    """ref_digest: digest(R), 32 bytes; f1: the frequencies of the contexts present, ascending (or all 52224, of which
    those are taken); used: bool [52224]; states: uint64 [groups, 64] (or int64 holding them); words: one uint32 array
    per group -> bytes."""
    group, n_blocks = _lp.frame_counts(_KIND, group, n_blocks)
    ref_digest = bytes(ref_digest)
    if len(ref_digest) != DIGEST:
        raise ValueError(f"{_NAME}: the reference's digest is {DIGEST} bytes")
    used = np.asarray(used).reshape(-1)
    if used.shape != (CONTEXTS,):
        raise ValueError(f"{_NAME}: the inter table has {CONTEXTS} contexts")
    used = used.astype(bool)
    if used[:1024].any():
        raise ValueError(f"{_NAME}: contexts 0..1023 belong to no level of the inter table")
    f1 = np.asarray(f1, np.int64).reshape(-1)
    if f1.size == CONTEXTS and int(used.sum()) != CONTEXTS:
        f1 = f1[used]
    if f1.size != int(used.sum()):
        raise ValueError(f"{_NAME}: the table names {int(used.sum())} contexts, {f1.size} frequencies given")
    if f1.size and (f1.min() < 1 or f1.max() > 65535):
        raise ValueError(f"{_NAME}: the table's frequencies are in [1, 65535]")
    by_t = used[SLOTS:].reshape(CLASSES, 1024)
    slots = np.concatenate([by_t.any(0), used[1024:SLOTS]])
    masks = (by_t.astype(np.uint64) << np.arange(CLASSES, dtype=np.uint64)[:, None]).sum(0, dtype=np.uint64)[slots[:1024]]
    table = ref_digest + np.packbits(slots, bitorder="little").tobytes() + masks.astype("<u8").tobytes() + \
        f1.astype("<u2").tobytes()
    return _lp.frame_write(_KIND, group, n_blocks, table, states, words)


def _read_table(data, at, tail):
    if len(data) < at + DIGEST:
        raise ValueError(f"{_NAME}: truncated digest of the reference")
    ref_digest = bytes(data[at:at + DIGEST])
    at += DIGEST
    if len(data) < at + _BITMAP:
        raise ValueError(f"{_NAME}: truncated bitmap")
    slots = np.unpackbits(np.frombuffer(data, np.uint8, _BITMAP, at), bitorder="little").astype(bool)
    at += _BITMAP
    slots0 = np.flatnonzero(slots[:1024])
    if len(data) < at + 8 * slots0.size:
        raise ValueError(f"{_NAME}: the bitmap names {slots0.size} level-0 slots, {(len(data) - at) // 8} masks follow")
    masks = np.frombuffer(data, "<u8", slots0.size, at).astype(np.uint64)
    at += 8 * slots0.size
    if slots0.size and masks.min() == 0:
        raise ValueError(f"{_NAME}: a class mask of 0 for slot {int(slots0[np.argmin(masks)])}")
    if slots0.size and int(masks.max()) >> CLASSES:
        raise ValueError(f"{_NAME}: a class mask with a bit at or above {CLASSES} for slot "
                         f"{int(slots0[np.argmax(masks)])}")
    used = np.zeros(CONTEXTS, bool)
    used[1024:SLOTS] = slots[1024:]
    used[SLOTS:].reshape(CLASSES, 1024)[:, slots0] = (masks[None, :] >> np.arange(CLASSES, dtype=np.uint64)[:, None]) & np.uint64(1)
    n_used = int(used.sum())
    if len(data) < at + 2 * n_used + tail:
        raise ValueError(f"{_NAME}: the bitmap and the masks name {n_used} contexts and {tail // 4} word counts follow "
                         f"them, {len(data) - at} bytes are left")
    present = np.frombuffer(data, "<u2", n_used, at).astype(np.int64)
    if n_used and present.min() < 1:
        raise ValueError(f"{_NAME}: a frequency of 0 in the table")
    f1 = np.full(CONTEXTS, 32768, np.int64)
    f1[used] = present
    return at + 2 * n_used, {"digest": ref_digest, "f1": f1, "used": used}, f", {n_used} contexts"


def read(data, n_blocks=None):
    """bytes -> {'group', 'n_blocks', 'digest' (32 bytes), 'f1' int64 [52224] (32768 where absent), 'used' bool [52224],
    'nwords', 'states', 'words'} as lossless_nbr_pack.read.  ValueError, naming the fault, on everything that reader
    rejects, on a digest cut short and on a mask with a bit at or above 48."""
    return _lp.frame_read(_KIND, _read_table, data, n_blocks)


# ---------------------------------------------------------------- device half
def _ref_spans(ref_words, N, span):
    if not isinstance(ref_words, torch.Tensor) or ref_words.dtype != torch.int64 or ref_words.shape != (N, 512):
        raise ValueError(f"{_NAME}: the reference words are int64 [{N}, 512], one row of 512 per block")
    return iter(ref_words[lo:lo + span].contiguous() for lo in range(0, N, span))


@torch.no_grad()
def encode_occupancy(net, latents, gt, ref_words, batch=64, group=GROUP, span_groups=SPAN_GROUPS):
    """lossless_nbr_pack.encode_occupancy under the inter contexts: ref_words int64 [N, 512] on the device
    (reference_words) after gt, else the same arguments and results (f1, used, cnt, occ over 52224 contexts, 'slots0',
    and 'digest': digest(ref_words)), version-4 bytes."""
    from . import ops
    N, batch, group, span = _lp.span_args(_KIND, latents, gt, batch, group, span_groups)
    refs = _ref_spans(ref_words, N, span)
    cnt = occ = bad = None
    for p, g in _lp.spans(net, latents, gt, batch, span):
        pyr = ops.occ_hier_pyramid(p, g, bad)
        bad = pyr["bad"]
        cnt, occ = ops.occ_inter_hist(pyr, next(refs), cnt, occ)
    if int(bad.item()):
        raise ValueError(f"{_NAME}: {int(bad.item())} probabilities are NaN or outside [0, 1]")
    cnt, occ = (t.cpu().numpy().view(np.uint64) for t in (cnt, occ))
    f1, used = table_from_counts(cnt, occ)
    f1_dev = torch.from_numpy(f1.astype(np.int32)).to(latents.device)
    refs = _ref_spans(ref_words, N, span)

    def code(p, g):
        pyr = ops.occ_hier_pyramid(p, g)
        return (*ops.occ_inter_encode(pyr, next(refs), f1_dev, group), pyr["gt_words"])
    states, words, gt_words = _lp.encode_spans(net, latents, gt, batch, span, code)
    ref_digest = digest(ref_words)
    pack = write(group, N, ref_digest, f1, used, states, words)
    return pack, {"ideal_bits": ideal_bits(f1[used], cnt[used], occ[used]), "f1": f1, "used": used, "cnt": cnt,
                  "occ": occ, "contexts": int(used.sum()), "symbols": int(cnt.sum()), "digest": ref_digest,
                  "slots0": int(used[SLOTS:].reshape(CLASSES, 1024).any(0).sum()),
                  "gt_words": tuple(torch.cat([g[lv] for g in gt_words], 0) for lv in range(3))}


@torch.no_grad()
def decode_occupancy(net, latents, data, ref_words, level=0, batch=64, span_groups=SPAN_GROUPS):
    """lossless_lod_pack.decode_occupancy for version-4 bytes, with the reference words (int64 [N, 512] on the device)
    after data.  ValueError naming both digests and the reference's point count when ref_words is not what the pack was
    coded under, before anything is decoded."""
    from . import ops
    if level not in (0, 1, 2):
        raise ValueError(f"{_NAME}: level {level!r}, the stream holds levels 0, 1 and 2")
    side = read(data, latents.shape[0])
    span = _lp._span(max(int(batch), 1), side["group"], span_groups)
    refs = _ref_spans(ref_words, latents.shape[0], span)
    have = digest(ref_words)
    if have != side["digest"]:
        n_ref = sum(int(ops.occ_hier_cells(ref_words[lo:lo + ops.OCC_HIER_MAX_BATCH].contiguous(), fill=False)[0].sum().item())
                    for lo in range(0, ref_words.shape[0], ops.OCC_HIER_MAX_BATCH))
        raise ValueError(f"{_NAME}: the reference is not the one the pack was coded under: its words' digest is "
                         f"{have.hex()}, the pack's {side['digest'].hex()}; the reference sets {n_ref} voxels under "
                         f"this frame's {latents.shape[0]} blocks")
    return _lp.decode_spans(_KIND, net, latents, side, batch, span_groups,
                            lambda p, *stream: ops.occ_inter_decode(ops.occ_hier_pyramid(p), next(refs), *stream, level)[:3])
