"""The `lossless_pack` entry of pack.pk: the true occupancy of every leaf block, entropy-coded under the decoder's field.

The decoder gives a probability p for every voxel of every leaf block, and the eval forward is bit-exact and
batch-invariant, so encoder and decoder see the same p.  The leaf blocks cover every input point, so the occupancy of
their voxels IS the cloud.  A voxel's context is a function of the float32 bits of p (include/nvf_hip.h, "lossless
geometry"): the focal loss does not train calibrated probabilities, so what the coder uses is not p but the measured
occupancy rate of the voxel's context, f1[ctx] / 65536, and the 256 rates travel in the pack.  The coder is a binary
rANS coder, 64 interleaved states per group of G consecutive blocks (csrc/occ_rans.hip).  Layout, little-endian:

    byte 0          version (VERSION)
    bytes 1..2      uint16 G: blocks per group (the last group may be shorter)
    bytes 3..6      uint32 block count N
    bytes 7..8      uint16 context count (256)
    then            uint16 f1[contexts], each in [1, 65535]
    then            uint32 word count of each of the ceil(N / G) groups
    then per group  64 uint64 states, then its uint32 words in the order the decoder reads them

The 64 final states of a group are flushed whole: 4096 bits per group, which is why G defaults to 64 and not to 1.
8 x len(lossless_pack) bits go into the side information of Gross bpp.  The host half of this module (the table rule,
write, read) needs no device; encode_occupancy / decode_occupancy run the forward and the kernels.

lossless_lod_pack.py is a second pack of the same frame with another table section and another coder call.  What the
two share is here, once: the table rule (table_rule), the framing (frame_counts, frame_write, frame_read, frame_size:
header, a table section passed in, word counts, per group 64 states and words, every size and range check), the span
loops (span_args, spans, encode_spans, decode_spans), check_status and points_from_words.  A Kind names the pack in
the errors and carries its version, context count and per-block word bound.
"""
import collections
import math
import struct

import numpy as np
import torch

VERSION = 1
CONTEXTS = 256
GROUP = 64
MAX_GROUP = 1024
SPAN_GROUPS = 8         # groups whose probabilities stay resident for one coder launch: one wave each, side by side
_HEADER = struct.Struct("<BHIH")
# what tells one pack from another (lossless_lod_pack.py has the second): the name its errors carry, its version byte,
# its context count and the words a block can emit at the most
Kind = collections.namedtuple("Kind", "name version contexts block_words")
_KIND = Kind("lossless_pack", VERSION, CONTEXTS, 32768)


def table_rule(kind, what, cnt, occ):
    """Per context the count and the occupied count -> (f1 as a list of Python integers, used as a list of bools):
    clamp((2 * 65536 * occ + cnt) // (2 * cnt), 1, 65535), and 32768, unused, for a context that counts nothing."""
    cnt, occ = [int(v) for v in cnt], [int(v) for v in occ]
    if len(cnt) != kind.contexts or len(occ) != kind.contexts or any(o < 0 or o > c for c, o in zip(cnt, occ)):
        raise ValueError(f"{kind.name}: the counts are {kind.contexts} pairs with 0 <= occupied <= {what}")
    f1 = [32768 if c == 0 else min(max((2 * 65536 * o + c) // (2 * c), 1), 65535) for c, o in zip(cnt, occ)]
    return f1, [c > 0 for c in cnt]


def table_from_counts(cnt, occ):
    """Per context the voxel count and the occupied count -> f1 as a list of Python integers (table_rule)."""
    return table_rule(_KIND, "voxels", cnt, occ)[0]


def ideal_bits(f1, cnt, occ):
    """Code length of the symbols under the table, in bits (float64): what a coder without any overhead would spend."""
    bits = 0.0
    for f, c, o in zip(f1, cnt, occ):
        f, c, o = int(f), int(c), int(o)
        if o:
            bits -= o * math.log2(f / 65536.0)
        if c - o:
            bits -= (c - o) * math.log2(1.0 - f / 65536.0)
    return bits


def n_groups(n_blocks, group):
    return (int(n_blocks) + int(group) - 1) // int(group)


def frame_size(table_bytes, n_blocks, group, n_words):
    """Bytes of a pack whose table section takes table_bytes: header, table, word counts, per group 64 states + words."""
    return _HEADER.size + int(table_bytes) + n_groups(n_blocks, group) * (4 + 64 * 8) + 4 * int(n_words)


def size(n_blocks, group, n_words):
    """Bytes of a pack of n_blocks blocks in groups of `group` whose groups hold n_words words in all."""
    return frame_size(2 * CONTEXTS, n_blocks, group, n_words)


def frame_counts(kind, group, n_blocks):
    """The group size and block count a pack can hold, as integers."""
    group, n_blocks = int(group), int(n_blocks)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"{kind.name}: group {group} outside [1, {MAX_GROUP}]")
    if not 1 <= n_blocks < 1 << 32:
        raise ValueError(f"{kind.name}: block count {n_blocks}")
    return group, n_blocks


def frame_write(kind, group, n_blocks, table, states, words):
    """The framing both packs share: header, the table section `table` (bytes), the groups' word counts, then per group
    its 64 states and its words.  group and n_blocks have passed frame_counts."""
    ng = n_groups(n_blocks, group)
    states = np.ascontiguousarray(states).view(np.uint64) if np.asarray(states).dtype == np.int64 else np.asarray(states, np.uint64)
    if states.shape != (ng, 64) or len(words) != ng:
        raise ValueError(f"{kind.name}: {n_blocks} blocks in groups of {group} are {ng} groups of 64 states")
    words = [np.ascontiguousarray(w).view(np.uint32) if np.asarray(w).dtype == np.int32 else np.asarray(w, np.uint32)
             for w in words]
    for g, w in enumerate(words):
        if w.ndim != 1 or w.size > min(group, n_blocks - g * group) * kind.block_words:
            raise ValueError(f"{kind.name}: group {g} holds more words than it has symbols")
    parts = [_HEADER.pack(kind.version, group, n_blocks, kind.contexts), table,
             np.asarray([w.size for w in words], "<u4").tobytes()]
    for g in range(ng):
        parts += [states[g].astype("<u8").tobytes(), words[g].astype("<u4").tobytes()]
    return b"".join(parts)


def frame_read(kind, read_table, data, n_blocks=None):
    """The inverse of frame_write.  read_table(data, at, tail) consumes the table section at data[at:], of which `tail`
    bytes of word counts must be left after it, and returns (the offset behind it, the dict entries it read, what the
    size fault calls them: '' or ', N contexts').  -> {'group', 'n_blocks', the table's entries, 'nwords' int64
    [groups], 'states' uint64 [groups, 64], 'words' uint32 [total] (the groups' words back to back)}."""
    name = kind.name
    data = bytes(data)
    if len(data) < 1:
        raise ValueError(f"{name}: empty")
    if data[0] != kind.version:
        raise ValueError(f"{name}: version {data[0]}, this reader knows {kind.version}")
    if len(data) < _HEADER.size:
        raise ValueError(f"{name}: truncated header")
    _, group, nb, nctx = _HEADER.unpack_from(data)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"{name}: group size {group} outside [1, {MAX_GROUP}]")
    if nb < 1:
        raise ValueError(f"{name}: no blocks")
    if n_blocks is not None and nb != int(n_blocks):
        raise ValueError(f"{name}: codes {nb} blocks, the pack holds {int(n_blocks)}")
    if nctx != kind.contexts:
        raise ValueError(f"{name}: {nctx} contexts, this reader knows {kind.contexts}")
    ng = n_groups(nb, group)
    at, table, what = read_table(data, _HEADER.size, 4 * ng)
    table_bytes = at - _HEADER.size
    nwords = np.frombuffer(data, "<u4", ng, at).astype(np.int64)
    at += 4 * ng
    for g in range(ng):
        if nwords[g] > min(group, nb - g * group) * kind.block_words:
            raise ValueError(f"{name}: group {g} claims {int(nwords[g])} words, more than it has symbols")
    need = frame_size(table_bytes, nb, group, int(nwords.sum()))
    if len(data) != need:
        raise ValueError(f"{name}: {len(data)} bytes, {need} expected for {nb} blocks{what} and {int(nwords.sum())} words")
    states, words = np.empty((ng, 64), np.uint64), []
    for g in range(ng):
        states[g] = np.frombuffer(data, "<u8", 64, at)
        at += 512
        words.append(np.frombuffer(data, "<u4", int(nwords[g]), at).astype(np.uint32))
        at += 4 * int(nwords[g])
    return {"group": group, "n_blocks": nb, **table, "nwords": nwords, "states": states,
            "words": np.concatenate(words) if words else np.zeros(0, np.uint32)}


def write(group, n_blocks, f1, states, words):
    """states: uint64 [groups, 64] (or int64 holding them); words: one uint32 array per group -> bytes."""
    group, n_blocks = frame_counts(_KIND, group, n_blocks)
    f1 = np.asarray(f1, np.int64).reshape(-1)
    if f1.shape != (CONTEXTS,) or f1.min() < 1 or f1.max() > 65535:
        raise ValueError(f"lossless_pack: the table is {CONTEXTS} frequencies in [1, 65535]")
    return frame_write(_KIND, group, n_blocks, f1.astype("<u2").tobytes(), states, words)


def _read_table(data, at, tail):
    if len(data) < at + 2 * CONTEXTS + tail:
        raise ValueError("lossless_pack: truncated table or word counts")
    f1 = np.frombuffer(data, "<u2", CONTEXTS, at).astype(np.int64)
    if f1.min() < 1:
        raise ValueError("lossless_pack: a frequency of 0 in the table")
    return at + 2 * CONTEXTS, {"f1": f1}, ""


def read(data, n_blocks=None):
    """bytes -> {'group', 'n_blocks', 'f1' int64 [256], 'nwords' int64 [groups], 'states' uint64 [groups, 64],
    'words' uint32 [total] (the groups' words back to back)}.  ValueError, naming the fault, on a wrong version, a
    truncated header, a group size or context count or frequency out of range, a word count no group can have, a
    block count other than `n_blocks`, and a payload that is shorter or longer than its counts say."""
    return frame_read(_KIND, _read_table, data, n_blocks)


def lossless_line(n_bytes, n_points, ideal, group):
    """The `[Lossless]` line of encode."""
    return "[Lossless] bytes: %d bpp: %.4f ideal bpp: %.4f contexts: %d group: %d" % (
        n_bytes, 8.0 * n_bytes / n_points, ideal / n_points, CONTEXTS, group)


# ---------------------------------------------------------------- device half
def _span(batch, group, span_groups):
    """Blocks per coder launch: a group is ONE wave, so a launch takes `span_groups` of them (more where the forward's
    batch holds more) and their probabilities, 128 KiB per block, stay resident for it."""
    return max(int(batch) // int(group), int(span_groups), 1) * int(group)


def span_args(kind, latents, gt, batch, group, span_groups):
    """What both encoders check first -> (N, batch, group, blocks per coder launch)."""
    N, batch, group = latents.shape[0], max(int(batch), 1), int(group)
    if not 1 <= group <= MAX_GROUP:
        raise ValueError(f"{kind.name}: group {group} outside [1, {MAX_GROUP}]")
    if gt.shape[0] != N:
        raise ValueError(f"{kind.name}: {N} latents and {gt.shape[0]} blocks of ground truth")
    return N, batch, group, _span(batch, group, span_groups)


def spans(net, latents, gt, batch, span):
    """Span by span (p, the span's ground truth or None): one pass of the forward over the cloud, `batch` blocks a call."""
    from .recon import eval_batches
    for lo in range(0, latents.shape[0], span):
        hi = min(lo + span, latents.shape[0])
        parts = [p for _, _, p in eval_batches(net, latents[lo:hi], batch)]
        yield parts[0] if len(parts) == 1 else torch.cat(parts, 0), None if gt is None else gt[lo:hi].contiguous()


def encode_spans(net, latents, gt, batch, span, code):
    """The coder's pass: code(p, gt) -> (states, the groups' words, anything) for every span -> (states uint64-holding
    int64 [groups, 64] and one word array per group, both numpy; the spans' third results)."""
    states, words, extras = [], [], []
    for p, g in spans(net, latents, gt, batch, span):
        s, w, extra = code(p, g)
        states.append(s.cpu().numpy())
        words += [x.cpu().numpy() for x in w]
        extras.append(extra)
    return np.concatenate(states, 0), words, extras


def decode_spans(kind, net, latents, side, batch, span_groups, decode):
    """The decoder's pass over a read pack: decode(p, f1, states, words, nwords, group) -> (occupancy words, counts,
    status) for every span, each with its own groups' side data -> (words, counts) of the cloud on the device;
    ValueError (check_status) when a group's status is not 0."""
    N, group, dev = side["n_blocks"], side["group"], latents.device
    span = _span(max(int(batch), 1), group, span_groups)
    f1_dev = torch.from_numpy(side["f1"].astype(np.int32)).to(dev)
    states = torch.from_numpy(side["states"].view(np.int64)).to(dev)
    words = torch.from_numpy(side["words"].view(np.int32)).to(dev)
    nwords = torch.from_numpy(side["nwords"].astype(np.int32)).to(dev)
    off = np.concatenate([[0], np.cumsum(side["nwords"])])
    out = []
    for i, (p, _) in enumerate(spans(net, latents, None, batch, span)):
        g0, g1 = i * span // group, n_groups(min((i + 1) * span, N), group)
        out.append(decode(p, f1_dev, states[g0:g1].contiguous(), words[int(off[g0]):int(off[g1])].contiguous(),
                          nwords[g0:g1].contiguous(), group))
    out_w, out_c, out_s = zip(*out)
    check_status(torch.cat(out_s).cpu().numpy(), kind.name)
    return torch.cat(out_w, 0), torch.cat(out_c, 0)


@torch.no_grad()
def encode_occupancy(net, latents, gt, batch=64, group=GROUP, span_groups=SPAN_GROUPS):
    """latents [N, ch, 2, 2, 2] (rounded, on the device) and gt float32 [N, 1, 32, 32, 32] (non-zero = occupied) ->
    (lossless_pack bytes, {'ideal_bits', 'f1', 'cnt', 'occ', 'gt_words' int64 [N, 512] on the device}).
    The forward runs twice -- once for the calibration table, once for the coder -- in calls of `batch` blocks, and the
    coder takes `span_groups` whole groups per launch (_span), so memory follows the batch and the span, not the cloud.
    ValueError when a probability is NaN or outside [0, 1]."""
    from . import ops
    N, batch, group, span = span_args(_KIND, latents, gt, batch, group, span_groups)
    acc = ()
    for p, g in spans(net, latents, gt, batch, span):
        acc = ops.occ_ctx_hist(p, g, *acc)
    cnt, occ, bad = (t.cpu().numpy().view(np.uint64) for t in acc)
    if int(bad[0]):
        raise ValueError(f"lossless_pack: {int(bad[0])} probabilities are NaN or outside [0, 1]")
    f1 = table_from_counts(cnt, occ)
    f1_dev = torch.tensor(f1, dtype=torch.int32, device=latents.device)
    states, words, gt_words = encode_spans(net, latents, gt, batch, span, lambda p, g: ops.occ_rans_encode(p, g, f1_dev, group))
    pack = write(group, N, f1, states, words)
    return pack, {"ideal_bits": ideal_bits(f1, cnt, occ), "f1": f1, "cnt": cnt, "occ": occ,
                  "gt_words": torch.cat(gt_words, 0)}


@torch.no_grad()
def decode_occupancy(net, latents, data, batch=64, span_groups=SPAN_GROUPS):
    """lossless_pack bytes -> (occupancy words int64 [N, 512] on the device: bit k of word w of a block = its voxel
    64 w + k in raster order; counts int32 [N]).  ValueError on a malformed pack (read), on one that codes another
    number of blocks than `latents` has, and on a stream whose decoder ends in a non-zero status: a read past the
    end of a group's words, a final state that is not 2^31, or words left over."""
    from . import ops
    return decode_spans(_KIND, net, latents, read(data, latents.shape[0]), batch, span_groups, ops.occ_rans_decode)


def check_status(status, name="lossless_pack"):
    """ValueError naming the first group whose decoder status is not 0, in the name of the pack `name`."""
    status = np.asarray(status).reshape(-1)
    bad = np.flatnonzero(status)
    if bad.size:
        g, s = int(bad[0]), int(status[bad[0]])
        what = [text for bit, text in ((1, "a read past the end of its words"), (2, "a final state that is not 2^31"),
                                       (4, "words left over")) if s & bit]
        raise ValueError(f"{name}: the stream of group {g} is damaged ({', '.join(what)}); "
                         f"{bad.size} of {status.size} groups are")


@torch.no_grad()
def points_from_words(words, counts, origins, level=0, batch=64):
    """Occupancy words of a level ([N, 512 >> 3 * level]) + counts -> int64 [n, 3] points (origin >> level) + (z, y, x)
    in (block, raster) order (numpy): at level 0 the cloud, above it the lattice of decode --lod."""
    from . import ops
    dev = words.device
    origins = torch.as_tensor(np.asarray(origins)).to(torch.int32)
    pts = []
    for lo in range(0, words.shape[0], batch):
        hi = min(lo + batch, words.shape[0])
        pts.append(ops.points_from_bits(words[lo:hi].contiguous(), counts[lo:hi].contiguous(),
                                        origins[lo:hi].to(dev).contiguous(), 32 >> level, level).cpu())
    return torch.cat(pts, 0).long().numpy()
