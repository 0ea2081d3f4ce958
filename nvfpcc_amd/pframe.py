"""Latents-only packs: a cloud coded under the frozen decoder of ANOTHER pack.

The decoder's weights are most of a pack.  A reference pack (an "I" pack: a plain pack or a group) carries them; a "P"
pack carries what a frame adds -- latents and side packs -- and, in place of `net_weight_pack`, 33 bytes that name the
decoder it was fitted under:

    {'ref_pack': version 1 | sha256 of the reference's net_weight_pack (32 bytes), ...every other key of the pack}

`join` puts the reference's `net_weight_pack` back, and the result is an ordinary plain or group pack: everything behind
it (decode, --frame, --lod, --lossless, --lossless_lod, gof.extract) reads it as before.  The digest covers exactly what
NVFPCC._decoder_from_pack reads from `net_weight_pack`, so two packs of one digest rebuild the same decoder bit for bit.
A P pack cannot be a reference (no chains).  Host only: numpy and hashlib.
"""
import hashlib
import struct

import numpy as np

VERSION = 1
DIGEST_BYTES = 32
REF_PACK_BYTES = 1 + DIGEST_BYTES       # what a P pack pays for its decoder


def _feed(h, tag, data):
    """One length-prefixed field: no two different field lists give the same byte string."""
    data = bytes(data)
    h.update(tag + struct.pack('<Q', len(data)) + data)


def _feed_array(h, tag, a):
    a = np.ascontiguousarray(np.asarray(a))
    shape = (1,) if a.ndim == 0 else a.shape
    a = a.reshape(shape).astype(a.dtype.newbyteorder('<'))
    _feed(h, tag, a.dtype.str.encode() + struct.pack('<B', a.ndim) + struct.pack(f'<{a.ndim}q', *a.shape) + a.tobytes())


def digest(net_weight_pack):
    """32 bytes: SHA-256 over a canonical serialisation of everything _decoder_from_pack reads from a net_weight_pack --
    the bit stream, the codebook (sorted by codeword), the element count, the shape list, both key lists and the as-is
    pool (dtype, shape and little-endian bytes of each array).  It does not depend on how the dict was pickled."""
    wp = net_weight_pack
    h = hashlib.sha256()
    _feed(h, b'B', wp['bit_stream'])
    book = sorted((str(k), int(v)) for k, v in wp['inv_codebook'].items())
    _feed(h, b'C', b''.join(struct.pack('<I', len(k)) + k.encode() + struct.pack('<q', v) for k, v in book))
    _feed(h, b'N', struct.pack('<q', int(wp['element_length'])))
    shapes = [tuple(int(d) for d in s) for s in wp['shape_list']]
    _feed(h, b'S', b''.join(struct.pack('<B', len(s)) + struct.pack(f'<{len(s)}q', *s) for s in shapes))
    for tag, keys in ((b'Q', wp['keys_quantize']), (b'K', wp['keys_code_as_is'])):
        _feed(h, tag, b''.join(struct.pack('<I', len(k.encode())) + k.encode() for k in keys))
    _feed(h, b'n', struct.pack('<q', len(wp['as_is_pool'])))
    for a in wp['as_is_pool']:
        _feed_array(h, b'A', a)
    return h.digest()


def split(pack):
    """A plain or group pack -> its P pack: 'ref_pack' first, then every other key in order, no net_weight_pack."""
    if 'net_weight_pack' not in pack:
        raise ValueError("split: the pack holds no net_weight_pack")
    return {'ref_pack': bytes([VERSION]) + digest(pack['net_weight_pack']),
            **{k: v for k, v in pack.items() if k != 'net_weight_pack'}}


def is_p_pack(pack):
    return 'ref_pack' in pack


def ref_digest(p_pack):
    """The digest a P pack names.  ValueError on a pack without ref_pack, another version byte or a wrong length."""
    ref = p_pack.get('ref_pack')
    if ref is None:
        raise ValueError("the pack holds no ref_pack: it is not a latents-only pack")
    ref = bytes(ref)
    if len(ref) < 1 or ref[0] != VERSION:
        raise ValueError(f"ref_pack: version {ref[0] if ref else None}, this decoder reads version {VERSION}")
    if len(ref) != REF_PACK_BYTES:
        raise ValueError(f"ref_pack: {len(ref)} bytes, version {VERSION} takes {REF_PACK_BYTES}")
    return ref[1:]


def join(p_pack, ref_pack):
    """P pack + its reference -> the plain or group pack `split` was given: the reference's net_weight_pack first,
    then the P pack's keys without 'ref_pack'.  ValueError: the reference has no net_weight_pack (a P pack cannot be a
    reference), an unknown version byte, or the reference's decoder is not the one the P pack was fitted under."""
    want = ref_digest(p_pack)
    if 'net_weight_pack' not in ref_pack:
        raise ValueError("the reference holds no net_weight_pack" +
                         (": it is a latents-only pack itself, and those do not chain" if is_p_pack(ref_pack) else ""))
    got = digest(ref_pack['net_weight_pack'])
    if got != want:
        raise ValueError(f"the reference's decoder (sha256 {got.hex()[:16]}..) is not the one this pack was fitted under "
                         f"({want.hex()[:16]}..)")
    return {'net_weight_pack': ref_pack['net_weight_pack'], **{k: v for k, v in p_pack.items() if k != 'ref_pack'}}


def pack_origins(pack):
    """int64 [n, 3]: the leaf origins of a plain pack, or of all frames of a group in order (origins / octree_pack)."""
    if 'frames' in pack:
        parts = [pack_origins(f) for f in pack['frames']]
        return np.concatenate(parts, 0) if parts else np.zeros((0, 3), np.int64)
    if 'octree_pack' in pack:
        from .preprocess import read_octree_pack
        return np.asarray(read_octree_pack(pack['octree_pack']), np.int64).reshape(-1, 3)
    return np.asarray(pack['origins'], np.int64).reshape(-1, 3)


def warm_start(ref_emb, ref_origins, origins):
    """Start table of a frame's latents from a reference frame's: a block whose origin occurs among the reference's
    takes that row; any other block the row of the nearest reference origin by L1 distance, ties to the lowest index
    (a repeated reference origin likewise: its first row).  ref_emb [m, ...], ref_origins [m, 3], origins [n, 3] ->
    [n, ...] of ref_emb's type (numpy array or torch tensor).  ValueError on an empty reference."""
    ro = np.asarray(ref_origins, np.int64).reshape(-1, 3)
    og = np.asarray(origins, np.int64).reshape(-1, 3)
    if ro.shape[0] == 0 or len(ref_emb) != ro.shape[0]:
        raise ValueError(f"warm_start: {len(ref_emb)} reference rows for {ro.shape[0]} reference origins (at least one "
                         f"of each, as many of one as of the other)")
    idx = np.empty(og.shape[0], np.int64)
    for lo in range(0, og.shape[0], 1024):       # [1024, m] distances at a time; argmin takes the lowest index of a tie
        d = np.abs(og[lo:lo + 1024, None, :] - ro[None, :, :]).sum(-1)
        idx[lo:lo + 1024] = d.argmin(1)
    if isinstance(ref_emb, np.ndarray):
        return ref_emb[idx].copy()
    import torch
    return ref_emb[torch.from_numpy(idx).to(ref_emb.device)].clone()
