"""numpy reference of the scalable lossless coder's third context model (include/nvf_hip.h "scalable lossless geometry,
inter contexts", csrc/occ_hier.hip): a voxel is coded under a reference cloud that both sides hold -- the previous
frame's decoded output, say -- as well as under the level-1 occupancy of its parent's neighbours.  Pyramid, sections,
symbol order, idle slots, coder and table rule are tests/occ_hier_ref.py's and tests/occ_rans_ref.py's; only the context
of a level-0 symbol differs:

    ctx = 3072 + (t * 4 + k) * 256 + occ_ctx(p[v]),    t = r * 16 + s in [0, 48)

r = 2 where the reference holds v itself, 1 where it holds one of v's six face neighbours, else 0 (the reference of the
SAME block; outside the block: 0); s = (F * 2 + (E > 0)) * 2 + C with F, E, C of tests/occ_nbr_ref.py.  The reference
travels as bool [nb, 32768] here and as words (H.words_of) on the device."""
import numpy as np

from tests import occ_hier_ref as H
from tests import occ_nbr_ref as N
from tests import occ_rans_ref as R

VOX = H.VOX
CONTEXTS = 3072 + 48 * 1024
BLOCK_WORDS = H.BLOCK_WORDS


def reference_words(points, origins):
    """points int [M, 3], origins int [nb, 3] (multiples of 32, distinct) -> (occupancy bool [nb, 32768], dropped): a
    point q sets voxel ((q0 & 31) * 32 + (q1 & 31)) * 32 + (q2 & 31) of the block whose origin is q & ~31; a point under
    no block is dropped and counted.  H.words_of gives the words."""
    points = np.asarray(points, np.int64).reshape(-1, 3)
    origins = np.asarray(origins, np.int64).reshape(-1, 3)
    block_of = {tuple(o): b for b, o in enumerate(origins.tolist())}
    ref = np.zeros((origins.shape[0], VOX), bool)
    dropped = 0
    for q in points.tolist():
        b = block_of.get((q[0] & ~31, q[1] & ~31, q[2] & ~31))
        if b is None or min(q) < 0:
            dropped += 1
        else:
            ref[b, ((q[0] & 31) * 32 + (q[1] & 31)) * 32 + (q[2] & 31)] = True
    return ref, dropped


def temporal_class(blk, cell, ref):
    """blk int [n], cell int [n] (raster voxels of the 32^3 grid), ref bool [nb, 32768] -> r int [n] in {0, 1, 2}."""
    ref = np.asarray(ref).astype(bool).reshape(-1, VOX)
    o = np.zeros((ref.shape[0], 34, 34, 34), np.int64)           # a border of zeros: blocks do not see each other
    o[:, 1:33, 1:33, 1:33] = ref.reshape(-1, 32, 32, 32)
    blk, cell = np.asarray(blk, np.int64), np.asarray(cell, np.int64)
    z, y, x = cell // 1024 + 1, (cell // 32) % 32 + 1, cell % 32 + 1
    a = o[blk, z, y, x]
    f = o[blk, z - 1, y, x] + o[blk, z + 1, y, x] + o[blk, z, y - 1, x] + o[blk, z, y + 1, x] + o[blk, z, y, x - 1] + \
        o[blk, z, y, x + 1]
    return np.where(a > 0, 2, (f > 0).astype(np.int64))


def spatial_class(blk, cell, occ1):
    """-> s int [n] in [0, 16): tests/occ_nbr_ref.py's class n = (F * 4 + E) * 2 + C with E folded to a bit."""
    n = N.neighbour_class(blk, cell, occ1)
    F, E, C = n >> 3, (n >> 1) & 3, n & 1
    return (F * 2 + (E > 0)) * 2 + C


def section(level, p, pyr, parent_occ, ref):
    """H.section, with the temporal and the spatial class in the context of a level-0 symbol."""
    blk, cell, ctx = H.section(level, p, pyr, parent_occ)
    if level == 0:
        t = temporal_class(blk, cell, ref) * 16 + spatial_class(blk, cell, parent_occ)
        ctx = 3072 + t * 1024 + ctx
    return blk, cell, ctx


def group_sections(p, gt, ref):
    """One group: [(level, block, cell, ctx, symbol bool)] for levels 2, 1, 0."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, VOX)
    pyr, g = H.pyramid(p), H.maxpool(gt)
    out = []
    for level in (2, 1, 0):
        blk, cell, ctx = section(level, p, pyr, None if level == 2 else g[level + 1], ref)
        out.append((level, blk, cell, ctx, g[level][blk, cell]))
    return out


def histogram(p, gt, ref):
    """(cnt, occ) int64 [52224] over the coded symbols of all blocks."""
    cnt, occ = np.zeros(CONTEXTS, np.int64), np.zeros(CONTEXTS, np.int64)
    for _, _, _, ctx, sym in group_sections(p, gt, ref):
        cnt += np.bincount(ctx, minlength=CONTEXTS)
        occ += np.bincount(ctx[sym], minlength=CONTEXTS)
    return cnt, occ


table = H.table
ideal_bits = R.ideal_bits


def encode_group(p, gt, ref, f1):
    """One group -> (states uint64 [64], words uint32 [m] in the decoder's reading order); f1 int [52224]."""
    f1 = np.asarray(f1, np.int64)
    x = np.full(H.LANES, H.L, np.uint64)
    out = []
    for _, _, _, ctx, sym in reversed(group_sections(p, gt, ref)):
        one = f1[ctx]
        x = R.encode_steps(x, out, R.padded(np.where(sym, one, 65536 - one).astype(np.uint64)),
                           R.padded(np.where(sym, 0, one).astype(np.uint64)))
    return x.copy(), R.stream_words(out)


def decode_group(p, ref, f1, states, words, stop=0):
    """-> (occupancy bool [nb, cells of level `stop`], states after the last section decoded, words consumed).
    IndexError on a read past the end."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, VOX)
    f1 = np.asarray(f1, np.int64)
    pyr = H.pyramid(p)
    x = np.asarray(states, np.uint64).copy()
    words = np.asarray(words, np.uint32)
    pos, occ = 0, None
    for level in (2, 1, 0):
        if level < stop:
            break
        blk, cell, ctx = section(level, p, pyr, occ, ref)
        sym, x, pos = R.decode_steps(x, words, pos, R.padded(f1[ctx].astype(np.uint64)))
        occ = np.zeros((p.shape[0], H.DIM[level] ** 3), bool)
        occ[blk, cell] = sym.reshape(-1)[:blk.size]
    return occ, x, pos


def encode(p, gt, ref, f1, group):
    """p, gt, ref [B, 32768] -> list of (states, words) per group of `group` blocks."""
    p = np.asarray(p, np.float32).reshape(-1, VOX)
    gt = np.asarray(gt).reshape(-1, VOX)
    ref = np.asarray(ref).reshape(-1, VOX)
    return [encode_group(p[b:b + group], gt[b:b + group], ref[b:b + group], f1) for b in range(0, p.shape[0], group)]


def symbols_coded(p, gt):
    return H.symbols_coded(p, gt)


def shifted(gt, dz, dy, dx):
    """gt [nb, 32768] moved by (dz, dy, dx) voxels inside each block, zero fill."""
    g = np.asarray(gt).astype(bool).reshape(-1, 32, 32, 32)
    out = np.zeros_like(g)
    src = [slice(max(-d, 0), 32 - max(d, 0)) for d in (dz, dy, dx)]
    dst = [slice(max(d, 0), 32 - max(-d, 0)) for d in (dz, dy, dx)]
    out[:, dst[0], dst[1], dst[2]] = g[:, src[0], src[1], src[2]]
    return out.reshape(-1, VOX)


def held_out_bits(p, gt, ref):
    """N.held_out_bits for this model: the reference's blocks split with the cloud's."""
    p = np.asarray(p, np.float32).reshape(-1, VOX)
    gt = np.asarray(gt).reshape(-1, VOX)
    ref = np.asarray(ref).reshape(-1, VOX)
    halves = iter([ref[0::2], ref[1::2]])
    return N.held_out_bits(lambda ph, gh: group_sections(ph, gh, next(halves)), CONTEXTS, p, gt)
