"""numpy reference of the scalable lossless coder's second context model (include/nvf_hip.h "scalable lossless geometry,
neighbour contexts", csrc/occ_hier.hip): a voxel is coded under the level-1 occupancy of its parent's neighbours, which
the decoder holds before the first voxel.  Pyramid, sections, symbol order, idle slots, coder and table rule are
tests/occ_hier_ref.py's and tests/occ_rans_ref.py's; only the context of a level-0 symbol differs:

    ctx = 3072 + (n * 4 + k) * 256 + occ_ctx(p[v]),    n = (F * 4 + E) * 2 + C in [0, 32)

with F, E, C the occupied 16^3 cells of the SAME block among the three face, three edge and one corner neighbour of the
voxel's parent on the voxel's side of it (outside the block: 0).  Sections 2 and 1 keep contexts 1024..3071."""
import numpy as np

from tests import occ_hier_ref as H
from tests import occ_rans_ref as R

VOX = H.VOX
CONTEXTS = 3072 + 32 * 1024
BLOCK_WORDS = H.BLOCK_WORDS


def neighbour_class(blk, cell, occ1):
    """blk int [n], cell int [n] (raster voxels of the 32^3 grid), occ1 bool [nb, 4096] -> n int [n] in [0, 32)."""
    occ1 = np.asarray(occ1).astype(bool)
    o = np.zeros((occ1.shape[0], 18, 18, 18), np.int64)          # a border of zeros: blocks do not see each other
    o[:, 1:17, 1:17, 1:17] = occ1.reshape(-1, 16, 16, 16)
    blk, cell = np.asarray(blk, np.int64), np.asarray(cell, np.int64)
    z, y, x = cell // 1024, (cell // 32) % 32, cell % 32
    Z, Y, X = (z >> 1) + 1, (y >> 1) + 1, (x >> 1) + 1
    sz, sy, sx = 2 * (z & 1) - 1, 2 * (y & 1) - 1, 2 * (x & 1) - 1
    O = lambda a, b, c: o[blk, Z + a * sz, Y + b * sy, X + c * sx]
    F = O(1, 0, 0) + O(0, 1, 0) + O(0, 0, 1)
    E = O(1, 1, 0) + O(1, 0, 1) + O(0, 1, 1)
    return (F * 4 + E) * 2 + O(1, 1, 1)


def section(level, p, pyr, parent_occ):
    """H.section, with the neighbour class in the context of a level-0 symbol: parent_occ IS the level-1 occupancy."""
    blk, cell, ctx = H.section(level, p, pyr, parent_occ)
    if level == 0:
        ctx = 3072 + neighbour_class(blk, cell, parent_occ) * 1024 + ctx
    return blk, cell, ctx


def group_sections(p, gt):
    """One group: [(level, block, cell, ctx, symbol bool)] for levels 2, 1, 0."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, VOX)
    pyr, g = H.pyramid(p), H.maxpool(gt)
    out = []
    for level in (2, 1, 0):
        blk, cell, ctx = section(level, p, pyr, None if level == 2 else g[level + 1])
        out.append((level, blk, cell, ctx, g[level][blk, cell]))
    return out


def histogram(p, gt):
    """(cnt, occ) int64 [35840] over the coded symbols of all blocks."""
    cnt, occ = np.zeros(CONTEXTS, np.int64), np.zeros(CONTEXTS, np.int64)
    for _, _, _, ctx, sym in group_sections(p, gt):
        cnt += np.bincount(ctx, minlength=CONTEXTS)
        occ += np.bincount(ctx[sym], minlength=CONTEXTS)
    return cnt, occ


table = H.table
ideal_bits = R.ideal_bits


def encode_group(p, gt, f1):
    """One group -> (states uint64 [64], words uint32 [m] in the decoder's reading order); f1 int [35840]."""
    f1 = np.asarray(f1, np.int64)
    x = np.full(H.LANES, H.L, np.uint64)
    out = []
    for _, _, _, ctx, sym in reversed(group_sections(p, gt)):
        one = f1[ctx]
        x = R.encode_steps(x, out, R.padded(np.where(sym, one, 65536 - one).astype(np.uint64)),
                           R.padded(np.where(sym, 0, one).astype(np.uint64)))
    return x.copy(), R.stream_words(out)


def decode_group(p, f1, states, words, stop=0):
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
        blk, cell, ctx = section(level, p, pyr, occ)
        sym, x, pos = R.decode_steps(x, words, pos, R.padded(f1[ctx].astype(np.uint64)))
        occ = np.zeros((p.shape[0], H.DIM[level] ** 3), bool)
        occ[blk, cell] = sym.reshape(-1)[:blk.size]
    return occ, x, pos


def encode(p, gt, f1, group):
    """p, gt [B, 32768] -> list of (states, words) per group of `group` blocks."""
    p = np.asarray(p, np.float32).reshape(-1, VOX)
    gt = np.asarray(gt).reshape(-1, VOX)
    return [encode_group(p[b:b + group], gt[b:b + group], f1) for b in range(0, p.shape[0], group)]


def symbols_coded(p, gt):
    return H.symbols_coded(p, gt)


def held_out_bits(sections, contexts, p, gt):
    """The held-out code length of a context model (sections = group_sections of it): a table built from the even
    blocks codes the odd ones and the other way round, a frequency being clip(round(65536 (occ + 0.5) / (cnt + 1)), 1,
    65535); the summed cross-entropy in bits."""
    p = np.asarray(p, np.float32).reshape(-1, VOX)
    gt = np.asarray(gt).reshape(-1, VOX)
    halves = []
    for half in (0, 1):
        secs = sections(p[half::2], gt[half::2])
        halves.append((np.concatenate([s[3] for s in secs]), np.concatenate([s[4] for s in secs])))
    bits = 0.0
    for train, test in ((0, 1), (1, 0)):
        ctx, sym = halves[train]
        cnt, occ = np.bincount(ctx, minlength=contexts), np.bincount(ctx[sym], minlength=contexts)
        f = np.clip(np.round(65536.0 * (occ + 0.5) / (cnt + 1.0)), 1, 65535) / 65536.0
        ctx, sym = halves[test]
        bits += float(-np.log2(np.where(sym, f[ctx], 1.0 - f[ctx])).sum())
    return bits
