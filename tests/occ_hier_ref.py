"""numpy reference of the scalable lossless occupancy coder (include/nvf_hip.h "scalable lossless geometry",
csrc/occ_hier.hip): the pyramid, the contexts, the three sections of a group and the table.  The coder is v1's
(tests/occ_rans_ref.py: encode_steps / decode_steps, here with idle slots), and so are the context function, the input
error rule and the table rule.  Everything past the float comparisons of the pyramid is integer arithmetic on uint64,
so the device must reproduce it byte for byte."""
import numpy as np

from tests import occ_rans_ref as R

VOX = 32768
LANES = 64
CONTEXTS = 3072
BLOCK_WORDS = 512 + 4096 + 32768
L = np.uint64(1 << 31)
DIM = {0: 32, 1: 16, 2: 8}


def children(cells, d):
    """Raster indices of cells of a d^3 grid, int [n] -> int [n, 8]: their children on the (2d)^3 grid, j = 4dz+2dy+dx."""
    cells = np.asarray(cells, np.int64)
    z, y, x = cells // (d * d), (cells // d) % d, cells % d
    j = np.arange(8)
    return ((2 * z[:, None] + (j >> 2)) * 2 * d + 2 * y[:, None] + ((j >> 1) & 1)) * 2 * d + 2 * x[:, None] + (j & 1)


def _fold(v):
    """v float32 [..., 8] in child order -> (m, k): m = c0, m = cj > m ? cj : m; k = min(3, #(c > 0.5))."""
    m = v[..., 0].copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, 8):
            m = np.where(v[..., j] > m, v[..., j], m)
        k = np.minimum((v > np.float32(0.5)).sum(-1), 3)
    return m.astype(np.float32), k.astype(np.uint8)


def pyramid(p):
    """p float32 [B, 32768] -> (P1 [B, 4096], K1 uint8 [B, 4096], P2 [B, 512], K2 uint8 [B, 512])."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, VOX)
    p1, k1 = _fold(p[:, children(np.arange(4096), 16)])
    p2, k2 = _fold(p1[:, children(np.arange(512), 8)])
    return p1, k1, p2, k2


def maxpool(gt):
    """gt [B, 32768] -> the occupancy at the three levels, bool [B, 32768], [B, 4096], [B, 512] (index = level)."""
    g0 = np.asarray(gt).astype(bool).reshape(-1, VOX)
    g1 = g0[:, children(np.arange(4096), 16)].any(-1)
    g2 = g1[:, children(np.arange(512), 8)].any(-1)
    return g0, g1, g2


def words_of(g):
    """bool [B, n] (n a multiple of 64) -> uint64 [B, n / 64]: bit k of word w = cell 64 w + k."""
    bits = np.asarray(g).astype(bool).reshape(g.shape[0], -1, 64)
    return (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def section(level, p, pyr, parent_occ):
    """The symbols of one section of a group: p [nb, 32768], pyr = pyramid(p), parent_occ bool [nb, cells of level + 1]
    (None at level 2) -> (block int [n], cell int [n], ctx int [n]) in the section's order."""
    p1, k1, p2, k2 = pyr
    nb = p.shape[0]
    if level == 2:
        blk, cell = np.repeat(np.arange(nb), 512), np.tile(np.arange(512), nb)
        val, k = p2[blk, cell], k2[blk, cell]
    else:
        blk, par = np.nonzero(parent_occ)                       # (block, raster) order
        cell = children(par, DIM[level + 1]).reshape(-1)
        blk = np.repeat(blk, 8)
        if level == 1:
            val, k = p1[blk, cell], k1[blk, cell]
        else:
            val, k = p[blk, cell], np.repeat(k1[np.nonzero(parent_occ)], 8)
    ctx = (level * 4 + k.astype(np.int64)) * 256 + R.contexts(val)
    return blk, cell, ctx


def group_sections(p, gt):
    """One group: [(level, block, cell, ctx, symbol bool)] for levels 2, 1, 0."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, VOX)
    pyr, g = pyramid(p), maxpool(gt)
    out = []
    for level in (2, 1, 0):
        blk, cell, ctx = section(level, p, pyr, None if level == 2 else g[level + 1])
        out.append((level, blk, cell, ctx, g[level][blk, cell]))
    return out


def histogram(p, gt, group=None):
    """(cnt, occ) int64 [3072] over the coded symbols of all blocks (the grouping does not change them)."""
    cnt, occ = np.zeros(CONTEXTS, np.int64), np.zeros(CONTEXTS, np.int64)
    for _, _, _, ctx, sym in group_sections(p, gt):
        cnt += np.bincount(ctx, minlength=CONTEXTS)
        occ += np.bincount(ctx[sym], minlength=CONTEXTS)
    return cnt, occ


def table(cnt, occ):
    return R.table(cnt, occ)


ideal_bits = R.ideal_bits


def encode_group(p, gt, f1):
    """p float32 [nb, 32768], gt [nb, 32768] (one group), f1 int [3072] -> (states uint64 [64], words uint32 [m] in
    the decoder's reading order)."""
    f1 = np.asarray(f1, np.int64)
    x = np.full(LANES, L, np.uint64)
    out = []
    for level, _, _, ctx, sym in reversed(group_sections(p, gt)):
        one = f1[ctx]
        x = R.encode_steps(x, out, R.padded(np.where(sym, one, 65536 - one).astype(np.uint64)),
                           R.padded(np.where(sym, 0, one).astype(np.uint64)))
    return x.copy(), R.stream_words(out)


def decode_group(p, f1, states, words, stop=0):
    """-> (occupancy bool [nb, cells of level `stop`], states uint64 [64] after the last section decoded, words
    consumed).  IndexError on a read past the end."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, VOX)
    f1 = np.asarray(f1, np.int64)
    pyr = pyramid(p)
    x = np.asarray(states, np.uint64).copy()
    words = np.asarray(words, np.uint32)
    pos, occ = 0, None
    for level in (2, 1, 0):
        if level < stop:
            break
        blk, cell, ctx = section(level, p, pyr, occ)
        sym, x, pos = R.decode_steps(x, words, pos, R.padded(f1[ctx].astype(np.uint64)))
        occ = np.zeros((p.shape[0], DIM[level] ** 3), bool)
        occ[blk, cell] = sym.reshape(-1)[:blk.size]
    return occ, x, pos


def encode(p, gt, f1, group):
    """p, gt [B, 32768] -> list of (states, words) per group of `group` blocks."""
    p = np.asarray(p, np.float32).reshape(-1, VOX)
    gt = np.asarray(gt).reshape(-1, VOX)
    return [encode_group(p[b:b + group], gt[b:b + group], f1) for b in range(0, p.shape[0], group)]


def symbols_coded(p, gt):
    return sum(s[3].size for s in group_sections(p, gt))
