"""numpy reference of the lossless occupancy coder (include/nvf_hip.h "lossless geometry", csrc/occ_rans.hip): the
context of a probability, the calibration table and the 64-lane interleaved binary rANS coder, vectorised over the
lanes.  Everything is integer arithmetic on uint64, so the device must reproduce it byte for byte."""
import numpy as np

VOX = 32768
LANES = 64
L = np.uint64(1 << 31)
_U = np.uint64


def contexts(p):
    """float32 array -> int array of contexts in [0, 256), any shape."""
    p = np.ascontiguousarray(p, np.float32)
    side = p > np.float32(0.5)
    with np.errstate(invalid="ignore"):
        q = np.where(side, np.float32(1.0) - p, p).astype(np.float32)
    key = (q.view(np.uint32) >> 21).astype(np.int64)
    idx = np.clip((0x3F000000 >> 21) - key, 0, 127)
    return 2 * idx + side.astype(np.int64)


def bad(p):
    """Voxels that are an input error: NaN, negative, over 1 (-0.0 counts as +0.0)."""
    key = np.ascontiguousarray(p, np.float32).view(np.uint32).astype(np.int64)
    key = np.where(key == 0x80000000, 0, key)
    return key > 0x3F800000


def histogram(p, gt):
    """(cnt, occ) int64 [256] over the voxels that are no input error."""
    ok = ~bad(p)
    c = contexts(p)[ok]
    g = np.asarray(gt).astype(bool)[ok]
    return np.bincount(c, minlength=256).astype(np.int64), np.bincount(c[g], minlength=256).astype(np.int64)


def table(cnt, occ):
    """f1[ctx] = clamp((2 * 65536 * occ + cnt) // (2 * cnt), 1, 65535), 32768 for an empty context; Python integers."""
    out = []
    for c, o in zip((int(v) for v in cnt), (int(v) for v in occ)):
        out.append(32768 if c == 0 else min(max((2 * 65536 * o + c) // (2 * c), 1), 65535))
    return np.asarray(out, np.int64)


def ideal_bits(f1, cnt, occ):
    f1, cnt, occ = (np.asarray(v, np.float64) for v in (f1, cnt, occ))
    return float(np.sum(-occ * np.log2(f1 / 65536.0) - (cnt - occ) * np.log2(1.0 - f1 / 65536.0)))


def padded(a, fill=0):
    """1-d array -> [steps, 64], the last step filled up with `fill` (0: idle slots)."""
    n = -(-a.size // LANES) * LANES
    return np.concatenate([a, np.full(n - a.size, fill, a.dtype)]).reshape(-1, LANES)


def encode_steps(x, out, freq, start):
    """THE encoder loop.  freq, start uint64 [steps, 64] (padded), walked backwards; freq 0 is an idle slot: the lane
    neither emits nor changes its state.  x uint64 [64] -> the states after the steps; the words of every step are
    appended to `out`, highest lane first: the last word written is the first one read (stream_words)."""
    for t in range(freq.shape[0] - 1, -1, -1):
        live = freq[t] != 0
        f = np.where(live, freq[t], _U(1))
        emit = live & (x >= (f << _U(47)))
        if emit.any():
            out.append((x[emit] & _U(0xFFFFFFFF)).astype(np.uint32)[::-1])
            x = np.where(emit, x >> _U(32), x)
        x = np.where(live, (x // f) * _U(65536) + x % f + start[t], x)
    return x


def stream_words(out):
    """What encode_steps appended -> uint32 [m] in the decoder's reading order."""
    return np.ascontiguousarray(np.concatenate(out)[::-1]) if out else np.zeros(0, np.uint32)


def decode_steps(x, words, pos, one):
    """THE decoder loop.  one uint64 [steps, 64] (padded): the frequency of a 1, 0 for an idle slot, which decodes 0 and
    keeps its state.  -> (symbols bool [steps, 64], states, words consumed so far).  IndexError on a read past the end."""
    sym = np.zeros(one.shape, bool)
    for t in range(one.shape[0]):
        o = one[t]
        live = o != 0
        slot = x & _U(0xFFFF)
        s = live & (slot < o)
        f = np.where(s, o, _U(65536) - o)
        x = np.where(live, f * (x >> _U(16)) + slot - np.where(s, _U(0), o), x)
        need = live & (x < L)
        k = int(need.sum())
        if k:
            if pos + k > words.size:
                raise IndexError("read past the end of the words")
            x[need] = (x[need] << _U(32)) | words[pos:pos + k].astype(np.uint64)
            pos += k
        sym[t] = s
    return sym, x, pos


def encode_group(p, gt, f1):
    """p float32 [n], gt bool [n] (n = blocks * 32768, one group), f1 int [256] -> (states uint64 [64], words uint32
    [m] in the decoder's reading order).  No slot is idle: a frequency is never 0."""
    one = np.asarray(f1, np.int64)[contexts(p)]
    s = np.asarray(gt).astype(bool).reshape(-1)
    out = []
    x = encode_steps(np.full(LANES, L, np.uint64), out, padded(np.where(s, one, 65536 - one).astype(np.uint64)),
                     padded(np.where(s, 0, one).astype(np.uint64)))
    return x.copy(), stream_words(out)


def decode_group(p, f1, states, words):
    """-> (symbols bool [n], final states uint64 [64], words consumed).  IndexError on a read past the end."""
    one = np.asarray(f1, np.int64)[contexts(p)].reshape(-1).astype(np.uint64)
    sym, x, pos = decode_steps(np.asarray(states, np.uint64).copy(), np.asarray(words, np.uint32), 0, padded(one))
    return sym.reshape(-1)[:one.size], x, pos


def encode(p, gt, f1, group):
    """p, gt [B, 32768] -> list of (states, words) per group of `group` blocks."""
    p = np.asarray(p, np.float32).reshape(-1, VOX)
    gt = np.asarray(gt).reshape(-1, VOX)
    return [encode_group(p[b:b + group].reshape(-1), gt[b:b + group].reshape(-1), f1) for b in range(0, p.shape[0], group)]


def occupancy_words(gt):
    """gt [B, 32768] -> uint64 [B, 512]: bit k of word w = voxel 64 w + k."""
    bits = np.asarray(gt).astype(bool).reshape(-1, 512, 64)
    return (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
