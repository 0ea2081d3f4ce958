"""The `lod_pack` entry of pack.pk: what a decoder needs to stop at a coarser level of detail.  Host only.

The decoder computes the cloud at three resolutions; the two coarse classifier heads (conv1_cls on the 16^3 grid =
level 1, conv0_cls on the 8^3 grid = level 2) are not among the weights a pack carries (weight_codec.keys_quantize /
keys_code_as_is), so `encode --pack_lod` adds them, with the threshold of each level:

    byte 0        version (VERSION)
    bytes 1..8    float32 t_1, t_2: the thresholds of level 1 and level 2, little-endian
    bytes 9..12   uint16 c_1, c_2: input channels of conv1_cls and of conv0_cls
    then          conv1_cls.kernel [c_1 * 27], conv1_cls.b [1], conv0_cls.kernel [c_2 * 27], conv0_cls.b [1],
                  little-endian float16

Kernel and bias are the trainable state-dict tensors; the frozen `*_init` buffers come from the seed on both sides, as
for every other layer.  The encoder rounds the four tensors to float16 BEFORE it evaluates anything at a coarse level
(round_heads_), and the decoder loads the very float16 numbers: both hold the same float32 values, and the float16
round trip is idempotent.  8 x len(lod_pack) bits go into the side information of Gross bpp.
"""
import struct

import numpy as np
import torch

VERSION = 1
HEADS = ("conv1_cls", "conv0_cls")            # level 1, level 2
_HEADER = struct.Struct("<BffHH")


def head_channels(chanstr):
    """(c_1, c_2): input channels of conv1_cls and conv0_cls for a channel string 'a,b,c,d' (or a tuple)."""
    c = tuple(int(v) for v in (chanstr.split(",") if isinstance(chanstr, str) else chanstr))
    if len(c) != 4:
        raise ValueError(f"channel string must name four widths, got {chanstr!r}")
    return c[2], c[1]


def round_f16(t):
    """float32 values of the nearest float16 (idempotent); raises on a value float16 cannot hold."""
    a = torch.as_tensor(t).detach().float().cpu()
    r = a.half()
    if not bool(torch.isfinite(r).all()):
        raise ValueError("lod_pack: a head parameter is not finite in float16")
    return r.float()


HEAD_KEYS = tuple(f"reconstructor.{h}.{p}" for h in HEADS for p in ("kernel", "b"))


def head_tensors(state):
    """{key: tensor} of the four tensors (HEAD_KEYS: kernel, b of conv1_cls; kernel, b of conv0_cls) out of a state
    dict, or KeyError naming the first missing key."""
    for k in HEAD_KEYS:
        if k not in state:
            raise KeyError(k)
    return {k: state[k] for k in HEAD_KEYS}


def round_heads_(net):
    """Round the coarse heads of `net` to float16 in place -> {key: the rounded tensor (CPU float32)}."""
    live = head_tensors(net.state_dict())
    rounded = {k: round_f16(t) for k, t in live.items()}
    with torch.no_grad():
        for k, t in live.items():
            t.copy_(rounded[k].to(t.device))
    return rounded


def write_lod_pack(t1, t2, k1, b1, k2, b2):
    """Thresholds of level 1 / 2 and the heads' tensors (conv1_cls kernel [1, c_1, 3, 3, 3], b [1]; conv0_cls kernel
    [1, c_2, 3, 3, 3], b [1]) -> bytes."""
    k1, b1, k2, b2 = (np.asarray(torch.as_tensor(v).detach().float().cpu().numpy()) for v in (k1, b1, k2, b2))
    for k, b in ((k1, b1), (k2, b2)):
        if k.ndim != 5 or k.shape[0] != 1 or k.shape[2:] != (3, 3, 3) or b.shape != (1,):
            raise ValueError(f"lod_pack: a head is a [1, c, 3, 3, 3] kernel and a [1] bias, got {k.shape} / {b.shape}")
    t = np.asarray([t1, t2], np.float32)
    if not np.all(np.isfinite(t)):
        raise ValueError("lod_pack: thresholds must be finite")
    body = b"".join(np.ascontiguousarray(v.reshape(-1)).astype("<f2").tobytes() for v in (k1, b1, k2, b2))
    return _HEADER.pack(VERSION, float(t[0]), float(t[1]), k1.shape[1], k2.shape[1]) + body


def read_lod_pack(data, chanstr=None):
    """bytes -> {'t': (t_1, t_2) floats, 'channels': (c_1, c_2), 'state': {state-dict key: float32 tensor}}.
    ValueError on a wrong version, a truncated or over-long payload, or channel counts other than `chanstr`'s."""
    data = bytes(data)
    if len(data) < 1:
        raise ValueError("lod_pack: empty")
    if data[0] != VERSION:
        raise ValueError(f"lod_pack: version {data[0]}, this reader knows {VERSION}")
    if len(data) < _HEADER.size:
        raise ValueError("lod_pack: truncated header")
    _, t1, t2, c1, c2 = _HEADER.unpack_from(data)
    if chanstr is not None and (c1, c2) != head_channels(chanstr):
        raise ValueError(f"lod_pack: heads of {c1} and {c2} channels do not fit --chanstr {chanstr} "
                         f"(conv1_cls {head_channels(chanstr)[0]}, conv0_cls {head_channels(chanstr)[1]})")
    if c1 == 0 or c2 == 0:
        raise ValueError("lod_pack: a head without channels")
    need = _HEADER.size + 2 * (27 * c1 + 1 + 27 * c2 + 1)
    if len(data) != need:
        raise ValueError(f"lod_pack: {len(data)} bytes, {need} expected for heads of {c1} and {c2} channels")
    v = np.frombuffer(data, dtype="<f2", offset=_HEADER.size).astype(np.float32)
    if not (np.all(np.isfinite(v)) and np.isfinite(t1) and np.isfinite(t2)):
        raise ValueError("lod_pack: a value is not finite")
    cut = np.cumsum([27 * c1, 1, 27 * c2])
    k1, b1, k2, b2 = np.split(v, cut)
    state = {"reconstructor.conv1_cls.kernel": torch.from_numpy(k1.reshape(1, c1, 3, 3, 3).copy()),
             "reconstructor.conv1_cls.b": torch.from_numpy(b1.copy()),
             "reconstructor.conv0_cls.kernel": torch.from_numpy(k2.reshape(1, c2, 3, 3, 3).copy()),
             "reconstructor.conv0_cls.b": torch.from_numpy(b2.copy())}
    return {"t": (float(t1), float(t2)), "channels": (c1, c2), "state": state}


def lod_line(lod, t, points, pacc=None, nacc=None):
    """The `[LoD l]` line of encode (with the accuracies against the pooled ground truth) and of decode."""
    s = "[LoD %d] t: %.9g points: %d" % (lod, float(np.float32(t)), int(points))
    if pacc is not None:
        s += " Pacc: %.4f Nacc: %.4f" % (pacc, nacc)
    return s
