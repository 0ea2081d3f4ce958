"""Which kernel form each decoder layer runs on, and which packed weights it holds for that.

engine.plan_step decides which launches a step consists of; this module decides the kernel FORM inside the per-layer
launches: the packings a layer keeps (PACKS, layer_packs) and, per pass, the form, packing, tile variant and plane-pair
count a call takes (conv_fwd, convT_fwd, conv_dx, convT_dx, conv_wgrad).  Everything here is a function of strings, small
integers and booleans -- no tensors, no library -- so tests/test_routes.py checks every combination without a device.

A decoder class fixes its layers' shapes ("narrow" = --chanstr 8,16,8,8, "wide" = 16,32,16,16; the latents are 2^3, so
conv1 maps 19^3 -> 16^3 and conv2 35^3 -> 32^3), and a layer's name stands for them.  The one free shape is the number of
latent channels, up0's input.  "generic" is any other --chanstr: the shape-generic kernels only.

Contract of the forward routes: train=False (evaluation, encode, decode) never takes a form with another summation order
-- Winograd, CONVT_ROWS, S2K5_SPLIT_G -- and its form does not depend on the batch (only the tile variant may, and every
variant of a form runs the same per-output fmaf chain).  Encode at any batch == decode at batch 1 rests on this.
"""
import functools
from typing import NamedTuple

# The 64-block boundary: up to here the batch-16 tiles, above it the tiles (or the VALU kernels) of a full batch.  The
# library's own choice by batch inside nvf_convT3d_k5s2_fwd / nvf_conv3d_gather switches at the same point
# (csrc/conv_direct.hip; tests/test_gpu_decode_bits.py, tests/test_gpu_batch_edges.py run both sides)
BATCH_SWITCH = 64

# ---------------------------------------------------------------------------------------------------------- packings
# pair axis of the three nvf_pack_mfma_k4 packings: it is their pack kind AND the pair_axis conv3d_k4_mfma is called with.
# backward-data mapping: rows pair outputs along z with 4x4 patches (conv1) or along x with flattened 18-cell rows (conv2;
# faster than the VALU kernel only while the batch is small)
PAIR_AXIS = {"k4_fwd": 0, "k4_dx_z": 2, "k4_dx_x": 0}


class Pack(NamedTuple):
    src: str        # the prepared layout it is packed from, "w_fwd" | "w_bwd".  (c0, c1) of its pack job are the (input,
                    # output) channels of that gather: the layer's (cin, cout) for w_fwd, (cout, cin) for w_bwd
    kind: object    # pack kind of pack_jobs_desc (csrc/pack_mfma.h); {kernel size: kind} for the 16-row gather forms
    floats: str     # the library's nvf_pack_<floats>_floats gives its size ...
    args: object    # ... called with these of (c0, c1, k)


G16_KIND = {4: 30, 5: 31}
# A kind-12 packing holds 65 A fragments of 64 floats per group of 4 input channels.  The library exports no
# nvf_pack_*_floats for it: the other definition of this size is pack_jobs_desc in csrc/pack_mfma.h
CONVT_ROWS_FRAGMENT_FLOATS = 65 * 64

# In the job order of nvf_pack_mfma_all / nvf_step_head: packing by packing in THIS order, layers in table order.
PACKS = {
    # matrix-core form of the narrow 4^3 convolutions: MFMA A-fragments, re-packed after every weight preparation
    "k4_fwd": Pack("w_fwd", PAIR_AXIS["k4_fwd"], "mfma_k4", lambda c0, c1, k: (c0, PAIR_AXIS["k4_fwd"])),
    "k4_dx_z": Pack("w_bwd", PAIR_AXIS["k4_dx_z"], "mfma_k4", lambda c0, c1, k: (c0, PAIR_AXIS["k4_dx_z"])),
    "k4_dx_x": Pack("w_bwd", PAIR_AXIS["k4_dx_x"], "mfma_k4", lambda c0, c1, k: (c0, PAIR_AXIS["k4_dx_x"])),
    # the Winograd (y, x) form: kind 40 with 8 -> 8 channels (conv_wino.hip), kind 41 with 16 -> 16 (conv16_wino.hip)
    "wino_dx": Pack("w_bwd", 40, "wino_k4", lambda c0, c1, k: ()),
    "wino16_dx": Pack("w_bwd", 41, "wino16_k4", lambda c0, c1, k: ()),
    "wino_fwd": Pack("w_fwd", 40, "wino_k4", lambda c0, c1, k: ()),
    "wino16_fwd": Pack("w_fwd", 41, "wino16_k4", lambda c0, c1, k: ()),
    # matrix-core form of the narrow padding-0 transposed convolutions: forward ...
    "convT": Pack("w_fwd", 10, "convT_mfma", lambda c0, c1, k: (c0,)),
    # ... the forward of TRAINING steps with the kx = 4 taps on rows (co, ey): 65 instead of 75 A fragments per channel
    # group, another summation order for the even x outputs (pack kind 12, kernel variant 15) ...
    "convT_rows": Pack("w_fwd", 12, None, None),
    # ... and backward-data (a stride-2 gather convolution with cin output channels)
    "s2k5_dx": Pack("w_bwd", 20, "s2k5_mfma", lambda c0, c1, k: (c0, c1)),
    # 16-row gather forms (conv16_mfma.hip): kind 30 (k = 4) / 31 (k = 5), c0 = input channels of the gather, c1 = its
    # output channels
    "g16_fwd": Pack("w_fwd", G16_KIND, "g16_mfma", lambda c0, c1, k: (c0, c1, k)),
    "g16_dx": Pack("w_bwd", G16_KIND, "g16_mfma", lambda c0, c1, k: (c0, c1, k)),
    "convT16": Pack("w_fwd", 11, "convT16_mfma", lambda c0, c1, k: (c0, c1)),
}


def pack_job(pack, cin, cout, k):
    """(pack kind, c0, c1) of the layer's pack job, as pack_jobs_desc takes them."""
    P = PACKS[pack]
    c0, c1 = (cin, cout) if P.src == "w_fwd" else (cout, cin)
    return (P.kind[k] if P.kind is G16_KIND else P.kind), c0, c1


def pack_floats(library, pack, cin, cout, k):
    """Size of the layer's packing in floats; ``library``: the loaded C library (_lib.lib())."""
    P = PACKS[pack]
    _, c0, c1 = pack_job(pack, cin, cout, k)
    if P.floats is None:
        return (c0 // 4) * CONVT_ROWS_FRAGMENT_FLOATS
    return int(getattr(library, "nvf_pack_%s_floats" % P.floats)(*P.args(c0, c1, k)))


# (decoder class, layer) -> (packings it always holds, packings it holds with winograd)
_NARROW_UP = (("convT", "s2k5_dx"), ("convT_rows",))
# wide decoder (16 / 32 channels): the output channels are the MFMA rows (conv16_mfma.hip) -- conv1 / conv2 forward and
# backward-data, and the backward-data of the transposed convolutions (stride-2 gather with cin output channels)
_WIDE_UP = (("g16_dx", "convT16"), ())
_LAYER_PACKS = {
    ("narrow", "up1"): _NARROW_UP,
    ("narrow", "up2"): _NARROW_UP,
    # backward-data in the reduced-multiplication form (Winograd over (y, x), z pairs on the matrix cores: 52 us against
    # 85 for the direct form at batch 16) and the forward of TRAINING steps (mode 'train': NVFPCC.py:160, 234)
    ("narrow", "conv1"): (("k4_fwd", "k4_dx_z"), ("wino_dx", "wino_fwd")),
    ("narrow", "conv2"): (("k4_fwd", "k4_dx_x"), ("wino_dx", "wino_fwd")),
    ("wide", "up0"): _WIDE_UP,          # with 8 latent channels only (_tuned): 16 -> 8 channels, rows 8..15 zero
    ("wide", "conv0"): _WIDE_UP,
    ("wide", "up1"): _WIDE_UP,
    ("wide", "up2"): _WIDE_UP,
    # the Winograd (y, x) form with the 16 output channels as MFMA rows (conv16_wino.hip), training steps only: conv2
    # backward-data 257 -> 140 us, forward 170 -> 95, conv1 backward-data 59 -> 33 at batch 16.
    # conv1's FORWARD stays direct (27 -> 25 us would cost the engine == operator-path agreement its 2e-5: measured
    # 2.004e-5), so only conv2 gets a forward packing -- and a pack-job slot stays free
    ("wide", "conv1"): (("g16_fwd", "g16_dx"), ("wino16_dx",)),
    ("wide", "conv2"): (("g16_fwd", "g16_dx"), ("wino16_dx", "wino16_fwd")),
}
WIDE_UP0_LATENT_CHANNELS = 8      # the one instantiation of the wide up0's matrix-core kernels


def _tuned(decoder_class, name, cin):
    """The layer runs on its class's matrix-core kernels.  Every shape but one follows from the class; the free one is
    the wide up0's input, the latent channels."""
    return ((decoder_class, name) in _LAYER_PACKS
            and ((decoder_class, name) != ("wide", "up0") or cin == WIDE_UP0_LATENT_CHANNELS))


def layer_packs(decoder_class, winograd, name, cin, cout, k, pad):
    """Names of the packings the layer holds, in PACKS order.  (cout, k, pad) follow from the class and the name."""
    if not _tuned(decoder_class, name, cin):
        return ()
    always, wino = _LAYER_PACKS[decoder_class, name]
    held = always + (wino if winograd else ())
    return tuple(p for p in PACKS if p in held)


# ------------------------------------------------------------------------------------------------------------ routes
# Tile variants, as the C entry points take them.  None = the module default (ops.set_mfma_variant).  Every variant of a
# form gives the same bits except the two marked "another summation order".
K4_8X4 = 5            # conv3d_k4_mfma: 8 rows x 4 planes on eight waves
CONVT_8WAVES = 5      # convT3d_k5s2_mfma: eight waves with one column tile each (two waves per SIMD)
CONVT_ROWS = 15       # convT3d_k5s2_mfma on a convT_rows packing: another summation order for the even x outputs
S2K5_2PLANES = 2      # conv3d_s2k5_mfma: two planes per wave
S2K5_4X4 = 5          # conv3d_s2k5_mfma: 4 rows x 4 planes on eight waves
S2K5_8X2 = 6          # conv3d_s2k5_mfma: 8 rows x 2 planes on eight waves
S2K5_SPLIT_G = 7      # conv3d_s2k5_mfma: the two channel groups of g on different waves -- another summation order

# forms that only a training step may take (the module docstring's contract)
WINOGRAD_FORMS = ("wino_fwd", "wino16_fwd", "wino_bwd", "wino16_bwd", "wino16_partial")
REORDERING_VARIANTS = (("convT_mfma", CONVT_ROWS), ("s2k5_mfma", S2K5_SPLIT_G))
# forms of the shape-generic kernels: they read w_fwd / w_bwd, no packing
GENERIC_FORMS = ("gather", "convT_fwd", "tiled")


class Route(NamedTuple):
    form: str                   # which ops entry point
    pack: str = None            # the packing it reads (None: w_fwd / w_bwd)
    variant: int = None
    ppc: int = 0                # Winograd forms: plane pairs per work unit (0: the kernel's batch-16 default; an explicit
                                # count without bit 16 = the two-set kernel of conv_wino.hip).  Every choice: the same bits
    bias_slabs: bool = False    # the launch leaves the channel sums of what it stored as slabs


class WgradRoute(NamedTuple):
    form: str
    zsplit: int = 0


@functools.lru_cache(maxsize=None)
def conv_fwd(decoder_class, winograd, name, batch, train, act_is_relu):
    """Forward of a stride-1 convolution."""
    big = batch > BATCH_SWITCH
    wino = winograd and train and act_is_relu
    # the Winograd forward serves TRAINING steps only; the eval / encode / decode forward keeps the direct fixed-order
    # kernel (bit-exact batch invariance, the occupancy contract)
    if (decoder_class, name) == ("narrow", "conv2"):
        if wino:
            # (a full-batch launch has workgroups to spare: more plane pairs per work unit repeat fewer plane transforms --
            # conv2 at batch 917: 1667 -> 1481 us with 8 pairs per unit; the same bits, tools/wino_ppc_sweep.py)
            # (above batch 64 the two-set kernel with all 16 pairs: 1480 us against 1507 for the one-set kernel with 8)
            return Route("wino_fwd", "wino_fwd", ppc=16 if big else 0)
        return Route("k4_mfma", "k4_fwd")
    if (decoder_class, name) == ("narrow", "conv1"):
        # conv1's training FORWARD in the Winograd form: measured slower at batch 16 -- 19.1 us two-set / 16.7 us one-set
        # kernel against 12.2 us for the direct kernel, r05 A/B -- 16^3 outputs do not amortise the transforms; used above
        # batch 64 only (the full-batch latent step: 207 us against 375 for the direct kernel at batch 917)
        if wino and big:
            return Route("wino_fwd", "wino_fwd", ppc=8)      # the two-set kernel, all eight plane pairs per unit
        # conv1 at large batch: 8 rows x 4 planes on eight waves (variant 5: 34.2 vs 39.4 us at batch 64, 107 vs 120
        # (variant 2) at 256, 402 vs 443 at 917; at batch 16 the default tile: 12.7 vs 17.6).  Every variant runs
        # the same per-output fmaf chain, so the bits -- and encode-at-any-batch == decode-at-batch-1 -- do not change
        # (eval_forward at 66 blocks against batch 1: tests/test_gpu_decode_bits.py)
        return Route("k4_mfma", "k4_fwd", variant=K4_8X4 if batch >= BATCH_SWITCH else None)
    if (decoder_class, name) == ("wide", "conv2") and wino:
        return Route("wino16_fwd", "wino16_fwd")
    if (decoder_class, name) in (("wide", "conv1"), ("wide", "conv2")):
        return Route("g16", "g16_fwd")
    return Route("gather")


@functools.lru_cache(maxsize=None)
def convT_fwd(decoder_class, winograd, name, cin, train):
    """Forward of a k5 s2 transposed convolution."""
    if not _tuned(decoder_class, name, cin):
        return Route("convT_fwd")
    if decoder_class == "wide":
        return Route("convT16", "convT16")
    # eight waves with one column tile each (variant 5: two waves per SIMD; up1 19.3 -> 15.6 us, up2 34.0 -> 30.7 at
    # batch 16 -- and at batch 917 (the full-batch latent step; r05 sweep): up2 1115 -> 916 us, up1 389 -> 310;
    # every variant runs the same per-output fmaf chain: bit-identical)
    if train and winograd:
        return Route("convT_mfma", "convT_rows", variant=CONVT_ROWS)     # evaluation / encode / decode keep "convT"
    return Route("convT_mfma", "convT", variant=CONVT_8WAVES)


@functools.lru_cache(maxsize=None)
def conv_dx(decoder_class, winograd, name, batch, masked, has_addend, want_bias_slabs):
    """Backward-data of a stride-1 convolution.  ``masked`` / ``has_addend``: through the ReLU mask of the layer below /
    plus the heads' share; ``want_bias_slabs``: the caller has a use for the channel sums of what this pass writes (the
    bias gradient of the layer below)."""
    big = batch > BATCH_SWITCH
    plain = masked and not has_addend          # what the Winograd kernels and the slab epilogues compute
    if (decoder_class, name) in (("wide", "conv1"), ("wide", "conv2")):
        if winograd and plain:
            # (the channel sums of dx -- the bias gradient of the layer below -- from this kernel's epilogue, bias_part=:
            # measured neutral, the reduction launch 48.9 -> 44.0 us against + 2.7 / + 2.1 us in the two epilogues)
            return Route("wino16_bwd", "wino16_dx")
        return Route("g16", "g16_dx")
    if (decoder_class, name) in (("narrow", "conv1"), ("narrow", "conv2")):
        if winograd and plain:
            if want_bias_slabs and not big:
                # (one slab of 8 sums per work unit: 126 units per block in conv2's default kernel, conv_wino1.hip)
                return Route("wino_bwd", "wino_dx", bias_slabs=True)
            # Plane pairs per work unit at a full batch.  Every choice gives the same bits; batch 917: conv2
            # 2182 -> 1945 us, conv1 569 -> 387 us (tools/wino_ppc_sweep.py, tools/wino_bench.py --batch 917).
            # (conv1: the two-set kernel of conv_wino.hip, all ten plane pairs per unit -- 387 us against 466 for the
            # one-set kernel with 5 at batch 917, tools/wino_bench.py --fwd --batch 917; the same bits)
            # (conv2 likewise: all 18 pairs in the two-set kernel 1945 us, one-set kernel with 9 / 18: 2203 / 2098 in the
            # same run)
            return Route("wino_bwd", "wino_dx", ppc=0 if not big else 18 if name == "conv2" else 10)
        if not big:
            return Route("k4_mfma", "k4_dx_z" if name == "conv1" else "k4_dx_x", bias_slabs=want_bias_slabs and plain)
        # (above batch 64 the VALU tile kernel is faster for both: conv1 222 vs 367 us, conv2 1167 vs 1234 us at batch 256)
    return Route("gather")


@functools.lru_cache(maxsize=None)
def convT_dx(decoder_class, winograd, name, cin, batch):
    """Backward-data of a k5 s2 transposed convolution (a stride-2 gather convolution)."""
    big = batch > BATCH_SWITCH
    if not _tuned(decoder_class, name, cin):
        return Route("gather")
    if decoder_class == "wide":
        return Route("g16", "g16_dx")
    if name == "up1":
        # up1 at large batch: two planes per wave (variant 2: 55 vs 63 us at batch 256; 173 vs 184 at 917)
        # up1 in training steps of the default engine: the two channel groups of g on different waves, 256 workgroups of
        # 2 rows x 2 planes (variant 7: another summation order, so not in the strict-trajectory engine)
        return Route("s2k5_mfma", "s2k5_dx", variant=S2K5_2PLANES if big else S2K5_SPLIT_G if winograd else None)
    # up2 at batch <= 64: 8 rows x 2 planes on eight waves (variant 6: 25.3 -> 22.8 us at batch 16; bit-identical;
    # nvf_conv3d_gather's own choice by batch for these layers is held by tests/test_gpu_decode_bits.py);
    # above: 4 rows x 4 planes on eight waves (variant 5: 1027 vs 1149 us at batch 917)
    return Route("s2k5_mfma", "s2k5_dx", variant=S2K5_4X4 if big else S2K5_8X2)


@functools.lru_cache(maxsize=None)
def conv_wgrad(decoder_class, winograd, name):
    """Weight gradient of a stride-1 convolution outside the one-launch groupings."""
    if winograd and (decoder_class, name) in (("wide", "conv1"), ("wide", "conv2")):
        # the Winograd (y, x) form (wgrad16_wino.hip): slabs for the common reduction (conv2 172 -> 100 us at batch 16)
        return WgradRoute("wino16_partial", zsplit=0 if name == "conv2" else 8)
    return WgradRoute("tiled")
