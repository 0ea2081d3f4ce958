"""What tests/golden/conformance_{S,W}.npz holds and how it is read: shared by tools/make_conformance_fixture.py (the
writer), tests/test_conformance_cpu.py and tests/test_gpu_conformance.py.  The host half (digests, the sampled-bits
diagnosis, contexts of the pooled levels from the committed voxel contexts) needs numpy only; the builders at the end
need a device and import the package where they are called.

Contexts of the scalable coders from `ctx0` alone.  occ_ctx (tests/occ_rans_ref.contexts) is 2 * idx + side with
side = p > 0.5 and idx falling in p below 0.5 and rising in p above it, so rank(ctx) = 128 + idx where side else
127 - idx never falls when p rises.  The pyramid takes a maximum of eight values by comparisons only: the context of
the maximum is the context of highest rank among the children, and K counts the children with side = 1.  Any float32
field with the same voxel contexts that is strictly increasing in rank therefore gives the coders the very contexts the
device's field gives them at all three levels: `surrogate_p` is such a field, built from `ctx0` on the host, and
tests/occ_hier_ref.py / tests/occ_nbr_ref.py decode the committed streams under it without a single committed float."""
import hashlib
import os

import numpy as np

TAGS = ("S", "W")
N_BLOCKS = 12
VOX = 32768
GROUPS = (64, 2)                # one partial group; six groups
ENCODE_BATCH = 5
SAMPLE_STRIDE = 61              # every 61st voxel of every block
CODERS = ("lossless", "lossless_lod", "lossless_nbr")
VERSION_BYTES = {"lossless": 1, "lossless_lod": 1, "lossless_nbr": 3, "lod_pack": 1}
HEAD_SAMPLES = {"cls1": np.arange(0, 4096, 7), "cls0": np.arange(0, 512, 3)}
SIZE_CAP = 503196               # tests/golden/net_S.npz, the largest golden before these


def fixture_path(golden_dir, tag):
    return os.path.join(golden_dir, f"conformance_{tag}.npz")


def load(golden_dir, tag):
    with np.load(fixture_path(golden_dir, tag)) as f:
        return {k: f[k] for k in f.files}


def ground_truth():
    """bool [12, 32768]: the occupancy the packs code, from numpy alone."""
    from nvfpcc_amd.synth import make_blocks
    return make_blocks(N_BLOCKS)[0].reshape(N_BLOCKS, VOX).astype(bool)


def sha_rows(a):
    """[n, ...] float32 -> uint8 [n, 32]: sha256 of each row's little-endian float32 bytes."""
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(len(a), -1)).astype("<f4")
    return np.stack([np.frombuffer(hashlib.sha256(r.tobytes()).digest(), np.uint8) for r in a])


def bits_of(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def diagnose(got, want_sha, index, want_bits, what):
    """None when every row of `got` [n, V] has its digest; else the message: which blocks, how many of the sampled
    voxels differ, the largest distance in ulps (probabilities are positive: the distance of the bit patterns)."""
    got = np.asarray(got, np.float32).reshape(len(want_sha), -1)
    bad = np.flatnonzero((sha_rows(got) != want_sha).any(1))
    if not bad.size:
        return None
    d = np.abs(bits_of(got[:, index]).astype(np.int64) - want_bits.astype(np.int64))
    per = ", ".join(f"block {b}: {int((d[b] != 0).sum())} of {index.size} sampled voxels differ, largest ulp distance "
                    f"{int(d[b].max())}" for b in bad)
    return (f"{what}: the float32 bits of blocks {bad.tolist()} are not the committed ones ({per}).  These bits are part "
            f"of the side packs' format: DESIGN.md, 'What the side packs fix'")


# ---------------------------------------------------------------- contexts of the pooled levels from ctx0
def _representatives():
    """float32 [256]: a p of every context, strictly increasing in rank; NaN for a context no float32 in [0, 1] whose
    1 - p is exact can have (above 0.5 a float32 is a multiple of 2^-24, so 1 - p is too)."""
    rep = np.full(256, np.nan, np.float32)
    for ctx in range(256):
        idx, side = ctx >> 1, ctx & 1
        q = np.array([(0x1F8 - idx) << 21], np.uint32).view(np.float32)[0]       # the lower edge of the bucket of 1 - p
        if not side:
            rep[ctx] = q
        elif idx == 127:
            rep[ctx] = 1.0
        elif idx >= 1 and np.float32(1.0 - np.float64(q)) == 1.0 - np.float64(q):
            rep[ctx] = np.float32(1.0 - np.float64(q))
    return rep


REPRESENTATIVE = _representatives()


def rank(ctx):
    ctx = np.asarray(ctx, np.int64)
    return np.where(ctx & 1, 128 + (ctx >> 1), 127 - (ctx >> 1))


def surrogate_p(ctx0):
    """uint8 contexts [..] -> float32 of the same shape: REPRESENTATIVE[ctx]; ValueError for a context without one."""
    p = REPRESENTATIVE[np.asarray(ctx0, np.int64)]
    if np.isnan(p).any():
        raise ValueError("a context no probability of the eval forward can have")
    return p


def write_npz(path, arrays):
    """np.savez_compressed's container with the members in sorted order and a fixed time stamp: numpy stamps every member
    with the wall clock, and two runs of the generator have to give the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# ---------------------------------------------------------------- device half: the builders
def seed_heads(tag):
    """{lod_pack.HEAD_KEYS: float16 numpy} as Net initialises the coarse heads (the trained packs carry none)."""
    from nvfpcc_amd import lod_pack, network
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    from tests.test_trained_golden import CFG
    ch, channels = CFG[tag]
    network.reset_seed(synthetic_seed())
    sd = Net(None, "Gaussian", ch, ",".join(str(c) for c in channels), verbose=False).state_dict()
    return {k: sd[k].detach().numpy().astype(np.float16) for k in lod_pack.HEAD_KEYS}


def build_decoder(golden_dir, tag, dev, heads=None):
    """(net on dev, latents [12, ch, 2, 2, 2] on dev, origins int16 [12, 3]): the decoder of trained_<tag>_pack.pk as
    tests/test_gpu_trained.py builds it, the latents of the pack's own stream; `heads` ({key: float16}) loaded and
    rounded as encode --pack_lod does."""
    import torch
    from nvfpcc_amd import latent_codec, lod_pack, network
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    from tests.test_trained_golden import CFG, load_pack, state_from_pack
    pack, _ = load_pack(golden_dir, tag)
    ch, channels = CFG[tag]
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", ch, ",".join(str(c) for c in channels), verbose=False)
    net.load_state_dict(state_from_pack(pack), strict=False)
    if heads is not None:
        net.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in heads.items()}, strict=False)
    net = net.to(dev)
    if heads is not None:
        lod_pack.round_heads_(net)
    lat = latent_codec.arithmetic_dec(pack["latent_pack"])
    assert lat.shape[0] == N_BLOCKS
    return net, lat.float().to(dev).contiguous(), np.asarray(pack["origins"])


def build_engine(golden_dir, tag, dev):
    """(TrainEngine, latents): the same decoder under the engine.  The engine's eval forward starts at the embeddings,
    so the latent generator is set to the identity (1x1x1 kernel I, no bias, GDN with beta 1 and gamma 0) and the
    embeddings ARE the pack's integer latents: the quantiser hands the decoder exactly them (the caller checks 'x0')."""
    import torch
    from nvfpcc_amd.engine import TrainEngine
    from nvfpcc_amd.synth import make_blocks
    net, lat, _ = build_decoder(golden_dir, tag, torch.device("cpu"))
    lg = net.latent_gen
    ch = lat.shape[1]
    with torch.no_grad():
        lg.h_analysis_2.kernel.copy_(torch.eye(ch).view(ch, ch, 1, 1, 1) - lg.h_analysis_2.kernel_init)
        lg.h_analysis_2.b.copy_(-lg.h_analysis_2.b_init)
        lg.gdn_2.beta.copy_(torch.sqrt(torch.ones(ch) + lg.gdn_2.pedestal_data))
        lg.gdn_2.gamma.zero_()
    gts, dists = make_blocks(N_BLOCKS)
    eng = TrainEngine(net.to(dev), torch.from_numpy(gts).float().to(dev), torch.from_numpy(dists).float().to(dev),
                      n_points_total=float(gts.sum()), lmbda=200.0, w1=10.0, w2=57.0, lr=1e-3, wemb=5.0, emb=lat.to(dev))
    return eng, lat.to(dev)


def batched(f, lat, batch):
    """torch.cat of f(latents[i:i + batch]) over the blocks."""
    import torch
    with torch.no_grad():
        return torch.cat([f(lat[i:i + batch].contiguous()) for i in range(0, lat.shape[0], batch)], 0)


def unpack_levels(gt):
    """bool [12, 32768] -> (gt, its 2^3 max-pool [12, 4096], its 4^3 max-pool [12, 512]) in numpy."""
    g0 = gt.reshape(-1, 32, 32, 32)
    g1 = g0.reshape(-1, 16, 2, 16, 2, 16, 2).any((2, 4, 6))
    g2 = g1.reshape(-1, 8, 2, 8, 2, 8, 2).any((2, 4, 6))
    return gt.reshape(len(gt), -1), g1.reshape(len(gt), -1), g2.reshape(len(gt), -1)


def lod_selection(net, lat, origins, gt_levels, batch):
    """What encode --pack_lod decides (NVFPCC.py, _encode_lod) for heads already rounded: per level 1, 2 the threshold by
    count against the pooled ground truth, the points of reconstruct_points_lod under it as occupancy [12, cells] bool,
    their per-block counts, k and the number of head probabilities equal to the k-th largest (1: no tie)."""
    from nvfpcc_amd import thh_select as ts
    from nvfpcc_amd.recon import reconstruct_points_lod
    out = {"t": [], "occ": [], "counts": [], "k": [], "ties": []}
    for level in (1, 2):
        k = int(gt_levels[level].sum())
        p = batched(lambda x: net.reconstruct_lod(x, level, 2, return_p=True)[1], lat, batch)
        v = ts.kth_largest(p, k)
        t = float(ts.threshold_below(v).item())
        pts, counts = reconstruct_points_lod(net, lat, origins, level, t, batch=batch)
        out["t"].append(t)
        out["occ"].append(occupancy_of_points(pts, counts, origins, level))
        out["counts"].append(np.asarray(counts, np.int32))
        out["k"].append(k)
        out["ties"].append(int((p == v).sum().item()))
    return out


def occupancy_of_points(pts, counts, origins, level):
    """Points of a level in (block, raster) order + per-block counts -> bool [12, cells]; asserts the order."""
    d = 32 >> level
    occ = np.zeros((len(counts), d ** 3), bool)
    blk = np.repeat(np.arange(len(counts)), np.asarray(counts, np.int64))
    rel = np.asarray(pts, np.int64) - (np.asarray(origins, np.int64)[blk] >> level)
    assert rel.shape[0] == blk.size and rel.min(initial=0) >= 0 and rel.max(initial=0) < d
    cell = (rel[:, 0] * d + rel[:, 1]) * d + rel[:, 2]
    key = blk * d ** 3 + cell
    assert (np.diff(key) > 0).all(), "points are not in (block, raster) order"
    occ[blk, cell] = True
    return occ
