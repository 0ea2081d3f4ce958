"""Level-of-detail decode on the GPU: the partial forward (CompDecoder.forward_lod / Net.reconstruct_lod), the two
kernels of csrc/lod_points.hip (nvf_head_occ_bits, nvf_points_from_bits), ops.head_points over them, and the rule
that picks a level's threshold by count.

The references are the paths that exist without the feature: the full forward's coarse heads, the head forward through
nvf_conv3d_gather followed by `p > t`, torch.nonzero, and ops.threshold_points.  Everything is compared exactly except
the oracle comparison, which holds the bound tests/test_gpu_net.py holds for probabilities against the reference
(1e-5 absolute)."""
import numpy as np
import pytest
import torch

from nvfpcc_amd.seeds import synthetic_seed
from tests.golden_inputs import CONFIGS, perturb_state_

pytestmark = pytest.mark.gpu
P_TOL = 1e-5            # tests/test_gpu_net.py: probabilities <= 1e-5 abs against the reference
SHAPES = [(8, 16), (16, 8), (16, 16), (32, 8)]      # (channels, grid) of conv1_cls / conv0_cls, narrow and wide


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


_NETS = {}


def net_for(tag, gpu):
    """The decoder on the golden weights of tests/golden/net_<tag>.npz (seed-derived init + perturb_state_), and the
    oracle's copy of the state."""
    if tag not in _NETS:
        from nvfpcc_amd import network
        from nvfpcc_amd.model import Net
        cfg = CONFIGS[tag]
        network.reset_seed(synthetic_seed())
        net = Net(None, "Gaussian", cfg["ch"], ",".join(str(c) for c in cfg["channels"]), verbose=False)
        sd = net.state_dict()
        perturb_state_(sd, cfg["param_seed"])
        net.load_state_dict(sd)
        P = {k: v.clone() for k, v in net.state_dict().items()}
        _NETS[tag] = (net.to(gpu), P)
    return _NETS[tag]


def latents_for(tag, B, seed=7):
    g = torch.Generator().manual_seed(seed + B)
    return torch.round(2.0 * torch.randn(B, CONFIGS[tag]["ch"], 2, 2, 2, generator=g))


def unpack(words, voxels):
    """int64 words [B, W] -> bool [B, 64 W]: bit k of word w first."""
    k = torch.arange(64, device=words.device, dtype=torch.int64)
    bits = (words.unsqueeze(-1) >> k) & 1
    return bits.reshape(words.shape[0], -1)[:, :voxels].bool()


def pack(bits):
    """bool [B, V] (V a multiple of 64) -> int64 words [B, V / 64]; bit 63 wraps into the sign."""
    k = torch.arange(64, device=bits.device, dtype=torch.int64)
    return (bits.reshape(bits.shape[0], -1, 64).long() << k).sum(-1)


# ---------------------------------------------------------------- 1. partial forward
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("tag", ["S", "W"])
def test_partial_forward_equals_the_full_forwards_coarse_heads(tag, B, gpu):
    from oracle import nvf_oracle as O
    net, P = net_for(tag, gpu)
    c = CONFIGS[tag]["channels"]
    lat = latents_for(tag, B)
    with torch.no_grad():
        full = net.reconstructor(lat.to(gpu), 2)[1]
        _, ref_cls, _ = O.decoder(P, lat, 2)
    for lod in (1, 2):
        x, p = net.reconstructor.forward_lod(lat.to(gpu), 2, lod, return_p=True)
        d = 32 >> lod
        assert x.shape == (B, c[2] if lod == 1 else c[1], d, d, d) and p.shape == (B, 1, d, d, d)
        assert torch.equal(p, full[2 - lod]), f"lod {lod}: not the bits of forward(x, 2)[1][{2 - lod}]"
        assert torch.equal(net.reconstruct_lod(lat.to(gpu), lod), x)
        assert torch.equal(net.reconstructor.forward_lod(lat.to(gpu), 2, lod), x)
        err = (p.cpu() - ref_cls[2 - lod]).abs().max().item()
        print(f"[{tag} B={B} lod={lod}] max |p - oracle| = {err:.2e} (bound {P_TOL:.0e})")
        assert err < P_TOL
    with pytest.raises(ValueError):
        net.reconstructor.forward_lod(lat.to(gpu), 2, 3)
    with pytest.raises(ValueError):
        net.reconstructor.forward_lod(lat.to(gpu), 1, 1)


@pytest.mark.parametrize("ch,chanstr", [(3, "8,16,8,8"), (8, "16,32,16,16"), (4, "4,8,4,4")])
def test_reconstruct_is_the_full_forwards_output_without_heads_or_rate(ch, chanstr, gpu, monkeypatch):
    """Net.reconstruct gives the bits of forward(x, 2)[0] and runs neither coarse head nor the weight rate.  Two blocks:
    the smallest batch at which a per-block indexing slip in the trunk walk can show."""
    from nvfpcc_amd import network
    from nvfpcc_amd.model import Net
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", ch, chanstr, verbose=False)
    sd = net.state_dict()
    perturb_state_(sd, 500 + ch)
    net.load_state_dict(sd)
    net = net.to(gpu)
    lat = torch.round(2.0 * torch.randn(2, ch, 2, 2, 2, generator=torch.Generator().manual_seed(ch))).to(gpu)
    with torch.no_grad():
        full = net.reconstructor(lat, 2)[0]
        assert full.shape == (2, 1, 32, 32, 32)
        assert torch.equal(net.reconstruct(lat, 2), full)

        def unused(*a, **k):
            raise AssertionError("a coarse head or the weight rate ran")
        r = net.reconstructor
        for mod in (r.conv0_cls, r.conv1_cls, r.likelihood_model):
            monkeypatch.setattr(mod, "forward", unused)
        assert torch.equal(net.reconstruct(lat, 2), full)
        with pytest.raises(AssertionError, match="a coarse head"):
            net.reconstructor(lat, 2)


# ---------------------------------------------------------------- 2. nvf_head_occ_bits
def head_case(C, D, B, gpu):
    """Activations with a few exact zeros and large magnitudes (a wrong halo or padding tap changes a logit by far more
    than a rounding), a 3^3 head, and its probabilities through the existing head forward."""
    from nvfpcc_amd import ops
    g = torch.Generator().manual_seed(1000 * C + 10 * D + B)
    x = torch.randn(B, C, D, D, D, generator=g)
    u = torch.rand(x.shape, generator=g)
    x[u < 0.02] = 0.0
    x[u > 0.98] *= 40.0
    x[:, :, 0, 0, 0] = 25.0                      # corners and edges of the grid: where the padding taps are
    x[:, :, -1, -1, -1] = -25.0
    x[:, :, 0, -1, :] *= 8.0
    w = 0.08 * torch.randn(1, C, 3, 3, 3, generator=g)
    bias = torch.tensor([0.1])
    x, w, bias = x.to(gpu), w.to(gpu), bias.to(gpu)
    wf = ops.pack_conv_weight(w.contiguous(), want_bwd=False)[0]
    p = ops.conv3d_gather(x, wf, bias, 1, 3, 1, 1, (D, D, D), ops.ACT_SIGMOID)
    return x, wf, bias, p


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("C,D", SHAPES)
def test_head_occ_bits_equals_head_forward_then_threshold(C, D, B, gpu):
    from nvfpcc_amd import ops
    x, wf, bias, p = head_case(C, D, B, gpu)
    V = D ** 3
    rows = p.reshape(B, V)
    assert 0.02 < float((rows > 0.5).float().mean()) < 0.98        # the case decides something
    srt = rows.sort(dim=1).values
    g = torch.Generator().manual_seed(B)
    cases = {
        "scalar": 0.5,
        "per block": (0.2 + 0.6 * torch.rand(B, generator=g)).to(gpu),
        "per block = the block's maximum": srt[:, -1].contiguous(),
        "per block = a middle value of the block": srt[:, V // 2].contiguous(),
        "scalar = a probability that occurs": float(rows[B // 2, V // 3].item()),
        "t = 1.0": 1.0,
        "t < 0": -0.25,
    }
    for what, t in cases.items():
        words, counts = ops.head_occ_bits(x, wf, bias, t)
        assert words.shape == (B, V // 64) and words.dtype == torch.int64 and counts.dtype == torch.int32
        tt = t.reshape(B, 1) if isinstance(t, torch.Tensor) else t
        ref = rows > tt
        got = unpack(words, V)
        assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} voxels differ"
        assert torch.equal(counts.long(), ref.sum(1)), what
        assert torch.equal(counts.long(), got.sum(1)), what
    assert int(ops.head_occ_bits(x, wf, bias, 1.0)[1].sum()) == 0
    assert int(ops.head_occ_bits(x, wf, bias, -0.25)[1].sum()) == B * V
    # ties: the middle value is kept out by `>`, and the voxels that equal it are not in the set
    mid = srt[:, V // 2]
    words, counts = ops.head_occ_bits(x, wf, bias, mid.contiguous())
    assert torch.equal(counts.long(), (rows > mid[:, None]).sum(1)) and bool((counts.long() <= V - V // 2 - 1).all())


def test_head_occ_bits_refuses_other_shapes(gpu):
    from nvfpcc_amd import ops
    x = torch.zeros(1, 4, 16, 16, 16, device=gpu)
    with pytest.raises(RuntimeError, match="no kernel"):
        ops.head_occ_bits(x, torch.zeros(4 * 27, device=gpu), None, 0.5)
    with pytest.raises(RuntimeError, match="shape"):
        ops.head_occ_bits(torch.zeros(2, 8, 16, 16, 16, device=gpu), torch.zeros(8 * 27, device=gpu), None,
                          torch.zeros(3, device=gpu))


# ---------------------------------------------------------------- 3. nvf_points_from_bits
def bit_blocks(kinds, D, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for kind in kinds:
        if kind == "empty":
            rows.append(torch.zeros(D ** 3, dtype=torch.bool))
        elif kind == "full":
            rows.append(torch.ones(D ** 3, dtype=torch.bool))
        else:
            rows.append(torch.rand(D ** 3, generator=g) < float(kind))
    return torch.stack(rows).to(gpu)


@pytest.mark.parametrize("D,shift", [(16, 1), (8, 2), (16, 2), (8, 0)])
@pytest.mark.parametrize("kinds", [("empty", 0.3, "empty", "full", 0.05, 0.9, "empty"), (0.4,), ("empty",), ("full",)],
                         ids=["mixed7", "one", "one-empty", "one-full"])
def test_points_from_bits_equals_nonzero(kinds, D, shift, gpu):
    from nvfpcc_amd import ops
    B = len(kinds)
    bits = bit_blocks(kinds, D, gpu, seed=D + shift)
    words = pack(bits)
    assert torch.equal(unpack(words, D ** 3), bits)
    counts = bits.sum(1).to(torch.int32)
    # origins up to 12 bits: the last cube of a 4096^3 volume, odd coordinates (the shift must floor), and zero
    org = torch.tensor([[4064, 4064, 4064], [4095, 4094, 4093], [0, 32, 4064], [2048, 0, 31], [1, 2, 3],
                        [4064, 0, 0], [33, 4095, 2047]], dtype=torch.int32)[:B].to(gpu)
    pts = ops.points_from_bits(words, counts, org, D, shift)
    nz = torch.nonzero(bits.reshape(B, D, D, D))
    ref = (org.long()[nz[:, 0]] >> shift) + nz[:, 1:]
    assert pts.dtype == torch.int32 and pts.shape == (int(counts.sum()), 3)
    assert torch.equal(pts.long(), ref), "order or values differ from torch.nonzero"
    if pts.shape[0]:
        assert int(pts.max()) <= (4095 >> shift) + D - 1
    none = ops.points_from_bits(words, counts, None, D, shift)
    assert torch.equal(none.long(), nz[:, 1:])


# ---------------------------------------------------------------- 4. ops.head_points
@pytest.mark.parametrize("C,D", SHAPES + [(4, 16)])         # (4, 16): no fused kernel, the head forward + threshold_points
def test_head_points_equals_threshold_points(C, D, gpu):
    from nvfpcc_amd import ops
    B, lod = 6, (1 if D == 16 else 2)
    x, wf, bias, p = head_case(C, D, B, gpu)
    org = (torch.tensor([[4064, 4064, 4064], [0, 0, 0], [32, 2048, 4064], [1024, 992, 64], [4064, 0, 32], [96, 96, 96]],
                        dtype=torch.int32)).to(gpu)
    srt = p.reshape(B, -1).sort(dim=1).values
    for t in (0.5, srt[:, D ** 3 // 2].contiguous(), 1.0, -1.0):
        pts, counts = ops.head_points(x, wf, bias, t, org, lod)
        ref_pts, ref_counts = ops.threshold_points(p, t, org >> lod)
        assert torch.equal(counts, ref_counts) and pts.dtype == ref_pts.dtype
        assert torch.equal(pts, ref_pts)
    with pytest.raises(RuntimeError):
        ops.head_points(x, wf, bias, 0.5, org, 3 - lod)        # the other level reads another grid


# ---------------------------------------------------------------- 5. the count rule
@pytest.mark.parametrize("lod", [1, 2])
def test_count_threshold_keeps_at_least_k_and_exactly_k_without_a_tie(lod, gpu):
    from nvfpcc_amd import ops
    from nvfpcc_amd.synth import make_blocks
    from nvfpcc_amd.thh_select import threshold_for_count, kth_largest
    net, _ = net_for("S", gpu)
    B = 6
    gt = torch.from_numpy(make_blocks(B)[0]).float().to(gpu)
    g = gt
    for _ in range(lod):
        g = ops.maxpool2(g.contiguous())
    k = int((g != 0).sum().item())
    assert 0 < k < g.numel()
    x, p = net.reconstruct_lod(latents_for("S", B).to(gpu), lod, return_p=True)
    t = float(threshold_for_count(p, k).item())
    v_k = float(kth_largest(p, k).item())
    kept = int((p > t).sum().item())
    ties = int((p == v_k).sum().item())
    print(f"[lod {lod}] k = {k}, kept = {kept}, voxels equal to v_k: {ties}")
    assert kept >= k and ties >= 1
    assert kept == int((p > v_k).sum().item()) + ties
    if ties == 1:
        assert kept == k
    wf, bias = net.lod_head_params(lod)
    pts, counts = ops.head_points(x, wf, bias, t, None, lod)
    assert int(counts.sum()) == kept and pts.shape[0] == kept
