"""Latents fitted under a frozen decoder (TrainEngine.fit_latents, block_costs, the main-head-only latent pass) on the two
committed trained decoders and their 12 blocks (tests/conformance_ref.build_engine: the decoder of trained_<tag>_pack.pk
under the engine, the latent generator set to the identity).

The gradient's reference is the oracle (oracle/nvf_oracle.py) in float64 on the CPU with the pass's own ReLU masks
imposed, differentiating the SAME objective -- the main output's focal term plus lambda w1 / n_pts times the latent bits;
the bound is the project's rule, max(8e-6, 3 x the float32 CPU oracle's own distance from float64) of max |de|, and the
masks are held to the float64 pre-activations as tests/test_gpu_measured_path.py holds them."""
import argparse

import numpy as np
import pytest
import torch

from tests import conformance_ref as C
from tests.philox_np import latent_noise
from tests.test_gpu_measured_path import GRAD_TOL, H, MASK_FLIP_MAX_ACTIVATION, MASK_FLIP_MAX_FRACTION, RELU_LAYERS

pytestmark = pytest.mark.gpu
N = C.N_BLOCKS
HEAD_KEYS = ("reconstructor.conv0_cls.kernel", "reconstructor.conv0_cls.b", "reconstructor.conv1_cls.kernel",
             "reconstructor.conv1_cls.b")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return torch.device("cuda")


def engine(golden_dir, tag, gpu):
    eng, _ = C.build_engine(golden_dir, tag, gpu)
    assert (eng.lmbda, eng.w1) == (H["lmbda"], H["w1"]) and (eng.narrow if tag == "S" else eng.wide)
    return eng


def main_only_pass(eng, lo, hi):
    """One main-head-only latent pass of blocks [lo, hi) at the engine's noise counter, as fit_latents runs it."""
    eng.prepare_weights(2)
    a, de = eng._latent_grad(lo, hi, main_only=True)
    torch.cuda.synchronize()
    return a, de


def oracle_main(P, emb, gt, dist, ids, n_pts, noise_step, masks, dtype, keep=None):
    """d/d emb[ids] of  focal(main output) + lambda w1 / n_pts * latent bits  by the oracle in ``dtype``, the engine's
    own noise draws and ReLU masks imposed."""
    from oracle import nvf_oracle as O
    P = {k: v.to(dtype) if v.is_floating_point() else v for k, v in P.items()}
    e = emb[ids].to(dtype).clone().requires_grad_(True)
    u = torch.from_numpy(latent_noise(0, noise_step, ids, emb.shape[1])).to(dtype)
    out, _, _, lbits = O.net_forward(P, e, "train", 2, u, None, keep=keep, relu_masks=masks)
    loss = O.surf_focal_dense(out, gt[ids].to(dtype), dist[ids].to(dtype), beta=1, alpha=0.9) \
        + H["lmbda"] * H["w1"] * lbits.sum() / n_pts
    loss.backward()
    return e.grad.detach()


@pytest.mark.parametrize("lo,hi", [(0, N), (3, 4)])
@pytest.mark.parametrize("tag", C.TAGS)
def test_main_head_only_gradient_against_the_float64_oracle(tag, lo, hi, gpu, golden_dir):
    eng = engine(golden_dir, tag, gpu)
    eng.noise_step = 7
    a, de = main_only_pass(eng, lo, hi)
    assert a["p0"] is None and a["p1"] is None, "the coarse heads did not run"
    assert eng.last["loss_terms"][1:3].tolist() == [0.0, 0.0]
    P = {k: v.detach().cpu().clone() for k, v in eng.net.state_dict().items()}
    emb, gt, dist = eng.emb.cpu(), eng.gt.cpu(), eng.dist.cpu()
    ids, n_pts = np.arange(lo, hi), float(eng.counts.sum())
    masks = {n: (a[k] > 0).cpu() for n, k in RELU_LAYERS.items()}
    keep = {}
    de64 = oracle_main(P, emb, gt, dist, ids, n_pts, eng.noise_step, masks, torch.float64, keep)
    for n, k in RELU_LAYERS.items():        # the masks differ from the float64 pre-activations only at zero to rounding
        pre = keep[n + ".pre"].detach()
        flip = (pre > 0) != masks[n]
        if flip.any():
            assert int(flip.sum()) <= max(1, MASK_FLIP_MAX_FRACTION * flip.numel()), (tag, n, int(flip.sum()))
            w = float(torch.maximum(pre.abs(), a[k].cpu().double().abs())[flip].max()) / float(pre.abs().max())
            assert w <= MASK_FLIP_MAX_ACTIVATION, (tag, n, w)
    de32 = oracle_main(P, emb, gt, dist, ids, n_pts, eng.noise_step, masks, torch.float32)
    scale = float(de64.abs().max())
    assert scale > 0
    err = float((de.cpu().double() - de64).abs().max()) / scale
    d32 = float((de32.double() - de64).abs().max()) / scale
    bound = max(GRAD_TOL, 3 * d32)
    print(f"[main-head-only latent gradient {tag} blocks {lo}..{hi - 1}] device {err:.2e} | float32 oracle {d32:.2e} | "
          f"bound {bound:.2e} | max |de| {scale:.3e}")
    assert bool(torch.isfinite(de).all()) and err < bound, (tag, err, d32, bound)


@pytest.mark.parametrize("tag", C.TAGS)
def test_gradient_does_not_depend_on_the_coarse_heads(tag, gpu, golden_dir):
    """A decoder rebuilt from a pack holds seed values in conv0_cls / conv1_cls: they must not push on the latents."""
    eng = engine(golden_dir, tag, gpu)
    eng.noise_step = 3
    _, de = main_only_pass(eng, 0, N)
    eng.prepare_weights(2)
    _, de_all = eng._latent_grad(0, N)
    g = torch.Generator().manual_seed(5)
    for k in HEAD_KEYS:
        off, n = eng.slices[k]
        eng.flat_p[off:off + n] += 0.05 * torch.randn(n, generator=g).to(gpu)
    _, de2 = main_only_pass(eng, 0, N)
    eng.prepare_weights(2)
    _, de_all2 = eng._latent_grad(0, N)
    torch.cuda.synchronize()
    assert torch.equal(de, de2)
    assert not torch.equal(de_all, de_all2), "the three-head pass does see the coarse heads"


@pytest.mark.parametrize("tag", C.TAGS)
def test_blocks_are_independent(tag, gpu, golden_dir):
    """Perturbing the emb rows of all blocks but b leaves row b of de, and J_b, bit-equal."""
    eng = engine(golden_dir, tag, gpu)
    eng.noise_step = 11
    _, de = main_only_pass(eng, 0, N)
    J = eng.block_costs()
    emb0 = eng.emb.clone()
    g = torch.Generator().manual_seed(6)
    for b in (0, 5, N - 1):
        eng.emb.copy_(emb0 + torch.randint(-2, 3, emb0.shape, generator=g).float().to(gpu)
                      + 0.3 * torch.rand(emb0.shape, generator=g).to(gpu))
        eng.emb[b] = emb0[b]
        _, de_b = main_only_pass(eng, 0, N)
        J_b = eng.block_costs()
        assert torch.equal(de_b[b], de[b]), (tag, b)
        assert torch.equal(J_b[b], J[b]), (tag, b)
        others = [i for i in range(N) if i != b]
        assert not torch.equal(J_b[others], J[others]), "the perturbation reached the other blocks"
    eng.emb.copy_(emb0)
    # ... and J is c_f * focal + c_r * bits of nvf_block_costs with the coefficients of the gradient's objective
    sums = eng._block_sums(0, N)
    c_r = eng.lmbda * eng.w1 / float(eng.counts.sum())
    assert J.dtype == torch.float64 and torch.equal(J, 1.0 * sums[:, 0] + c_r * sums[:, 1])


STEPS, EVERY = 40, 5


@pytest.mark.parametrize("tag", C.TAGS)
def test_fit_from_a_table_of_ones(tag, gpu, golden_dir):
    """fit_latents(40, eval_every=5) from emb = 1 with lr_emb = 0.05 (the latent generator of the fixture engine is the
    identity, so a rounded latent changes once Adam has moved its row by 0.5: ten steps at this rate).

    Measured on one MI355X, sum of J_b over the 12 blocks, start -> final, every block improved:
    S 1.925516592e+05 -> 1.835725107e+04, W 9.427525916e+04 -> 5.510682633e+03."""
    eng = engine(golden_dir, tag, gpu)
    eng.emb.fill_(1.0)
    eng.lr_emb = 0.05
    before = (eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone(), eng.opt_step, eng.noise_step)
    seen = []
    J0, J1 = eng.fit_latents(STEPS, eval_every=EVERY, report=lambda s, J, imp, bits: seen.append((s, float(J.sum()), int(imp.sum()))))
    torch.cuda.synchronize()
    print(f"[fit_latents {tag}] sum J: start {float(J0.sum()):.9e} -> final {float(J1.sum()):.9e}; improved blocks "
          f"{int((J1 < J0).sum())} of {N}; evaluations {[s for s, _, _ in seen]}")
    assert [s for s, _, _ in seen] == list(range(0, STEPS + 1, EVERY))
    assert J0.dtype == torch.float64 and J1.dtype == torch.float64 and tuple(J0.shape) == (N,)
    assert bool((J1 <= J0).all()), "no block ends worse than it started"
    assert float(J1.sum()) < float(J0.sum()), "the summed cost fell"
    sums = [j for _, j, _ in seen]
    assert all(b <= a for a, b in zip(sums, sums[1:])), sums
    assert torch.equal(eng.block_costs(), J1), "the kept rows ARE the table"
    assert torch.equal(eng.flat_p, before[0]) and torch.equal(eng.flat_m, before[1]) and torch.equal(eng.flat_v, before[2])
    assert eng.opt_step == before[3] and eng.noise_step == before[4] + STEPS and eng.emb_step == STEPS


@pytest.mark.parametrize("tag", C.TAGS)
def test_effective_weights_are_those_of_the_decoder_the_pack_rebuilds(tag, gpu, golden_dir):
    """After the fit's prepare_weights(2) every layer's effective weights are, bit for bit, those of a decoder that
    NVFPCC._decoder_from_pack builds from the fixture pack's bytes."""
    import NVFPCC
    from nvfpcc_amd import network
    from nvfpcc_amd.engine import TRUNK, TrainEngine
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    from tests.test_trained_golden import CFG, load_pack
    eng = engine(golden_dir, tag, gpu)
    eng.fit_latents(1, eval_every=1)
    pack, _ = load_pack(golden_dir, tag)
    ch, channels = CFG[tag]
    network.reset_seed(synthetic_seed())
    fresh = Net(None, "Gaussian", ch, ",".join(str(c) for c in channels), verbose=False)
    net2, lat2 = NVFPCC._decoder_from_pack(argparse.Namespace(qp=16.0), pack, gpu, net=fresh)
    eng2 = TrainEngine(net2, eng.gt, eng.dist, n_points_total=eng.n_points_total, emb=lat2.float(), **H)
    eng2.prepare_weights(2)
    torch.cuda.synchronize()
    for name in TRUNK:
        a, b = eng.layers[name], eng2.layers[name]
        assert torch.equal(a.w_fwd, b.w_fwd) and torch.equal(a.w_bwd, b.w_bwd) and torch.equal(a.b_eff, b.b_eff), (tag, name)
        assert all(torch.equal(a.wp[p], b.wp[p]) for p in a.wp), (tag, name)
