"""The training step against the float64 oracle at a TRAINED state.

Every other gradient-parity test runs at seed-initialised parameters with a small perturbation: probabilities near 0.5,
logits O(1), half of every ReLU mask on, the GDN and rate parameters at their initial values.  Here each decoder of
BASELINE.json is first trained by the engine itself on the schedule of tools/make_trained_fixture.py (201 epochs over
the 12 synthetic blocks, batch 4, q = 1 up to epoch 79 and q = 2 from epoch 80, one latent step per epoch) -- the state
at which a codec's rate-distortion numbers are decided: a third or more of the output probabilities under the focal
loss's 1e-9 clamp, logits of -20 .. -100, sparse and tiny dy, trained beta / gamma / sigma / mu.  The oracle is then
evaluated at the ENGINE's state (parameters from flat_p, latents from eng.emb), so nothing depends on training being
reproduced bit for bit.

Bounds.  Loss 2e-5 relative and probabilities 1e-5 absolute against the float32 oracle, and the ReLU-mask assertions of
_oracle64_with_masks, as in tests/test_gpu_measured_path.py.  The gradient bound is taken from the reference at run time:
with d32[name] = max |g32 - g64| / max |g64| the distance of the float32 CPU oracle (same masks imposed) from the float64
one, every slice of the engine must satisfy

    err < max(GRAD_TOL_BY_SLICE.get(name, GRAD_TOL), 3 * d32[name])

-- the floor is the bound held at initialisation, 3 the margin the project gives another fixed summation order
(profiles/r05_relu_mask_parity.md).  It never comes from the engine's own numbers.  Measured: profiles/trained_state_parity.md."""
import time

import numpy as np
import pytest
import torch

from tests.test_gpu_measured_path import (GRAD_TOL, GRAD_TOL_BY_SLICE, H, NPTS, RELU_LAYERS, _layer_ids, _oracle64_with_masks,
                                          _oracle_step, make)

pytestmark = pytest.mark.gpu
CONFIGS = {"S": (3, (8, 16, 8, 8), 5.0), "W": (8, (16, 32, 16, 16), 8.0)}       # ch, channels, --wemb of the fixture tool
N_BLOCKS, EPOCHS, PHASE, BATCH, LR = 12, 201, 80, 4, 1e-3                       # tools/make_trained_fixture.py
# floors of the regime: a third and a half of what the committed goldens of the narrow decoder show on the same data
# and schedule (trained_S.npz / trained_W.npz: 0.30 / 0.53 below 1e-9, 0.42 / 0.64 below 1e-6)
MIN_SHARE_BELOW_1E9, MIN_SHARE_BELOW_1E6 = 0.10, 0.20


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return torch.device("cuda")


class Trained:
    pass


@pytest.fixture(scope="module", params=["S", "W"])
def trained(request, gpu):
    """One decoder trained by the engine; the oracle's state rebuilt from the engine's."""
    from NVFPCC import lr_at_epoch
    from oracle import nvf_oracle as O
    dec = request.param
    ch, chans, wemb = CONFIGS[dec]
    net, eng, P, gt, dist, emb = make(gpu, ch, chans, N_BLOCKS)
    assert eng.winograd and (eng.narrow if dec == "S" else eng.wide)
    eng.lr_emb = LR * wemb
    torch.cuda.synchronize()
    t0 = time.time()
    for epoch in range(EPOCHS):
        q = 1 if epoch < PHASE else 2
        eng.lr = lr_at_epoch(LR, epoch)
        order = torch.randperm(N_BLOCKS, generator=torch.Generator().manual_seed(1000003 + epoch)).numpy()
        for s in range(0, N_BLOCKS, BATCH):
            eng.train_step(order[s:s + BATCH], q)
        eng.latent_step(q)
    torch.cuda.synchronize()
    wall = time.time() - t0
    assert eng.opt_step == EPOCHS * (N_BLOCKS // BATCH) and eng.emb_step == EPOCHS
    assert bool(torch.isfinite(eng.flat_p).all()) and bool(torch.isfinite(eng.emb).all())
    # the oracle's state from the engine's: every trainable key, and the latent table
    keys = O.trainable_keys(P)
    refreshed = set()
    for name, (off, n) in eng.slices.items():
        new = eng.flat_p[off:off + n].cpu().view(P[name].shape).clone()
        assert not torch.equal(new, P[name]), f"{name} is still at its initial value"
        P[name] = new
        refreshed.add(name)
    assert refreshed == set(keys), refreshed ^ set(keys)
    emb_t = eng.emb.cpu().clone()
    assert emb_t.shape == emb.shape and bool(((emb_t - emb).flatten(1).abs().amax(1) > 0).all())
    # the regime: these tests must not quietly run on an untrained state
    ev = eng.eval_forward(q=2)
    p = ev["p2"].cpu()
    s9, s6, zeros = float((p < 1e-9).float().mean()), float((p < 1e-6).float().mean()), int((p == 0).sum())
    on = {n: float((ev[k] > 0).float().mean()) for n, k in RELU_LAYERS.items()}
    T = Trained()
    T.dec, T.net, T.eng, T.P, T.gt, T.dist, T.emb, T.ch, T.chans = dec, net, eng, P, gt, dist, emb_t, ch, chans
    tpr, tnr = float((p[gt != 0] > 0.5).float().mean()), float((p[gt == 0] <= 0.5).float().mean())
    T.regime = (f"[trained state {dec}] fixture {wall:.1f} s; p < 1e-9: {s9:.3f}, p < 1e-6: {s6:.3f}, p == 0: {zeros} of "
                f"{p.numel()}; occupied voxels with p > 0.5: {tpr:.3f}, empty ones with p <= 0.5: {tnr:.4f}; ReLU on-share "
                + ", ".join(f"{n} {v:.3f}" for n, v in on.items()))
    print(T.regime)
    assert s9 >= MIN_SHARE_BELOW_1E9 and s6 >= MIN_SHARE_BELOW_1E6, (s9, s6)
    return T


def _check(T, eng, net, engine, case, step, ids, q):
    """One pass of `eng` (`step`: "train" = train_step, "latent" = the full-batch latent pass) at the trained state."""
    P, gt, dist, emb = T.P, T.gt, T.dist, T.emb
    ids = np.asarray(ids, np.int64)
    lids = _layer_ids(net)
    tag = f"trained/{T.dec}/{engine}/{case}"
    if step == "train":
        n_pts = float(eng.counts[ids].sum())
        a, de = eng.train_step(ids, q, update=False), None
    else:
        n_pts = float(eng.counts.sum())
        a, de = eng.latent_step(q, update=False)
    loss_ref, out_ref, cls_ref, _, _ = _oracle_step(P, emb, gt, dist, ids, q, n_pts, eng.noise_step, layer_ids=lids)
    assert float((a["p2"].cpu() - out_ref).abs().max()) < 1e-5
    assert float((a["p0"].cpu() - cls_ref[0]).abs().max()) < 1e-5 and float((a["p1"].cpu() - cls_ref[1]).abs().max()) < 1e-5
    assert abs(eng.loss_value() - loss_ref) < 2e-5 * abs(loss_ref), (tag, eng.loss_value(), loss_ref)
    g64, de64 = _oracle64_with_masks(eng, net, P, gt, dist, emb, ids, q, n_pts, a, tag)
    # the reference's own float32 arithmetic under the same masks: its distance from float64 sets the bound
    masks = {n: (a[k] > 0).cpu() for n, k in RELU_LAYERS.items()}
    _, _, _, g32, de32 = _oracle_step(P, emb, gt, dist, ids, q, n_pts, eng.noise_step, layer_ids=lids, relu_masks=masks)
    if step == "train":
        got = {name: eng.flat_g[off:off + n].cpu().numpy().astype(np.float64) for name, (off, n) in eng.slices.items()}
        ref32, ref64 = g32, g64
    else:
        got, ref32, ref64 = {"latent": de.cpu().numpy().astype(np.float64).reshape(-1)}, {"latent": de32}, {"latent": de64}
    rows = []
    for name, mine in got.items():
        r = ref64[name].numpy().reshape(-1)
        scale = max(np.abs(r).max(), 1e-30)
        err = np.abs(mine - r).max() / scale
        d32 = np.abs(ref32[name].numpy().reshape(-1).astype(np.float64) - r).max() / scale
        floor = GRAD_TOL_BY_SLICE.get(name, GRAD_TOL)
        rows.append((err / max(floor, 3 * d32), name, err, d32, max(floor, 3 * d32)))
    _, name, err, d32, bound = max(rows)
    print(f"[trained-state parity] | {T.dec} | {engine} | {case} | {name} | {err:.2e} | {d32:.2e} | {bound:.2e} |")
    for _, name, err, d32, bound in rows:
        assert err < bound, (tag, name, err, d32, bound)


MINI = np.random.default_rng(5).permutation(N_BLOCKS)[:BATCH]


@pytest.mark.parametrize("q", [2, 1])
def test_minibatch_step_matches_the_oracle_at_a_trained_state(trained, q):
    """train_step(update=False) of the default engine (Winograd forms of the 4^3 layers included) on one mini-batch of 4;
    q = 1 feeds the oracle the engine's own weight-noise draws."""
    _check(trained, trained.eng, trained.net, "default", f"train_step, 4 blocks, q={q}", "train", MINI, q)


def test_twelve_block_step_matches_the_oracle_at_a_trained_state(trained):
    """All 12 blocks in one step: three times the slabs per gradient, other workgroup counts."""
    _check(trained, trained.eng, trained.net, "default", "train_step, 12 blocks, q=2", "train", np.arange(N_BLOCKS), 2)


def test_latent_pass_matches_the_oracle_at_a_trained_state(trained):
    """The full-batch latent pass: the latent gradient through the trained stem (GDN at trained beta / gamma, the rate
    term at trained sigma / mu)."""
    _check(trained, trained.eng, trained.net, "default", "latent_step, 12 blocks, q=2", "latent", np.arange(N_BLOCKS), 2)


def test_direct_engine_matches_the_oracle_at_a_trained_state(trained, gpu):
    """A second engine with winograd=False on the same parameters and latents: the direct fixed-order kernels."""
    from nvfpcc_amd import network
    from nvfpcc_amd.engine import TrainEngine
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    T = trained
    network.reset_seed(synthetic_seed())
    network.set_noise_seed(0, 0)
    net2 = Net(None, "Gaussian", T.ch, ",".join(str(c) for c in T.chans), verbose=False)
    net2.load_state_dict({k: v.detach().cpu().clone() for k, v in T.net.state_dict().items()})
    net2 = net2.to(gpu)
    eng2 = TrainEngine(net2, T.gt.to(gpu), T.dist.to(gpu), n_points_total=NPTS, emb=T.eng.emb, seed=0, winograd=False, **H)
    assert not eng2.winograd and not any(p.startswith("wino") for p in eng2.layers["conv2"].wp)
    assert torch.equal(eng2.flat_p, T.eng.flat_p) and torch.equal(eng2.emb, T.eng.emb)
    _check(T, eng2, net2, "direct", "train_step, 4 blocks, q=2", "train", MINI, 2)
