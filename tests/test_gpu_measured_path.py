"""Parity on the path the bench line is measured on: the 16- and 4-step UNROLLED graphs fed by a
device-resident schedule at batch 16 over 917 resident blocks; one batch-16 step directly against the CPU oracle (q = 2
and q = 1 with the engine's own counter-RNG draws fed to the oracle); and decoder configurations other than the two of
BASELINE.json (the reference's argparse default `--ch 8 --chanstr 8,16,8,8`, NVFPCC.py:723-735, and an off-grid string)."""
import numpy as np
import pytest
import torch

from nvfpcc_amd.seeds import synthetic_seed
from nvfpcc_amd.synth import make_blocks
from tests.golden_inputs import perturb_state_, make_emb
from tests.philox_np import latent_noise, weight_noise

pytestmark = pytest.mark.gpu
H = dict(lmbda=200.0, w1=10.0, w2=57.0, lr=1e-3, wemb=5.0)
NPTS = 917 * 936.0
TRUNK = ("up0", "conv0", "up1", "conv1", "up2", "conv2", "conv2_cls")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


def make(gpu, ch, channels, nblk, distinct=None, param_seed=101, emb_seed=202):
    from nvfpcc_amd import network
    from nvfpcc_amd.engine import TrainEngine
    from nvfpcc_amd.model import Net
    network.reset_seed(synthetic_seed())
    network.set_noise_seed(0, 0)
    net = Net(None, "Gaussian", ch, ",".join(str(c) for c in channels), verbose=False)
    sd = net.state_dict()
    perturb_state_(sd, param_seed)
    net.load_state_dict(sd)
    P = {k: v.clone() for k, v in net.state_dict().items()}          # the oracle's copy (CPU)
    net = net.to(gpu)
    distinct = nblk if distinct is None else min(distinct, nblk)
    gts, dists = make_blocks(distinct)
    reps = (nblk + distinct - 1) // distinct
    gt = torch.from_numpy(np.tile(gts, (reps, 1, 1, 1, 1))[:nblk]).float()
    dist = torch.from_numpy(np.tile(dists, (reps, 1, 1, 1, 1))[:nblk]).float()
    emb = make_emb(nblk, ch, emb_seed)
    eng = TrainEngine(net, gt.to(gpu), dist.to(gpu), n_points_total=NPTS, emb=emb.to(gpu), seed=0, **H)
    return net, eng, P, gt, dist, emb


def test_unrolled_schedule_replay_equals_host_steps(gpu):
    """bench.py and NVFPCC.py train drive GraphedTrainStep.load_schedule((ids, n_pts)) + replay_all(): 20 steps = one
    16-step graph + one 4-step graph, the last-arriving workgroup of every step's final launch handing the step buffer
    over to the next schedule row INSIDE the graph.  Against 20 host-launched train_steps from the same state: parameters,
    both Adam moments, the latent table and the epoch accumulators bit for bit (q = 1: weight and latent noise on)."""
    from nvfpcc_amd.engine import GraphedTrainStep
    net, eng, P, gt, dist, emb = make(gpu, 3, (8, 16, 8, 8), 917, distinct=24)
    eng.enable_epoch_stats()
    B, K = 16, 20
    order = np.random.default_rng(11).permutation(917)[:K * B].reshape(K, B).astype(np.int64)
    npts = eng.counts[order].sum(axis=1).astype(np.float64)
    snap = lambda: (eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone(), eng.noise_step, eng.opt_step)

    def restore(s):
        eng.flat_p.copy_(s[0]); eng.flat_m.copy_(s[1]); eng.flat_v.copy_(s[2])
        eng.noise_step, eng.opt_step = s[3], s[4]
        eng.epoch_acc.zero_()
    s0 = snap()
    for k in range(K):
        eng.train_step(order[k], 1, n_pts=float(npts[k]))
    torch.cuda.synchronize()
    ref = (eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone(), eng.emb.clone(), eng.epoch_acc.clone(), eng.flat_g.clone())
    assert float((ref[0] - s0[0]).abs().max()) > 0
    restore(s0)
    g = GraphedTrainStep(eng, B, 1)                      # captures run the body: restore what they touched
    assert sorted(g.graphs_u) == [2, 4, 8, 16]
    restore(s0)
    g.load_schedule((order, npts))
    g.replay_all()
    torch.cuda.synchronize()
    assert not g.pending and eng.opt_step == s0[4] + K and eng.noise_step == s0[3] + K
    assert torch.equal(eng.flat_p, ref[0]), float((eng.flat_p - ref[0]).abs().max())
    assert torch.equal(eng.flat_m, ref[1]) and torch.equal(eng.flat_v, ref[2])
    assert torch.equal(eng.emb, ref[3])
    assert torch.equal(eng.epoch_acc, ref[4]), (eng.epoch_acc, ref[4])
    assert torch.equal(eng.flat_g, ref[5])               # the last step's gradients
    assert float(eng.epoch_acc[7]) == K


def _oracle_step(P, emb, gt, dist, ids, q, n_pts, noise_step, seed=0, layer_ids=None, relu_masks=None, keep=None):
    """The oracle's objective and gradients for the mini-batch `ids` with the engine's own noise draws."""
    from oracle import nvf_oracle as O
    P = {k: v.clone() for k, v in P.items()}
    keys = O.trainable_keys(P)
    for k in keys:
        P[k].requires_grad_(True)
    e = emb[ids].clone().requires_grad_(True)
    ch = emb.shape[1]
    u_latent = torch.from_numpy(latent_noise(seed, noise_step, ids, ch))
    u_w = None
    if q == 1:
        u_w = {n: torch.from_numpy(weight_noise(seed, noise_step, layer_ids[n], tuple(P["reconstructor." + n + ".kernel"].shape)))
               for n in TRUNK}
    out, cls, nbits, lbits = O.net_forward(P, e, "train", q, u_latent, u_w, keep=keep, relu_masks=relu_masks)
    g = gt[ids]
    pyr = O.gt_pyramid(g)
    loss = (O.surf_focal_dense(out, g, dist[ids], beta=1, alpha=0.9) + O.focal_dense(cls[0], pyr[0], alpha=0.85)
            + O.focal_dense(cls[1], pyr[1], alpha=0.85)
            + H["lmbda"] * (lbits.sum() / n_pts * H["w1"] + nbits.sum() / NPTS * H["w2"]))
    loss.backward()
    return loss.item(), out.detach(), [c.detach() for c in cls], {k: P[k].grad for k in keys}, e.grad


def _layer_ids(net):
    rec = net.reconstructor
    return {n: getattr(rec, n).layer_id for n in TRUNK}


# ReLU layers of the decoder (oracle name -> the engine's saved activation)
RELU_LAYERS = {"conv0": "y1", "up1": "y2", "conv1": "y3", "up2": "y4", "conv2": "y5"}
# Gradient bounds of the engine (default = Winograd forms included) against the oracle evaluated in FLOAT64 with the
# engine's own ReLU masks imposed (oracle/nvf_oracle.py decoder(relu_masks=)): max |difference| / max |slice|.  3 x the
# worst case measured on MI355X over both decoders of BASELINE.json at batch 16, q = 1 and 2 (tools/diag_masks.py,
# profiles/r05_relu_mask_parity.md: 1.9e-6 over the data-term slices, 2.4e-6 on a head bias, 1.05e-5 on the weight
# likelihood's mu -- a signed sum over 2e5 weights).  Why masks: a ReLU's derivative is discontinuous at 0; one
# pre-activation in ten million that two correctly rounded evaluations put on either side of zero (|x| < 1e-7 of the
# layer's range: measured, asserted below) switches a gradient entry on or off and moves slices by 1e-4 .. 8e-4 -- the
# fp32 oracle (oneDNN) is itself 2e-4 from float64 on the wide decoder for that reason.  With the masks imposed the
# comparison is about arithmetic, and holds 100 x tighter than SURVEY 8(c)'s 1e-4.
GRAD_TOL = 8e-6
GRAD_TOL_BY_SLICE = {"reconstructor.likelihood_model.mu": 3.5e-5}
MASK_FLIP_MAX_FRACTION = 1e-5        # of a layer's entries (measured: <= 5 of 8.4e6)
MASK_FLIP_MAX_ACTIVATION = 1e-6      # |activation| of a disagreeing entry / the layer's largest (measured: <= 1.2e-7)


def _oracle64_with_masks(eng, net, P, gt, dist, emb, ids, q, n_pts, a, tag):
    """(gradients, latent gradient) of the float64 oracle with the engine's ReLU masks imposed; asserts that the masks
    themselves disagree with the float64 pre-activations only where those are zero to rounding."""
    masks = {n: (a[k] > 0).cpu() for n, k in RELU_LAYERS.items()}
    keep = {}
    out = _oracle_step({k: v.double() for k, v in P.items()}, emb.double(), gt.double(), dist.double(), ids, q, n_pts,
                       eng.noise_step, layer_ids=_layer_ids(net), relu_masks=masks, keep=keep)
    nflip, worst = 0, 0.0
    for n, k in RELU_LAYERS.items():
        pre = keep[n + ".pre"].detach()
        flip = (pre > 0) != masks[n]
        big = float(pre.abs().max())
        if flip.any():
            nflip += int(flip.sum())
            w = float(torch.maximum(pre.abs(), a[k].cpu().double().abs())[flip].max()) / big
            worst = max(worst, w)
            assert int(flip.sum()) <= max(1, MASK_FLIP_MAX_FRACTION * flip.numel()), (tag, n, int(flip.sum()))
            assert w <= MASK_FLIP_MAX_ACTIVATION, (tag, n, w)
    print(f"[relu masks {tag}] {nflip} entries differ from the float64 oracle's; largest |activation| among them / layer max = {worst:.1e}")
    return out[3], out[4]


def _check_against_oracle(eng, net, P, gt, dist, emb, ids, q, tag=None):
    """One mini-batch step of the engine against the oracle: probabilities and loss against the oracle as the reference
    runs it (float32), every weight-gradient slice against the oracle in float64 with the engine's ReLU masks imposed."""
    ids = np.asarray(ids, np.int64)
    n_pts = float(eng.counts[ids].sum())
    lids = _layer_ids(net)
    a = eng.train_step(ids, q, update=False)
    loss_ref, out_ref, cls_ref, g_ref, _ = _oracle_step(P, emb, gt, dist, ids, q, n_pts, eng.noise_step, layer_ids=lids)
    assert float((a["p2"].cpu() - out_ref).abs().max()) < 1e-5
    assert float((a["p0"].cpu() - cls_ref[0]).abs().max()) < 1e-5 and float((a["p1"].cpu() - cls_ref[1]).abs().max()) < 1e-5
    assert abs(eng.loss_value() - loss_ref) < 2e-5 * abs(loss_ref), (eng.loss_value(), loss_ref)
    g64, _ = _oracle64_with_masks(eng, net, P, gt, dist, emb, ids, q, n_pts, a, tag)
    worst = (0.0, None)
    for name, (off, n) in eng.slices.items():
        mine = eng.flat_g[off:off + n].cpu().numpy().astype(np.float64)
        r = g64[name].numpy().reshape(-1)
        err = np.abs(mine - r).max() / max(np.abs(r).max(), 1e-30)
        if name not in GRAD_TOL_BY_SLICE:
            worst = max(worst, (err, name))
        assert err < GRAD_TOL_BY_SLICE.get(name, GRAD_TOL), (tag, name, err)
    print(f"[grad vs float64 oracle, masks imposed: {tag} q={q}] worst slice {worst[1]}: {worst[0]:.2e} (bound {GRAD_TOL:.0e})")
    return loss_ref


def _check_latent_gradient(eng, net, P, gt, dist, emb, q, tag):
    """The full-batch latent pass (n_pts = all resident blocks, NVFPCC.py:233-250) against the float64 oracle with the
    pass's own ReLU masks imposed."""
    a, de = eng.latent_step(q, update=False)
    ids = np.arange(eng.N_leaf)
    _, de64 = _oracle64_with_masks(eng, net, P, gt, dist, emb, ids, q, float(eng.counts.sum()), a, tag + "/latent")
    err = float((de.cpu().double() - de64).abs().max()) / float(de64.abs().max())
    print(f"[latent gradient vs float64 oracle, masks imposed: {tag} q={q}] {err:.2e} (bound {GRAD_TOL:.0e})")
    assert err < GRAD_TOL, (tag, err)


@pytest.mark.parametrize("q", [2, 1])
@pytest.mark.parametrize("dec", ["S", "W"])
def test_batch16_train_step_matches_the_oracle(dec, q, gpu):
    """The bench configuration's batch (16 blocks of 917 resident): loss, probabilities, all 28 gradient slices against the
    CPU oracle on the same 16 blocks -- slab counts, workgroup caps and the eight-wave kernel variants depend on the
    batch, and the golden vectors stop at batch 4.  q = 1 feeds the oracle the engine's counter-RNG draws (Philox
    restated in NumPy, tests/philox_np.py).  The latent gradient comes from a 16-block latent pass.  Both decoders of
    BASELINE.json (S: ch 3, 8,16,8,8; W: ch 8, 16,32,16,16 = configs[4]) through the DEFAULT engine -- the Winograd forms of
    the 4^3 layers included -- so the wide decoder's batch-16 launches are held to the oracle too, not only to its own
    direct forms."""
    ch, chans = (3, (8, 16, 8, 8)) if dec == "S" else (8, (16, 32, 16, 16))
    net, eng, P, gt, dist, emb = make(gpu, ch, chans, 40)
    assert eng.winograd and (eng.narrow if dec == "S" else eng.wide)
    ids = np.random.default_rng(3).permutation(40)[:16]
    _check_against_oracle(eng, net, P, gt, dist, emb, ids, q, tag="B16/" + dec)
    # latent gradient: the full-batch latent pass over 16 resident blocks
    net2, eng2, P2, gt2, dist2, emb2 = make(gpu, ch, chans, 16)
    _check_latent_gradient(eng2, net2, P2, gt2, dist2, emb2, q, "B16/" + dec)


# the decoders the engine has fused / matrix-core launches for; anything else must either run (generic kernels) and
# agree with the oracle, or refuse with a message naming these
CONFIGS3 = [(8, (8, 16, 8, 8)),       # the reference's argparse default: --ch 8 --chanstr 8,16,8,8 (NVFPCC.py:723-735)
            (4, (4, 8, 4, 4)),        # off-grid: no instantiation of the fused stem / one-launch heads / trunk5
            (3, (8, 8, 8, 8)),        # narrow trunk, other stem
            # the fused stem at other latent widths than the two of BASELINE.json (ch is the codec's rate knob) ...
            (1, (8, 16, 8, 8)), (5, (8, 16, 8, 8)),
            (9, (8, 16, 8, 8)),       # ... one past its limit: per-layer stem kernels, un-queued latent tail
            (3, (16, 32, 16, 16)), (5, (16, 32, 16, 16))]     # wide: up0 on the generic kernels under a fused stem


@pytest.mark.parametrize("ch,channels", CONFIGS3)
def test_other_channel_strings_match_the_oracle_or_refuse(ch, channels, gpu):
    """`--ch` / `--chanstr` beyond BASELINE.json's two decoders: forward + all gradients through whatever launches the
    engine picks, against the oracle -- or an explicit NotImplementedError that names the supported strings
    ("Decoder configurations")."""
    try:
        net, eng, P, gt, dist, emb = make(gpu, ch, channels, 6)
    except NotImplementedError as e:
        assert "8,16,8,8" in str(e) and "16,32,16,16" in str(e), str(e)
        return
    tag = "ch%d/%s" % (ch, ",".join(str(c) for c in channels))
    for q in (2, 1):
        _check_against_oracle(eng, net, P, gt, dist, emb, [4, 1, 3, 0], q, tag=tag)
    # latent gradient: round 4 allowed max(2e-4, 10 x the fp32 oracle's own distance from float64) here and blamed the
    # Gaussian-CDF ratio of the rate term; tools/diag_latent2.py (profiles/r05_relu_mask_parity.md) shows every stage of the
    # latent backward accurate to 1e-7 -- the 3.6e-4 at ch = 8 was ONE ReLU mask entry -- so the same bound as everywhere
    _check_latent_gradient(eng, net, P, gt, dist, emb, 2, tag)
    # eval forward is batch-invariant bit for bit here as well (rc_enc.ply == rc_dec.ply)
    p_all = eng.eval_forward(q=2)["p2"]
    one = eng.eval_forward(lo=3, hi=4, q=2)["p2"]
    assert torch.equal(one[0], p_all[3])


def test_winograd_step_equals_the_direct_step(gpu, monkeypatch):
    """Round 4 runs the 4^3 layers of a TRAINING step in a reduced-multiplication (Winograd) form.  With the engine's
    switch off (NVF_WINO=0: conv2's forward and backward-data and conv1's backward-data through the direct fixed-order
    kernels of rounds 1-3) the same step must give the same probabilities, loss and gradients to rounding -- and the EVAL
    forward must not depend on the switch at all, bit for bit (it never uses the Winograd kernels).  (conv2's weight
    gradient inside the five-gradient launch follows the engine's context -- nvf_step_ctx_set_direct -- too; its two
    forms are also compared by tests/test_gpu_ops.py::test_wgrad_k4_wino and ::test_three_mfma_weight_gradients_in_one_launch.)"""
    from nvfpcc_amd import engine as E
    got = {}
    for wino in (True, False):
        monkeypatch.setattr(E, "_WINO", wino)
        net, eng, P, gt, dist, emb = make(gpu, 3, (8, 16, 8, 8), 24)
        assert ("wino_dx" in eng.layers["conv2"].wp) == wino and ("wino_fwd" in eng.layers["conv2"].wp) == wino
        ids = np.arange(16)
        a = eng.train_step(ids, 1, update=False)
        ev = eng.eval_forward(lo=0, hi=5, q=2)["p2"].clone()
        got[wino] = (a["p2"].clone(), eng.loss_value(), eng.flat_g.clone(), ev)
    (p_w, l_w, g_w, e_w), (p_d, l_d, g_d, e_d) = got[True], got[False]
    assert torch.equal(e_w, e_d)
    assert float((p_w - p_d).abs().max()) < 1e-5
    assert abs(l_w - l_d) < 2e-5 * abs(l_d)
    for name, (off, n) in eng.slices.items():
        ref = g_d[off:off + n]
        err = float((g_w[off:off + n] - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
        assert err < 2e-5, (name, err)


def test_wide_winograd_step_equals_the_direct_step(gpu, monkeypatch):
    """The wide decoder (BASELINE configs[4]: --ch 8 --chanstr 16,32,16,16) runs conv2 / conv1 of a TRAINING step through
    conv16_wino.hip (forward, backward-data) and wgrad16_wino.hip (weight gradient).  With the engine's switch off
    (TrainEngine(winograd=False): the direct 16-row kernels of rounds 2-3, which the gradient goldens were pinned with)
    the same batch-16 step gives the same probabilities, loss and all gradients to rounding; the EVAL forward does not
    depend on the switch, bit for bit."""
    from nvfpcc_amd import engine as E
    got = {}
    for wino in (True, False):
        monkeypatch.setattr(E, "_WINO", wino)
        net, eng, P, gt, dist, emb = make(gpu, 8, (16, 32, 16, 16), 20)
        assert eng.wide and ("wino16_dx" in eng.layers["conv2"].wp) == wino and ("wino16_fwd" in eng.layers["conv2"].wp) == wino and "wino16_fwd" not in eng.layers["conv1"].wp
        ids = np.arange(16)
        a = eng.train_step(ids, 1, update=False)
        ev = eng.eval_forward(lo=0, hi=5, q=2)["p2"].clone()
        got[wino] = (a["p2"].clone(), eng.loss_value(), eng.flat_g.clone(), ev)
    (p_w, l_w, g_w, e_w), (p_d, l_d, g_d, e_d) = got[True], got[False]
    assert torch.equal(e_w, e_d)
    assert float((p_w - p_d).abs().max()) < 1e-5
    assert abs(l_w - l_d) < 2e-5 * abs(l_d)
    for name, (off, n) in eng.slices.items():
        ref = g_d[off:off + n]
        err = float((g_w[off:off + n] - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
        # (two Winograd layers, forward and backward, above the deepest parameters: measured 3.0e-5 at up0's kernel, 1e-5
        # or less elsewhere; the gradient goldens are held to 2e-4)
        assert err < 1e-4, (name, err)
