"""The numbers a user reads: TrainEngine.eval_sums -> NVFPCC.test_log_fields (the TEST line) and the counts a training step
writes into TrainEngine.step_counts -> nvf_step_tail -> train_log_fields (Pacc .. PSNR1 of the TRAIN line).

With the suite's synthetic perturbed weights no probability is decisive, so MSE1 is 0 / 0 and the accuracies sit at 0 or 1.
The three classifier biases are therefore shifted first (DECODERS[...]['shifts']: chosen from the float64 CPU oracle's logit quantiles over
the 21 evaluation blocks, nothing else), so that every head has voxels on both sides of its thresholds; the tests assert
that condition from the oracle before they look at the engine."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nvfpcc_amd.seeds import synthetic_seed
from nvfpcc_amd.synth import make_blocks
from tests.golden_inputs import CONFIGS, perturb_state_, make_emb
from tests.test_gpu_engine import H

pytestmark = pytest.mark.gpu
NPTS = 917 * 936.0
N_EVAL = 21
MARGIN = 2e-6      # a voxel whose float64 probability is this close to a threshold may fall on either side in float32
                   # (tests/test_gpu_net.py test_forward_eval_matches_reference)

# (ch, channels, param seed, latent seed) and the shifts of conv2_cls.b (main output), conv0_cls.b (head 0, 8^3) and
# conv1_cls.b (head 1, 16^3).  Oracle logit quantiles (5 %, 50 %, 95 %) over the 21 blocks before the shift:
#   S  main -0.17 / +0.07 / +0.38   head 0 -0.17 / +0.17 / +0.66   head 1 +0.16 / +0.49 / +0.88
#   W  main -0.83 / +0.46 / +2.07   head 0 -0.22 / +0.45 / +1.44   head 1 -0.68 / +0.20 / +1.33
# logit(0.5) = 0, logit(0.6) = 0.405.  S main + 0.10: about 10 % above 0.6 and 85 % above 0.5 (its logits span less than the
# distance between the two thresholds); the heads' medians are moved to 0.5; W main - 0.20: about 40 % / 62 %.
# "G" (no fused launch fits it: per-layer heads) serves the training-step test only, which needs nothing of it but nonzero
# counts and asserts that from each step's own outputs; assert_heads_are_decisive is not applied to it.  Its shifts move the
# oracle's eval-mode medians over 40 blocks (-0.80 / +0.22 / -0.36) to about +0.20 / 0 / 0.
DECODERS = {
    "S": dict(ch=CONFIGS["S"]["ch"], channels=CONFIGS["S"]["channels"], param_seed=CONFIGS["S"]["param_seed"],
              emb_seed=CONFIGS["S"]["emb_seed"], shifts=dict(conv2_cls=0.10, conv0_cls=-0.17, conv1_cls=-0.50)),
    "W": dict(ch=CONFIGS["W"]["ch"], channels=CONFIGS["W"]["channels"], param_seed=CONFIGS["W"]["param_seed"],
              emb_seed=CONFIGS["W"]["emb_seed"], shifts=dict(conv2_cls=-0.20, conv0_cls=-0.45, conv1_cls=-0.20)),
    "G": dict(ch=4, channels=(4, 8, 4, 4), param_seed=101, emb_seed=202, shifts=dict(conv2_cls=1.00, conv0_cls=-0.20, conv1_cls=0.35)),
}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


def host_state(tag):
    """The decoder's state dict on the host, biases shifted: what both the engine and the oracle start from."""
    from nvfpcc_amd import network
    from nvfpcc_amd.model import Net
    d = DECODERS[tag]
    network.reset_seed(synthetic_seed())
    network.set_noise_seed(0, 0)
    net = Net(None, "Gaussian", d["ch"], ",".join(str(c) for c in d["channels"]), verbose=False)
    sd = net.state_dict()
    perturb_state_(sd, d["param_seed"])
    for name, s in d["shifts"].items():
        sd["reconstructor." + name + ".b"].add_(s)
    net.load_state_dict(sd)
    return net, {k: v.clone() for k, v in net.state_dict().items()}


def make(tag, gpu, nblk, winograd=None):
    from nvfpcc_amd.engine import TrainEngine
    net, P = host_state(tag)
    net = net.to(gpu)
    gts, dists = make_blocks(nblk)
    gt, dist = torch.from_numpy(gts).float(), torch.from_numpy(dists).float()
    emb = make_emb(nblk, DECODERS[tag]["ch"], DECODERS[tag]["emb_seed"])
    eng = TrainEngine(net, gt.to(gpu), dist.to(gpu), n_points_total=NPTS, emb=emb.to(gpu), seed=0, winograd=winograd, **H)
    return net, eng, P, gt, dist, emb


@functools.lru_cache(maxsize=None)
def oracle_eval(tag, nblk=N_EVAL):
    """net(emb, 'eval', 2) of the float64 oracle on `nblk` blocks, with everything the TEST line is made of.  Computed once per
    decoder and never modified."""
    from oracle import nvf_oracle as O
    _, P = host_state(tag)
    P = {k: v.double() for k, v in P.items()}
    gts, dists = make_blocks(nblk)
    gt, dist = torch.from_numpy(gts).double(), torch.from_numpy(dists).double()
    emb = make_emb(nblk, DECODERS[tag]["ch"], DECODERS[tag]["emb_seed"]).double()
    with torch.no_grad():
        out, cls, nbits, lbits = O.net_forward(P, emb, "eval", 2)
        pyr = O.gt_pyramid(gt)
        o = dict(p=[out, cls[0], cls[1]], gt=[gt, pyr[0], pyr[1]], dist=dist, lbits=float(lbits.sum()),
                 nbits=float(nbits.sum()),
                 network_bits=float(nbits.sum()) + O.latent_header_bits(P) + O.decoder_aux_bits(DECODERS[tag]["channels"]),
                 focal=[float(O.surf_focal_dense(out, gt, dist, beta=1, alpha=0.9)),
                        float(O.focal_dense(cls[0], pyr[0], alpha=0.85)), float(O.focal_dense(cls[1], pyr[1], alpha=0.85))])
    return o


def near(p, thh):
    return (p - thh).abs() <= MARGIN


def assert_heads_are_decisive(o):
    """The condition on the INPUTS (oracle only): 5 % .. 95 % of every output above its thresholds, every numerator and
    denominator of the six ratios nonzero, at most 0.1 % of each denominator within MARGIN of a threshold.  Returns the
    number of such voxels per (head, threshold)."""
    close = {}
    for t, (p, gt) in enumerate(zip(o["p"], o["gt"])):
        occ = gt.bool()
        for thh in ((0.5, 0.6) if t == 0 else (0.5,)):
            frac = float((p > thh).double().mean())
            assert 0.05 <= frac <= 0.95, (t, thh, frac)
        tp, ap = int(((p > 0.5) & occ).sum()), int(occ.sum())
        tn, an = int(((p <= 0.5) & ~occ).sum()), int((~occ).sum())
        assert min(tp, ap, tn, an) > 0 and tp < ap and tn < an, (t, tp, ap, tn, an)
        n_pos, n_neg = int((near(p, 0.5) & occ).sum()), int((near(p, 0.5) & ~occ).sum())
        assert n_pos <= 1e-3 * ap and n_neg <= 1e-3 * an, (t, n_pos, ap, n_neg, an)
        close[(t, "pos")], close[(t, "neg")] = n_pos, n_neg
    denom = int((o["p"][0] > 0.6).sum())
    close["sse"] = int(near(o["p"][0], 0.6).sum())
    assert denom > 0 and close["sse"] <= 1e-3 * denom, (close["sse"], denom)
    return close


def exact_counts(ps, gts, dist):
    """18 reference sums of metrics3([p2, p0, p1], [gt, gt8, gt16], [dist, None, None], 0.5, 0.6) from tensors on the
    device: counts as Python ints, sse as float64."""
    ta, ts = torch.tensor(0.5, device=ps[0].device), torch.tensor(0.6, device=ps[0].device)
    ref = []
    for t, (p, gt) in enumerate(zip(ps, gts)):
        occ = gt != 0
        sel = p > ts
        sse = float((dist.double() ** 2)[sel].sum()) if t == 0 else 0.0
        ref += [int(((p > ta) & occ).sum()), int(occ.sum()), int(((p <= ta) & ~occ).sum()), int((~occ).sum()), sse,
                int(sel.sum())]
    return ref


def assert_counts(got, ref, what):
    got = np.asarray(got, np.float64)
    for k in range(18):
        if k % 6 == 4:
            assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), (what, k, got[k], ref[k])
        else:
            assert got[k] == ref[k], (what, k, got.tolist(), ref)


COUNT_IDX = [3 + 6 * t + k for t in range(3) for k in (0, 1, 2, 3, 5)]     # the 15 integer entries of eval_sums


@pytest.mark.parametrize("tag", ["S", "W"])
def test_eval_sums_are_the_sums_of_the_engines_own_outputs(tag, gpu):
    """sums[3:21] are exactly the counts of the engine's own eval_forward() outputs against gt and a pyramid pooled HERE
    from gt with F.max_pool3d (which also checks eng.gt16 / eng.gt8 and which head meets which level); sums[0:3] are the
    oracle's focal terms evaluated in float64 on those same outputs; sums[21] the oracle's latent bits."""
    from oracle import nvf_oracle as O
    o = oracle_eval(tag)
    assert_heads_are_decisive(o)
    net, eng, P, gt, dist, emb = make(tag, gpu, N_EVAL)
    a = eng.eval_forward()
    ps = [a["p2"], a["p0"], a["p1"]]
    g = gt.to(gpu)
    g16 = F.max_pool3d(g, 2, 2)
    gts = [g, F.max_pool3d(g16, 2, 2), g16]
    assert [tuple(p.shape) for p in ps] == [tuple(x.shape) for x in gts]
    sums = eng.eval_sums().double().cpu().numpy()
    assert sums.shape == (22,)
    ref = exact_counts(ps, gts, dist.to(gpu))
    assert min(ref[k] for k in range(18) if k % 6 != 4) > 0 and ref[4] > 0
    assert_counts(sums[3:21], ref, tag)
    p64 = [p.double().cpu() for p in ps]
    focal = [float(O.surf_focal_dense(p64[0], gt.double(), dist.double(), beta=1, alpha=0.9)),
             float(O.focal_dense(p64[1], o["gt"][1], alpha=0.85)), float(O.focal_dense(p64[2], o["gt"][2], alpha=0.85))]
    np.testing.assert_allclose(sums[0:3], focal, rtol=2e-5)
    np.testing.assert_allclose(sums[21], o["lbits"], rtol=2e-5)


@pytest.mark.parametrize("tag", ["S", "W"])
def test_eval_shards_add_up_to_the_whole(tag, gpu):
    """Every rank evaluates dist.shard_range of the blocks and the 22 sums are added: integer entries exactly, the others
    to 1e-5 of the float64 sum of the shards; an empty shard is 22 zeros; the 17 fields of the TEST line agree."""
    import NVFPCC
    from nvfpcc_amd import dist as nd
    assert_heads_are_decisive(oracle_eval(tag))
    engines = {n: make(tag, gpu, n) for n in (N_EVAL, 5)}
    for n, world in ((21, 2), (21, 3), (21, 8), (5, 8)):
        net, eng = engines[n][:2]
        whole = eng.eval_sums().double().cpu().numpy()
        parts = []
        for rank in range(world):
            lo, hi = nd.shard_range(n, rank, world)
            s = eng.eval_sums(lo, hi)
            assert s.shape == (22,)
            if hi <= lo:
                assert float(s.abs().sum()) == 0.0
            parts.append(s.double().cpu().numpy())
        assert sum(nd.shard_range(n, r, world)[1] - nd.shard_range(n, r, world)[0] for r in range(world)) == n
        assert (n, world) != (5, 8) or sum(float(np.abs(s).sum()) == 0.0 for s in parts) == 3
        total = np.sum(parts, axis=0)
        np.testing.assert_array_equal(total[COUNT_IDX], whole[COUNT_IDX])
        np.testing.assert_allclose(total, whole, rtol=1e-5)
        args = (eng.weight_bits(), float(eng.counts.sum()), NPTS, H["lmbda"], net.get_network_bits())
        f_whole, f_parts = NVFPCC.test_fields_from_sums(whole, *args), NVFPCC.test_fields_from_sums(total, *args)
        assert len(f_whole) == 17 and np.isfinite(np.asarray(f_whole, np.float64)).all()
        np.testing.assert_allclose(np.asarray(f_parts, np.float64), np.asarray(f_whole, np.float64), rtol=1e-5)
    lo, hi = nd.shard_range(5, 7, 8)
    assert hi <= lo and torch.equal(engines[5][1].eval_sums(lo, hi), torch.zeros(22, device=gpu))


def mse1_range(p, dist, sse, denom):
    """[least, greatest] value sse' / denom' can take when every voxel within MARGIN of 0.6 may or may not be selected
    (exact: the decided voxels are fixed, the undecided ones are added in the order that moves the ratio furthest)."""
    und = near(p, 0.6)
    sel = (p > 0.6) & ~und
    s0, n0 = float((dist[sel] ** 2).sum()), int(sel.sum())
    d2 = np.sort((dist[und] ** 2).numpy().reshape(-1))
    lo = hi = (s0, n0)
    for v in d2:                       # ascending: pull the ratio down while a voxel lies below it
        if lo[1] == 0 or v < lo[0] / lo[1]:
            lo = (lo[0] + v, lo[1] + 1)
    for v in d2[::-1]:
        if hi[1] == 0 or v > hi[0] / hi[1]:
            hi = (hi[0] + v, hi[1] + 1)
    return lo[0] / lo[1], hi[0] / hi[1], int(und.sum())


@pytest.mark.parametrize("peak", [1023, 4095])
@pytest.mark.parametrize("tag", ["S", "W"])
def test_the_test_line_equals_the_oracles(tag, peak, gpu):
    """The 17 fields of the reference's TEST line (its NVFPCC.py:308-392) written out from the float64 oracle -- Loss adds
    lambda * (b_latent + b_net) WITHOUT w1 / w2, as there -- against NVFPCC.test_log_fields on the engine.  Sums to 2e-5;
    a ratio may differ by the voxels within MARGIN of its threshold over its denominator (+ 1e-6); MSE1 lies in the exact
    range those voxels allow (+ 1e-5)."""
    import NVFPCC
    from oracle import nvf_oracle as O
    o = oracle_eval(tag)
    close = assert_heads_are_decisive(o)
    print(f"{tag}: voxels within {MARGIN:g} of a threshold: {close}")
    p, gts, dist = o["p"], o["gt"], o["dist"]
    n_pts = float(gts[0].sum())
    b_latent, b_net = o["lbits"] / n_pts, o["nbits"] / NPTS
    acc = [O.acc_dense(p[t], gts[t], thh=0.5) for t in range(3)]
    sse, denom = O.sse1(p[0], dist, 0.6)
    mse1 = float(sse) / float(denom)
    want = [sum(o["focal"]) + H["lmbda"] * (b_latent + b_net), 0.0, 0.0, float(acc[0][0]), float(acc[0][1]), o["focal"][1],
            o["focal"][2], float(acc[1][0]), float(acc[1][1]), float(acc[2][0]), float(acc[2][1]), b_latent + b_net, b_latent,
            b_net, (o["lbits"] + o["network_bits"]) / NPTS, mse1, 20 * np.log10(peak / np.sqrt(mse1 / 3))]
    net, eng, P, gt, dist_, emb = make(tag, gpu, N_EVAL)
    got = [float(x) for x in NVFPCC.test_log_fields(eng, net, NPTS, H["lmbda"], peak=peak)]
    assert len(got) == 17 and got[1] == 0.0 and got[2] == 0.0
    print(f"{tag} peak {peak}: TEST " + " ".join(f"{x:.6g}" for x in got))
    for k in (0, 5, 6, 11, 12, 13, 14):
        assert abs(got[k] - want[k]) <= 2e-5 * abs(want[k]), (k, got[k], want[k])
    for t, (kp, kn) in enumerate(((3, 4), (7, 8), (9, 10))):
        occ = gts[t].bool()
        tol_p = close[(t, "pos")] / float(occ.sum()) + 1e-6
        tol_n = close[(t, "neg")] / float((~occ).sum()) + 1e-6
        assert abs(got[kp] - want[kp]) <= tol_p and abs(got[kn] - want[kn]) <= tol_n, (t, got[kp], want[kp], got[kn], want[kn])
        assert 0.0 < got[kp] < 1.0 and 0.0 < got[kn] < 1.0
    lo, hi, n_und = mse1_range(p[0], dist, float(sse), float(denom))
    assert n_und == close["sse"] and lo <= mse1 <= hi
    assert lo * (1 - 1e-5) <= got[15] <= hi * (1 + 1e-5), (got[15], lo, hi)
    psnr = lambda m: 20 * np.log10(peak / np.sqrt(m / 3))
    assert psnr(hi) <= want[16] <= psnr(lo)
    assert psnr(hi * (1 + 1e-5)) - 1e-9 <= got[16] <= psnr(lo * (1 - 1e-5)) + 1e-9, (got[16], psnr(hi), psnr(lo))
    assert abs(got[16] - psnr(got[15])) <= 1e-9 * abs(got[16])


# (decoder, batch, winograd, switches of nvfpcc_amd.engine turned off, route, the plan.heads it must reach)
# "step": TrainEngine.train_step (the heads' forward deferred into the loss launch where one exists); "split": the same step
# from forward() and backward(), heads' forward in forward() -- the one route to "fused_loss" with weight gradients, where
# metrics3 is issued BEFORE the launch that turns the probabilities into logit gradients; "G": per-layer heads.
STEP_CASES = [
    ("S", 5, None, (), "step", "deferred"), ("S", 16, False, (), "step", "deferred"), ("S", 33, None, (), "step", "heads3"),
    ("S", 16, None, ("_SUMS_IN_TRUNK5", "_HEAD_BIAS_IN_LOSS"), "step", "deferred"),
    ("S", 16, None, ("_HEADS_IN_TRUNK5", "_STEM_IN_TRUNK5", "_STEM_IN_HEAD"), "step", "deferred"),
    ("S", 16, None, (), "split", "fused_loss"), ("S", 33, None, (), "split", "heads3"),
    ("W", 5, None, (), "step", "deferred"), ("W", 16, False, (), "step", "deferred"), ("W", 33, None, (), "step", "heads3"),
    ("W", 16, None, (), "split", "fused_loss"),
    ("G", 5, None, (), "step", "layers"),
]


def split_step(eng, ids, q):
    """train_step's launches with the heads' forward in forward(): host-launched, Adam tail included.  It restates the
    non-empty, single-GPU branch of TrainEngine.train_step line by line -- the noise_step bump, batch_and_prepare(with_rate,
    stem_mode="train"), forward, backward(want_w=True), the optimiser tail -- with two differences: defer_heads=False, and no
    `fuse` dict, so Adam runs in _tail() as it does behind a data-parallel hook.  A step added to train_step belongs here."""
    idx = torch.from_numpy(ids).to(eng.dev)
    n_pts = float(eng.counts[ids].sum())
    eng.noise_step += 1
    gt, dist, gt16, gt8, e, stem = eng.batch_and_prepare(idx, q, with_rate=True, stem_mode="train")
    a = eng.forward(e, "train", idx, defer_heads=False, stem=stem)
    eng.backward(a, gt, dist, gt16, gt8, n_pts, "train", idx, want_w=True, want_emb=False)
    eng._tail(n_pts)
    return a


@pytest.mark.parametrize("tag,batch,winograd,off,route,heads", STEP_CASES)
def test_a_steps_counts_are_that_steps_counts(tag, batch, winograd, off, route, heads, gpu, monkeypatch):
    """After every one of three real training steps (Adam included), step_counts[:18] are exactly the counts of the p2 / p0 /
    p1 that step returned, against that mini-batch's gt, its pyramid pooled here, and its dist -- for every order in which
    the step issues metrics3 relative to the loss launch.  Then the epoch accumulators hold the sum of the per-step ratios,
    of sse and of denom, and the TRAIN line's MSE1 / PSNR1 are finite and follow from them."""
    from nvfpcc_amd import engine as E
    for name in off:
        monkeypatch.setattr(E, name, False)
    net, eng, P, gt, dist, emb = make(tag, gpu, 40, winograd=winograd)
    assert eng._plan(batch, want_w=True, fuse=route == "step", step_head=True, defer_heads=route == "step").heads == heads
    eng.enable_epoch_stats()
    G, D = gt.to(gpu), dist.to(gpu)
    rng = np.random.default_rng(100 + batch)
    ratios, sse_sum, sse_ref, denom_sum = np.zeros(6), 0.0, 0.0, 0
    before = eng.flat_p.clone()
    for step in range(3):
        ids = rng.permutation(40)[:batch].astype(np.int64)
        a = eng.train_step(ids, 1) if route == "step" else split_step(eng, ids, 1)
        torch.cuda.synchronize()
        g = G[torch.from_numpy(ids).to(gpu)]
        g16 = F.max_pool3d(g, 2, 2)
        ref = exact_counts([a["p2"], a["p0"], a["p1"]], [g, F.max_pool3d(g16, 2, 2), g16], D[torch.from_numpy(ids).to(gpu)])
        assert min(ref[k] for k in range(18) if k % 6 != 4) > 0 and ref[4] > 0, ref      # a condition on the inputs
        got = eng.step_counts[:18].double().cpu().numpy()
        assert_counts(got, ref, (tag, batch, route, step))
        ratios += [ref[6 * t + k] / ref[6 * t + k + 1] for t in range(3) for k in (0, 2)]
        sse_sum, sse_ref, denom_sum = sse_sum + got[4], sse_ref + ref[4], denom_sum + ref[5]
    assert eng.opt_step == 3 and not torch.equal(eng.flat_p, before)
    acc = eng.read_epoch_stats()
    assert acc[7] == 3
    np.testing.assert_allclose(acc[8:14], ratios, rtol=1e-6)
    np.testing.assert_allclose(acc[14], sse_sum, rtol=1e-6)
    assert acc[15] == denom_sum
    for peak in (1023, 4095):
        f = eng.train_log_fields(acc, 3, peak=peak)
        assert len(f) == 16 and np.isfinite(np.asarray(f, np.float64)).all()
        np.testing.assert_allclose(f[14], sse_sum / denom_sum, rtol=1e-6)
        np.testing.assert_allclose(f[14], sse_ref / denom_sum, rtol=1e-5)
        np.testing.assert_allclose(f[15], 20 * np.log10(peak / np.sqrt((sse_sum / denom_sum) / 3)), rtol=1e-6)
        np.testing.assert_allclose(np.asarray(f[3:5] + f[7:11], np.float64), ratios / 3, rtol=1e-6)
