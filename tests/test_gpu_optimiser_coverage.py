"""Every parameter gets exactly one Adam update per training step -- the device side of the coverage contract.

On one GPU a step has no optimiser launch of its own: adam_fused_elem (csrc/finals.h) is applied by whichever launch writes a
gradient element (the slab reduction, the bias / weight-rate / head-bias / IGDN final passes, and one workgroup that walks the
ranges TrainEngine._fused_tail computes as the complement of what those launches cover).  A fused step leaves its own gradient
in flat_g -- every writer stores the element, then updates from the stored value -- and the library states that the fused
arithmetic is nvf_adam_step's bit for bit (include/nvf_hip.h, NvfStepTail).  So after ANY step, whatever its plan,

    (p, m, v)_after == nvf_adam_step((p, m, v)_before, flat_g_after)        as bits, at every index

and an element whose gradient is not finite keeps p, m, v and is counted in epoch_acc[6].  No tolerance anywhere below except
against torch.optim.Adam (the reference's optimiser), where test_adam_matches_torch's applies."""
import functools

import numpy as np
import pytest
import torch

from nvfpcc_amd.seeds import synthetic_seed
from nvfpcc_amd.synth import make_blocks
from tests.golden_inputs import CONFIGS, perturb_state_, make_emb

pytestmark = pytest.mark.gpu
H = dict(lmbda=200.0, w1=10.0, w2=57.0, lr=1e-3, wemb=5.0)
# S / W: the two decoders of BASELINE.json; G: a decoder no fused launch is instantiated for (tests/test_gpu_eval_line.py)
DECODERS = {
    "S": dict(ch=CONFIGS["S"]["ch"], channels=CONFIGS["S"]["channels"], param_seed=CONFIGS["S"]["param_seed"],
              emb_seed=CONFIGS["S"]["emb_seed"]),
    "W": dict(ch=CONFIGS["W"]["ch"], channels=CONFIGS["W"]["channels"], param_seed=CONFIGS["W"]["param_seed"],
              emb_seed=CONFIGS["W"]["emb_seed"]),
    "G": dict(ch=4, channels=(4, 8, 4, 4), param_seed=101, emb_seed=202),
}
SWITCHES = ("_HEAD_BIAS_IN_LOSS", "_SUMS_IN_TRUNK5", "_STEM_IN_TRUNK5", "_STEM_IN_HEAD", "_HEADS_IN_TRUNK5")
QUANTISED = ("up0", "conv0", "up1", "conv1", "up2", "conv2", "conv2_cls")
TRUNK_BIAS = ("up0", "conv0", "up1", "conv1", "up2", "conv2")
HEAD_BIAS = ("conv0_cls", "conv1_cls", "conv2_cls")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _blocks():
    """The 70 synthetic blocks every engine below takes a prefix of (block j does not depend on how many are made)."""
    return make_blocks(70)


def make(tag, gpu, nblk, winograd=None):
    """tests/test_gpu_engine.py::make, with the generic decoder added."""
    from nvfpcc_amd import network
    from nvfpcc_amd.engine import TrainEngine
    from nvfpcc_amd.model import Net
    cfg = DECODERS[tag]
    network.reset_seed(synthetic_seed())
    network.set_noise_seed(0, 0)
    net = Net(None, "Gaussian", cfg["ch"], ",".join(str(c) for c in cfg["channels"]), verbose=False)
    sd = net.state_dict()
    perturb_state_(sd, cfg["param_seed"])
    net.load_state_dict(sd)
    net = net.to(gpu)
    gts, dists = _blocks()
    assert nblk <= gts.shape[0]
    gt = torch.from_numpy(gts[:nblk]).float().to(gpu)
    dist = torch.from_numpy(dists[:nblk]).float().to(gpu)
    emb = make_emb(nblk, cfg["ch"], cfg["emb_seed"]).to(gpu)
    eng = TrainEngine(net, gt, dist, n_points_total=917 * 936.0, emb=emb, seed=0, winograd=winograd, **H)
    return net, eng


def bits(t):
    return t.contiguous().view(torch.int32)


def slice_of(eng, i):
    for name, (off, n) in eng.slices.items():
        if off <= i < off + n:
            return "%s[%d]" % (name, i - off)
    return "outside every slice"


def assert_same_bits(eng, what, got, ref, where=None):
    """got == ref as bits (on the elements `where` selects); the message names the first differing index and its slice."""
    ne = bits(got) != bits(ref)
    if where is not None:
        ne &= where
    if bool(ne.any()):
        idx = torch.nonzero(ne).reshape(-1)
        i = int(idx[0])
        raise AssertionError("%s: %d of %d elements differ; first at flat index %d = %s: got %r, expected %r"
                             % (what, idx.numel(), ne.numel(), i, slice_of(eng, i), float(got[i]), float(ref[i])))


# flat_g is allocated as zeros and never cleared: every writer overwrites its elements.  An element that a launch claims but
# never reaches would keep g = 0, m = v = 0 and its parameter, and nvf_adam_step of that is the same nothing.  So the tests put
# this value into every element before a step; none may be left afterwards (a computed gradient with exactly these bits is
# a 2^-32 event per element).
SENTINEL = 1.2345678e-3


def arm(eng):
    eng.flat_g.fill_(SENTINEL)


def assert_all_written(eng, what, g):
    left = bits(g) == bits(torch.full((1,), SENTINEL, device=g.device))
    if bool(left.any()):
        idx = torch.nonzero(left).reshape(-1)
        i = int(idx[0])
        raise AssertionError("%s: %d gradient elements were never written by the step; first at flat index %d = %s"
                             % (what, idx.numel(), i, slice_of(eng, i)))


def adam_reference(p0, m0, v0, g, lr, step):
    """nvf_adam_step on copies of the pre-step state."""
    from nvfpcc_amd import ops
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    ops.adam_step(p, g, m, v, lr, step)
    return p, m, v


def pick_ids(rng, nblk, batch):
    """`batch` distinct block ids out of nblk = batch + 5, in permuted order: never a contiguous ascending run."""
    while True:
        ids = rng.permutation(nblk)[:batch].astype(np.int64)
        if batch == 1 or not np.array_equal(ids, np.arange(ids[0], ids[0] + batch)):
            return ids


# ------------------------------------------------------------------ 1. exactly one update per element, every plan
def _case(tag, batch, q=2, winograd=None, off=(), hook=False):
    name = "%s-b%d-q%d" % (tag, batch, q)
    if winograd is False:
        name += "-direct"
    for s in off:
        name += "-no" + s.lower()
    if hook:
        name += "-hook"
    return pytest.param(tag, batch, q, winograd, tuple(off), hook, id=name)


UPDATE_CASES = (
    [_case("S", b) for b in (1, 5, 16, 32, 33, 65)]
    + [_case("S", 16, q=1), _case("S", 16, winograd=False)]
    + [_case("S", 16, off=(s,)) for s in SWITCHES]
    + [_case("S", 16, hook=True)]
    + [_case("W", b) for b in (3, 16, 33)]
    + [_case("G", b) for b in (5, 16)]
)


@pytest.mark.parametrize("tag,batch,q,winograd,off,hook", UPDATE_CASES)
def test_every_element_gets_one_adam_update(gpu, monkeypatch, request, tag, batch, q, winograd, off, hook):
    """Three consecutive updating steps (from the second on the moments are non-zero: a writer that read stale m / v shows):
    after each, p / m / v over their whole length are nvf_adam_step of the pre-step state and the gradient the step left."""
    from nvfpcc_amd import engine as E
    for s in off:
        monkeypatch.setattr(E, s, False)
    nblk = batch + 5
    assert nblk <= 70
    net, eng = make(tag, gpu, nblk, winograd=winograd)
    if hook:
        eng.grad_hook = lambda flat: None          # the data-parallel route over one rank: nvf_step_tail behind the hook
    eng.enable_epoch_stats()
    rng = np.random.default_rng(1000 + batch)
    n = eng.flat_p.numel()
    routes = []
    for k in range(3):
        ids = pick_ids(rng, nblk, batch)
        p0, m0, v0 = eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone()
        step0 = eng.opt_step
        arm(eng)
        eng.train_step(ids, q, update=True)
        torch.cuda.synchronize()
        routes.append(bool(eng.tail_done))
        assert eng.opt_step == step0 + 1
        g = eng.flat_g.clone()
        assert_all_written(eng, "step %d" % k, g)
        assert bool(torch.isfinite(g).all()), "step %d left a non-finite gradient" % k
        p1, m1, v1 = adam_reference(p0, m0, v0, g, eng.lr, eng.opt_step)
        for what, got, ref in (("flat_m", eng.flat_m, m1), ("flat_v", eng.flat_v, v1), ("flat_p", eng.flat_p, p1)):
            assert got.numel() == ref.numel() == n
            assert_same_bits(eng, "step %d, %s" % (k, what), got, ref)
        if k == 0:
            # the comparison above must not be one of two no-ops: the step moved (nearly) every parameter, and something in
            # every slice that has a gradient
            changed = bits(eng.flat_p) != bits(p0)
            frac = float(changed.float().mean())
            print("changed in step 1: %.5f of %d parameters" % (frac, n))
            assert frac >= 0.99, frac
            for name, (o, c) in eng.slices.items():
                if bool((g[o:o + c] != 0).any()):
                    assert bool(changed[o:o + c].any()), name
    acc = eng.epoch_acc.cpu()
    assert float(acc[6]) == 0 and float(acc[7]) == 3, acc
    print("ROUTE %s -> %s" % (request.node.callspec.id, " / ".join("fused" if r else "separate tail" for r in routes)))
    if tag == "S" and not off and not hook and batch <= 32:
        assert all(routes), "the narrow decoder's default plan must end in the fused tail (the fallback was checked instead)"
    if hook:
        assert not any(routes)


# ------------------------------------------------------------------ 2. non-finite gradients, every writer
NONFINITE_CASES = [
    pytest.param("S", 16, (), False, id="S-b16-one-launch"),
    pytest.param("S", 16, ("_SUMS_IN_TRUNK5", "_HEAD_BIAS_IN_LOSS"), False, id="S-b16-sums-then-flush-tail"),
    pytest.param("S", 33, (), False, id="S-b33"),
    pytest.param("W", 16, (), False, id="W-b16"),
    pytest.param("S", 16, (), True, id="S-b16-hook"),
]
POISONED = "reconstructor.conv0_cls.b"     # head 0 only: its loss term, conv0_cls and everything upstream of y1


def _category(eng, names):
    mask = torch.zeros(eng.flat_p.numel(), dtype=torch.bool, device=eng.flat_p.device)
    for name in names:
        off, n = eng.slices[name]
        mask[off:off + n] = True
    return mask


def _poisoned_step(gpu, tag, batch, hook):
    """One clean step, then one with head 0's bias NaN.  Returns (eng, state before the poisoned step, its gradient)."""
    nblk = batch + 5
    net, eng = make(tag, gpu, nblk)
    if hook:
        eng.grad_hook = lambda flat: None
    eng.enable_epoch_stats()
    rng = np.random.default_rng(2000 + batch)
    eng.train_step(pick_ids(rng, nblk, batch), 2, update=True)
    off, n = eng.slices[POISONED]
    eng.flat_p[off:off + n] = float("nan")
    snap = (eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone())
    arm(eng)
    eng.train_step(pick_ids(rng, nblk, batch), 2, update=True)
    torch.cuda.synchronize()
    g = eng.flat_g.clone()
    assert_all_written(eng, "the poisoned step", g)
    return eng, snap, g


@pytest.mark.parametrize("tag,batch,off,hook", NONFINITE_CASES)
def test_nonfinite_gradients_are_skipped_and_counted(gpu, monkeypatch, request, tag, batch, off, hook):
    """A NaN parameter makes part of the gradient non-finite.  Every writer of the step -- not only nvf_step_tail -- must keep
    p / m / v of such an element, count it in epoch_acc[6], and update every other element as usual."""
    from nvfpcc_amd import engine as E
    for s in off:
        monkeypatch.setattr(E, s, False)
    eng, (p0, m0, v0), g = _poisoned_step(gpu, tag, batch, hook)
    print("ROUTE nonfinite %s -> %s" % (request.node.callspec.id, "fused" if eng.tail_done else "separate tail"))
    assert eng.opt_step == 2
    assert bool(eng.tail_done) == (not hook), "this case is about the %s route" % ("separate tail" if hook else "fused")
    n = g.numel()
    bad = ~torch.isfinite(g)
    nbad = int(bad.sum())
    per_slice = {name: int(bad[o:o + c].sum()) for name, (o, c) in eng.slices.items() if bool(bad[o:o + c].any())}
    print("non-finite gradient entries: %d of %d: %s" % (nbad, n, per_slice))
    assert 0 < nbad < n
    cats = {"quantised kernel": ["reconstructor.%s.kernel" % x for x in QUANTISED],
            "trunk bias": ["reconstructor.%s.b" % x for x in TRUNK_BIAS],
            "head bias": ["reconstructor.%s.b" % x for x in HEAD_BIAS]}
    for cat, names in cats.items():
        mask = _category(eng, names)
        assert bool((bad & mask).any()), "no non-finite gradient in a " + cat
        assert bool((~bad & mask).any()), "no finite gradient in a " + cat
    assert bool((bad & _category(eng, ["reconstructor.activation.beta"])).any())
    acc = eng.epoch_acc.cpu()
    assert float(acc[7]) == 2
    assert float(acc[6]) == nbad, ("epoch_acc[6] = %d, non-finite gradient entries = %d (missing %d); per slice: %s"
                                   % (int(acc[6]), nbad, nbad - int(acc[6]), per_slice))
    for what, got, ref in (("flat_m", eng.flat_m, m0), ("flat_v", eng.flat_v, v0), ("flat_p", eng.flat_p, p0)):
        assert_same_bits(eng, what + " where the gradient is not finite (must be kept)", got, ref, where=bad)
    p1, m1, v1 = adam_reference(p0, m0, v0, g, eng.lr, eng.opt_step)
    for what, got, ref in (("flat_m", eng.flat_m, m1), ("flat_v", eng.flat_v, v1), ("flat_p", eng.flat_p, p1)):
        assert_same_bits(eng, what + " where the gradient is finite", got, ref, where=~bad)
    assert float(acc[5]) >= 1
    with pytest.raises(ValueError, match="Problem in loss"):
        eng.read_epoch_stats()
    # the same case again, the objective's own counter cleared: the gradient count alone must trip the guard
    eng, _, g2 = _poisoned_step(gpu, tag, batch, hook)
    assert float(eng.epoch_acc[6]) == int((~torch.isfinite(g2)).sum()) == nbad
    eng.epoch_acc[5] = 0.0
    with pytest.raises(ValueError, match="Problem with grad"):
        eng.read_epoch_stats()


# ------------------------------------------------------------------ 3. graph replay == host steps, wide and generic
@pytest.mark.parametrize("tag,batch", [("W", 16), ("G", 8)])
def test_schedule_replay_equals_host_steps_wide_and_generic(gpu, tag, batch):
    """tests/test_gpu_measured_path.py::test_unrolled_schedule_replay_equals_host_steps for the decoders it leaves out: six
    steps = one 4-step graph + one 2-step graph from a device-resident schedule (Adam's coefficients read from device
    memory) against six host-launched train_steps from the same state, bit for bit (q = 1: weight and latent noise on)."""
    from nvfpcc_amd.engine import GraphedTrainStep
    nblk, K = 40, 6
    net, eng = make(tag, gpu, nblk)
    eng.enable_epoch_stats()
    order = np.stack([np.random.default_rng(30 + k).permutation(nblk)[:batch] for k in range(K)]).astype(np.int64)
    npts = eng.counts[order].sum(axis=1).astype(np.float64)
    snap = lambda: (eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone(), eng.noise_step, eng.opt_step)

    def restore(s):
        eng.flat_p.copy_(s[0]); eng.flat_m.copy_(s[1]); eng.flat_v.copy_(s[2])
        eng.noise_step, eng.opt_step = s[3], s[4]
        eng.epoch_acc.zero_()
    s0 = snap()
    emb0 = eng.emb.clone()
    arm(eng)
    for k in range(K):
        eng.train_step(order[k], 1, n_pts=float(npts[k]))
    torch.cuda.synchronize()
    ref = (eng.flat_p.clone(), eng.flat_m.clone(), eng.flat_v.clone(), eng.emb.clone(), eng.epoch_acc.clone(),
           eng.flat_g.clone())
    assert float((ref[0] - s0[0]).abs().max()) > 0 and torch.equal(ref[3], emb0)
    assert_all_written(eng, "host steps", ref[5])
    restore(s0)
    g = GraphedTrainStep(eng, batch, 1, unroll=(4, 2))      # captures run the body: restore what they touched
    assert sorted(g.graphs_u) == [2, 4]
    restore(s0)
    arm(eng)
    g.load_schedule((order, npts))
    g.replay_all()
    torch.cuda.synchronize()
    print("ROUTE replay %s-b%d -> %s" % (tag, batch, "fused" if eng.tail_done else "separate tail"))
    assert bool(eng.tail_done) == (tag == "W"), "W replays the fused tail, the generic decoder nvf_step_tail"
    assert not g.pending and eng.opt_step == s0[4] + K and eng.noise_step == s0[3] + K
    for what, got, want in (("flat_p", eng.flat_p, ref[0]), ("flat_m", eng.flat_m, ref[1]), ("flat_v", eng.flat_v, ref[2]),
                            ("flat_g", eng.flat_g, ref[5])):
        assert_same_bits(eng, what, got, want)
    assert torch.equal(eng.emb, ref[3])
    assert torch.equal(eng.epoch_acc, ref[4]), (eng.epoch_acc, ref[4])
    assert float(eng.epoch_acc[7]) == K and float(eng.epoch_acc[6]) == 0


# ------------------------------------------------------------------ 4. small things
def test_latent_step_updates_its_rows_only(gpu):
    """latent_step over blocks [3, 11) of 16: rows outside keep the latent table and both moments; rows inside are
    nvf_adam_step of the gradient the step returned, with the latents' learning rate and step count."""
    net, eng = make("S", gpu, 16)
    lo, hi = 3, 11
    inside = torch.zeros(16, dtype=torch.bool, device=gpu)
    inside[lo:hi] = True
    p_dec = eng.flat_p.clone()
    for k in range(2):
        e0, m0, v0 = eng.emb.clone(), eng.emb_m.clone(), eng.emb_v.clone()
        a, de = eng.latent_step(2, lo=lo, hi=hi)
        torch.cuda.synchronize()
        assert eng.emb_step == k + 1 and tuple(de.shape) == (hi - lo,) + tuple(eng.emb.shape[1:])
        assert bool(torch.isfinite(de).all()) and float(de.abs().max()) > 0
        ref = adam_reference(e0[lo:hi].reshape(-1), m0[lo:hi].reshape(-1), v0[lo:hi].reshape(-1), de.reshape(-1).clone(),
                             eng.lr_emb, eng.emb_step)
        for what, got, before, want in (("emb", eng.emb, e0, ref[0]), ("emb_m", eng.emb_m, m0, ref[1]),
                                        ("emb_v", eng.emb_v, v0, ref[2])):
            assert torch.equal(bits(got[~inside]), bits(before[~inside])), what + ": a row outside [3, 11) changed"
            assert torch.equal(bits(got[lo:hi].reshape(-1)), bits(want)), what + ": rows inside [3, 11)"
        assert not torch.equal(eng.emb[lo:hi], e0[lo:hi])
    assert torch.equal(eng.flat_p, p_dec), "the latent phase must not touch the decoder"


ADAM_MAGNITUDES = (0.0, 1e-30, 1e-20, 1e-4, 1e4, 1e19)


@pytest.mark.parametrize("n", [1, 63, 65, 1025, 5001])
def test_adam_kernels_equal_each_other_and_torch_adam(gpu, n):
    """nvf_adam_step and nvf_step_tail (device and host coefficients in turn) against torch.optim.Adam on the CPU in float32
    -- the reference's optimiser -- over five steps, gradient magnitudes from 0 to 1e19 of both signs mixed within one
    buffer (1e19^2 = 1e38 is still a float32; 1e-20^2 is a subnormal).  Tolerance on p: test_adam_matches_torch's.  The two
    kernels: the same bits in p, m and v.

    The moments against torch's exp_avg / exp_avg_sq: gradients of 1e19 and 1e-30 share a buffer and m can cancel (0.9 m and
    0.1 g of opposite sign), so a relative tolerance on the result means nothing; the bound is on the arithmetic.  With G the
    largest |g| an element has seen, |m| <= G.  A step of either implementation rounds at most three times (m * b1,
    g * (1 - b1), the sum; torch: g - m, the product, the sum), each by <= 2^-24 of a value <= 1.1 G, and the two hold
    1 - b1 to 2^-24 of each other: <= 8 * 2^-24 * G of new difference per step, old difference shrinking by b1 < 1 -- over
    five steps <= 40 * 2^-24 * G.  The same for v with G^2 (b2 < 1).  Below the smallest normal float32 (1.2e-38) neither side
    promises digits: that is the absolute part."""
    from nvfpcc_amd import ops
    gen = torch.Generator().manual_seed(700 + n)
    lr = 1e-3
    p0 = torch.randn(n, generator=gen)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=lr)
    p_a, p_b = p0.to(gpu), p0.to(gpu)
    m_a, v_a, m_b, v_b = (torch.zeros(n, device=gpu) for _ in range(4))
    coef = torch.zeros(2, device=gpu)
    mags = torch.tensor(ADAM_MAGNITUDES)
    g_max = torch.zeros(n)
    for step in range(1, 6):
        # every magnitude in (nearly) equal numbers, shuffled; the rotation by `step` walks a buffer shorter than the list
        # through it, so that n = 1 sees 1e-30, 1e-20, 1e-4, 1e4, 1e19 in turn and not whatever one draw gives it
        cls = (torch.arange(n) + step) % len(mags)
        cls = cls[torch.randperm(n, generator=gen)]
        sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
        grad = sign * mags[cls]
        p_ref.grad = grad.clone()
        opt.step()
        g_max = torch.maximum(g_max, grad.abs())
        g = grad.to(gpu)
        ops.adam_step(p_a, g, m_a, v_a, lr, step)
        c = ops.adam_coefficients(lr, step)
        if step % 2:
            coef.copy_(torch.tensor(c))
            ops.step_tail(p_b, g, m_b, v_b, coef)
        else:
            ops.step_tail(p_b, g, m_b, v_b, None, c)
        for what, a, b in (("p", p_a, p_b), ("m", m_a, m_b), ("v", v_a, v_b)):
            assert torch.equal(bits(a), bits(b)), "step %d: nvf_adam_step and nvf_step_tail differ in %s" % (step, what)
        assert bool(torch.isfinite(p_a).all() and torch.isfinite(m_a).all() and torch.isfinite(v_a).all())
    assert torch.allclose(p_a.cpu(), p_ref.detach(), rtol=1e-6, atol=1e-7), float((p_a.cpu() - p_ref.detach()).abs().max())
    assert float((p_a.cpu() - p0).abs().max()) > 0
    st = opt.state[p_ref]
    for what, got, want, scale in (("m", m_a, st["exp_avg"], g_max), ("v", v_a, st["exp_avg_sq"], g_max * g_max)):
        err = (got.cpu().double() - want.double()).abs()
        bound = 40 * 2.0 ** -24 * scale.double() + 1.2e-38
        print("%s: max err / bound = %.3f" % (what, float((err / bound).max())))
        assert bool((err <= bound).all()), (what, float((err / bound).max()))
