"""engine.plan_step decides which launches a step consists of.  It takes no tensors, so every combination of its inputs
can be checked here, without a device, against the preconditions the library enforces with NVF_EINVAL
(launch_trunk_wgrads, csrc/wgrad.hip) and the batch limits of the cooperative launches."""
import itertools

from nvfpcc_amd.engine import StepPlan, plan_step

SWITCHES = ("head_bias_in_loss", "sums_in_trunk5", "stem_in_trunk5", "stem_in_head", "heads_in_trunk5")
CLASSES = {"narrow": dict(narrow=True, wide=False, ch=3), "wide": dict(narrow=False, wide=True, ch=8),
           "generic": dict(narrow=False, wide=False, ch=4)}


def make(cls, batch, want_w=True, want_emb=False, naive=0, winograd=True, hook=False, off=None, fuse=None, step=True):
    """The plan an engine of decoder class ``cls`` makes; ``step``: the train_step route (step head + deferred heads)."""
    c = CLASSES[cls]
    tuned_class = cls != "generic"
    sw = {s: s != off for s in SWITCHES}
    return plan_step(c["narrow"], c["wide"], winograd, tuned_class and c["ch"] <= 8, True, tuned_class, c["ch"], batch,
                     want_w, want_emb, (not hook) if fuse is None else fuse, hook, naive, *[sw[s] for s in SWITCHES],
                     step_head=step, defer_heads=step)


def test_every_plan_satisfies_what_the_library_requires():
    seen = set()
    for cls, batch, (want_w, want_emb), naive, wino, hook, off, step in itertools.product(
            CLASSES, (1, 5, 16, 32, 33, 64, 65, 512, 513), ((True, False), (False, True), (True, True)), (0, 1),
            (True, False), (True, False), (None,) + SWITCHES, (True, False)):
        p = make(cls, batch, want_w, want_emb, naive, wino, hook, off, step=step)
        what = (cls, batch, want_w, want_emb, naive, wino, hook, off, step, p)
        ch = CLASSES[cls]["ch"]
        if p.stem_bwd == "queued":
            assert p.tail_queued and p.trunk5 and p.heads_in_trunk5 and batch <= 32, what
        if p.sums_in_trunk5:
            assert p.heads_in_trunk5, what
        if p.heads_in_trunk5:
            assert p.trunk5, what
        if p.heads == "deferred":
            assert want_w and step and batch <= 32 and naive == 0 and cls != "generic", what
        if p.head_bias_in_loss:
            assert want_w and p.heads in ("deferred", "fused_loss"), what
        if p.heads in ("deferred", "fused_loss"):
            assert batch <= 32 and naive == 0, what
        if p.trunk5:
            assert cls == "narrow" and naive == 0 and want_w, what
        if p.tail_queued:
            assert want_w and not want_emb and ch <= 8, what
        if p.stem_fwd == "head":
            assert step and batch <= 32 and naive == 0 and off != "stem_in_head", what
        if p.conv0_wgrad_in_stem:
            assert want_w and not p.trunk5 and p.stem_bwd == "partial", what
        if p.fused_optimiser:
            assert not hook, what
        if not want_w:
            assert not (p.trunk5 or p.heads_in_trunk5 or p.tail_queued or p.sums_in_trunk5 or p.head_bias_in_loss), what
            assert p.stem_bwd in ("plain", "layers"), what
        if cls == "generic":
            assert p.stem_fwd == "layers" and p.stem_bwd == "layers" and p.heads == "layers", what
        assert (p.want_w, p.want_emb) == (want_w, want_emb), what
        seen.add(p)
    # each switch, the naive kernels and a batch above 32 change the plan of the step they belong to
    base = make("narrow", 16)
    assert all(make("narrow", 16, off=s) != base for s in SWITCHES)
    assert make("narrow", 16, naive=1) != base and make("narrow", 33) != base
    assert make("narrow", 16, winograd=False) == base         # kernel forms, not launches
    assert len(seen) > 20


def test_the_default_narrow_batch_16_step():
    """The single-GPU training step of the narrow decoder (README: 12 launches): everything rides in a merged launch."""
    assert make("narrow", 16) == StepPlan(
        want_w=True, want_emb=False, stem_fwd="head", latent_fwd_fused=True, heads="deferred", head_bias_in_loss=True,
        heads_in_trunk5=True, trunk5=True, conv0_wgrad_in_stem=False, stem_bwd="queued", tail_queued=True,
        sums_in_trunk5=True, fused_optimiser=True)
    # the latent phase of the same engine: no weight gradients, nothing queued
    assert make("narrow", 513, want_w=False, want_emb=True, fuse=False, step=False) == StepPlan(
        want_w=False, want_emb=True, stem_fwd="latent", latent_fwd_fused=True, heads="heads3", head_bias_in_loss=False,
        heads_in_trunk5=False, trunk5=False, conv0_wgrad_in_stem=False, stem_bwd="plain", tail_queued=False,
        sums_in_trunk5=False, fused_optimiser=False)
    # a data-parallel rank: the same launches, the optimiser behind the all-reduce
    assert make("narrow", 16, hook=True, fuse=True) == make("narrow", 16)._replace(fused_optimiser=False)
