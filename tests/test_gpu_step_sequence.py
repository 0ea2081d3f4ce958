"""What one step of TrainEngine leaves behind for the next -- after a step that succeeded, and after one that did not.

A training step leaves a lot behind: the StepCtx queues (deferred final passes, the queued stem backward, the queued latent
tail), the pending reduction jobs and the slab offset of the WgradBatch, the arrival counters of the in-launch hand-overs
(csrc/stem_bwd.h, csrc/head_fwd.h: values cross workgroups through device-scope stores and loads because the eight XCD L2s are
not coherent for ordinary accesses), activation and workspace buffers reused at the same addresses, and the flags
_rate_ready / tail_done / sums_done.

Part A holds the cooperative (one-launch) forms of the engine to the separate-launch forms over a sequence of DIFFERENT
consecutive steps into the same buffers: a consumer that read last step's line, or a counter that did not return to zero, gives
other bits than the form that hands over at a launch boundary.  Part B leaves one library call out of a step (or raises
behind it), and holds the next step to the bits of an engine that never failed.

Every step here is host-launched; nothing captures or replays a graph.  No bound is new: bit equality, the 2e-6 of
test_stem_backward_inside_the_five_gradient_launch, and GRAD_TOL / GRAD_TOL_BY_SLICE of tests/test_gpu_measured_path.py."""
import time

import numpy as np
import pytest
import torch

from tests.test_gpu_engine import make
from tests.test_gpu_eval_line import split_step
from tests.test_gpu_measured_path import GRAD_TOL, GRAD_TOL_BY_SLICE

pytestmark = pytest.mark.gpu

STATE = ("flat_p", "flat_m", "flat_v", "emb", "emb_m", "emb_v")
COUNTERS = ("noise_step", "opt_step", "emb_step")
ACTS = ("h", "lat", "x0", "lbits", "a0", "h0", "y1", "p2")     # test_stem_forward_inside_the_step_head_launch's list
NBLK = 40


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


def copy_state(src, dst):
    """dst starts its next step from src's parameters, moments, latent table and step counters (its buffers, queues and
    arrival counters stay its own)."""
    for k in STATE:
        getattr(dst, k).copy_(getattr(src, k))
    for c in COUNTERS:
        setattr(dst, c, getattr(src, c))


def assert_idle(eng, where):
    """"No step in flight": nothing queued in the context, every arrival counter back at zero, no reduction pending."""
    assert not eng.ctx.stem_pending() and not eng.ctx.tail_pending(), where
    for key, t in eng.ctx._ws.items():
        if isinstance(key, str) and key.endswith("_flags"):
            assert int(t.abs().sum().item()) == 0, (where, key)
    assert eng._wg is None or (eng._wg.jobs == [] and eng._wg.offset == 0), (where, len(eng._wg.jobs), eng._wg.offset)


def rel_err(x, ref):
    """max |x - ref| / max |ref|: the slice error of tests/test_gpu_measured_path.py."""
    return float((x.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-30)


# ---------------------------------------------------------------------------------------------------------------------
# A. cooperative and separate forms over a sequence of different steps
# ---------------------------------------------------------------------------------------------------------------------
BATCHES = {"S": (16, 5, 32, 16, 3, 16), "W": (16, 3, 16, 5)}
# slices of the split_step case that are not the same bits at step 0 (see the test's docstring)
SPLIT_TO_ROUNDING = {"S": frozenset(), "W": frozenset()}


def sequence(tag, seed=40):
    """[(kind, ids, q)]: twelve (narrow) / eight (wide) train steps on slices of seeded permutations of the 40 blocks, batch
    sizes cycling so that consecutive steps use other workgroup counts and another number of arrival counters, the first
    half at q = 1 and the second at q = 2, and a latent step (the other plan on the same context) after the third and the
    sixth train step, as an epoch runs it."""
    rng = np.random.default_rng(seed)
    sizes = BATCHES[tag]
    n = 2 * len(sizes)
    steps = []
    for k in range(n):
        q = 1 if k < n // 2 else 2
        steps.append(("train", rng.permutation(NBLK)[:sizes[k % len(sizes)]].astype(np.int64), q))
        if k in (2, 5):
            steps.append(("latent", None, q))
    return steps


def assert_can_show_a_stale_read(name, prev, cur, where):
    """A condition on the inputs: a consumer that read step k's words in step k + 1 would read other bits.  ``prev`` and
    ``cur`` are compared over the elements the two steps share (the first min(B_k, B_k+1) blocks' worth).

    h, lat, lbits, a0, h0, p2, flat_g: they differ in at least half of those elements (measured: 99.9 % and more).
    Two tensors cannot meet that with any ids, because half of their elements are the same in EVERY block:
      y1 is a ReLU output, and 50 to 53 % of its units are off whatever the block (measured differing fraction 0.46 ..
         0.53): at least half of the elements that are on in either step differ;
      x0 is the rounded latent, integers on 4 (narrow) to 7 (wide) levels in a pattern the blocks largely share
         (measured 0.27 .. 0.55): every shared block row of it (24 / 64 floats, a cache line's worth) differs somewhere.
         Its image a0 = up0(x0), compared bit for bit as well, meets the first condition."""
    x, y = prev.reshape(-1), cur.reshape(-1)
    n = min(x.numel(), y.numel())
    ne = x[:n] != y[:n]
    if name == "x0":
        rows = min(prev.shape[0], cur.shape[0])
        assert bool(ne.reshape(rows, -1).any(dim=1).all()), (where, name, "a shared block row is the same bits")
        return
    if name == "y1":
        ne = ne[(x[:n] != 0) | (y[:n] != 0)]
    frac = float(ne.float().mean())
    assert frac >= 0.5, (where, name, frac)


@pytest.mark.parametrize("tag,case", [("S", "stem_in_head"), ("W", "stem_in_head"), ("S", "stem_in_trunk5"),
                                      ("S", "split_step"), ("W", "split_step")])
def test_cooperative_forms_equal_separate_forms_over_different_steps(gpu, monkeypatch, tag, case):
    """Engine A is the default engine; engine B, on the same parameters, takes the separate-launch form:

      stem_in_head    B has _STEM_IN_HEAD off (the stem's forward as a launch of its own).  Bit for bit: every saved
                      activation, the loss, every slice of flat_g -- and with them the Adam-updated parameters and moments.
      stem_in_trunk5  B has _STEM_IN_TRUNK5 off (the stem's backward as two launches).  Bit for bit: the loss and every slice
                      of flat_g except reconstructor.up0.b, a per-block wave sum added over the blocks in the cooperative
                      form: to 2e-6 of max |slice| (test_stem_backward_inside_the_five_gradient_launch).
      split_step      B runs tests/test_gpu_eval_line.py's split_step (defer_heads=False: the heads' forward in forward(),
                      loss and backward-data in nvf_heads3_loss_bwd_data_bias), A train_step(update=False) + _tail(n_pts)
                      (the heads' forward handed to the loss workgroups inside nvf_heads3_fwd_loss_bwd_data), so that
                      neither side fuses Adam.  Step 0, from clean engines, decides which slices of flat_g are compared as
                      bits and which to GRAD_TOL / GRAD_TOL_BY_SLICE; no later step may move a slice into the worse class.
                      Step-0 classification, both decoders: EVERY slice is the same bits (SPLIT_TO_ROUNDING is empty).
                      Read from the code: both sides plan the step with fuse=None and step_head=True, so they differ in
                      plan.heads alone ("deferred" against "fused_loss"), and nvf_heads3_fwd_loss_bwd_data is the forward
                      kernel's and the loss kernel's bodies with p handed over inside the launch -- "the bits of the two
                      calls" (ops.heads3_fwd_loss_bwd_data); every launch behind it is the same call on both sides.  The
                      activations, the loss and the updated parameters are therefore held to bits as well.

    Before every step B receives A's parameters, moments, latent table and counters, so a rounding-level difference never
    accumulates -- but each engine keeps its own buffers, queues and arrival counters from its own previous, different
    step.  After every step, on both engines: nothing pending in the context, every *_flags tensor zero, no reduction job.

    The inputs can show a stale read: between consecutive train steps every compared activation and flat_g differ in at
    least half of the elements the two steps share -- x0 and y1 in the form their values allow
    (assert_can_show_a_stale_read; asserted once per case, on engine A)."""
    from nvfpcc_amd import engine as E
    t0 = time.perf_counter()
    off = {"stem_in_head": "_STEM_IN_HEAD", "stem_in_trunk5": "_STEM_IN_TRUNK5"}.get(case)
    _, A, *_ = make(tag, gpu, nblk=NBLK)
    _, B, *_ = make(tag, gpu, nblk=NBLK)

    def on_b(fn):
        with monkeypatch.context() as m:
            if off is not None:
                m.setattr(E, off, False)
            return fn()

    history, to_rounding = [], None
    for step, (kind, ids, q) in enumerate(sequence(tag)):
        where = (tag, case, step, kind)
        copy_state(A, B)
        if kind == "latent":
            (_, de_a), (_, de_b) = A.latent_step(q), on_b(lambda: B.latent_step(q))
            assert torch.equal(de_a, de_b) and torch.equal(A.emb, B.emb), where
            assert_idle(A, where)
            assert_idle(B, where)
            continue
        if case == "split_step":
            n_pts = float(A.counts[ids].sum())
            a = A.train_step(ids, q, update=False)
            A._tail(n_pts)
            b = split_step(B, ids, q)
        else:
            a = A.train_step(ids, q)
            b = on_b(lambda: B.train_step(ids, q))
        torch.cuda.synchronize()
        assert_idle(A, where)
        assert_idle(B, where)
        assert (A.opt_step, A.noise_step) == (B.opt_step, B.noise_step), where
        la, lb = A.loss_value(), B.loss_value()
        assert la == lb, (where, la, lb)
        if case != "stem_in_trunk5":
            for k in ACTS:
                assert torch.equal(a[k], b[k]), (where, k)
        differs = {name for name, (o, n) in A.slices.items() if not torch.equal(A.flat_g[o:o + n], B.flat_g[o:o + n])}
        if case == "stem_in_head":
            allowed, tol = set(), {}
        elif case == "stem_in_trunk5":
            allowed, tol = {"reconstructor.up0.b"}, {"reconstructor.up0.b": 2e-6}
        else:
            if to_rounding is None:         # step 0 decides
                to_rounding = set(differs)
                print(f"[step-0 classification {tag}] to rounding: {sorted(to_rounding) or 'none'}")
                assert to_rounding <= SPLIT_TO_ROUNDING[tag], (where, sorted(to_rounding))
            allowed = to_rounding
            tol = {name: GRAD_TOL_BY_SLICE.get(name, GRAD_TOL) for name in allowed}
        assert differs <= allowed, (where, sorted(differs - allowed))
        for name in differs:
            o, n = A.slices[name]
            err = rel_err(A.flat_g[o:o + n], B.flat_g[o:o + n])
            print(f"[{tag} {case} step {step}] {name}: {err:.2e} (bound {tol[name]:.1e})")
            assert err <= tol[name], (where, name, err)
        if not allowed:                     # the same gradient bits through the same optimiser launches
            for k in STATE[:3]:
                assert torch.equal(getattr(A, k), getattr(B, k)), (where, k)
        compared = () if case == "stem_in_trunk5" else ACTS
        history.append({**{k: a[k].clone() for k in compared}, "flat_g": A.flat_g.clone()})
    for k, (prev, cur) in enumerate(zip(history, history[1:])):
        for name in prev:
            assert_can_show_a_stale_read(name, prev[name], cur[name], (tag, case, "train steps %d -> %d" % (k, k + 1)))
    print(f"[wall] sequence {tag} {case}: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------------------------------
# B. the step after a failed step
# ---------------------------------------------------------------------------------------------------------------------
class InjectedFailure(RuntimeError):
    pass


class Injector:
    """The Recorder of test_the_narrow_training_step_is_these_library_calls -- a proxy in front of nvfpcc_amd._lib._lib that
    lists every nvf_* entry point fetched -- extended in one way: the k-th fetch returns a function that raises
    InjectedFailure INSTEAD of making the call (mode "instead": a whole launch is left out, nothing on the device is
    interrupted), or makes the real call and raises when it returns (mode "after": an interrupt between two calls)."""

    def __init__(self, real, k=None, mode=None):
        self.real, self.calls, self.k, self.mode = real, [], k, mode

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("nvf_"):
            return fn
        i = len(self.calls)
        self.calls.append(name)
        if i != self.k:
            return fn

        def fail(*args):
            if self.mode == "after":
                fn(*args)
            raise InjectedFailure("%s call %d (%s)" % (self.mode, i, name))
        return fail


def recorded(monkeypatch, fn, k=None, mode=None):
    """(fn's result, the nvf_* calls it fetched), with the failure injected at call k."""
    from nvfpcc_amd import _lib as L
    inj = Injector(L.lib(), k, mode)
    with monkeypatch.context() as m:
        m.setattr(L, "_lib", inj)
        out = fn()
    return out, inj.calls


def snapshot(eng):
    return {k: getattr(eng, k).clone() for k in STATE + ("epoch_acc",)}, {c: getattr(eng, c) for c in COUNTERS}


def restore(eng, snap):
    for k, v in snap[0].items():
        getattr(eng, k).copy_(v)
    for c, v in snap[1].items():
        setattr(eng, c, v)


def tensors_of(out):
    """The tensors a step returned, by name: train_step's dict, latent_step's (dict, de)."""
    a, de = out if isinstance(out, tuple) else (out, None)
    d = {k: v for k, v in a.items() if torch.is_tensor(v)}
    if de is not None:
        d["de"] = de
    return d


def train(batch, q=1):
    def draw(rng):
        ids = rng.permutation(NBLK)[:batch].astype(np.int64)
        return lambda eng: eng.train_step(ids, q)
    return draw


def latent(q=1):
    def draw(rng):          # 33 blocks or more: one call list
        lo, hi = int(rng.integers(0, 4)), NBLK - int(rng.integers(0, 4))
        return lambda eng: eng.latent_step(q, lo, hi)
    return draw


def evaluate(rng):
    lo = int(rng.integers(0, NBLK - 16))
    return lambda eng: eng.eval_forward(lo, lo + 16)


def after_latent(rng):
    """The clean step behind a failed latent step: another latent step, then a mini-batch step (the phase that uses the
    WgradBatch and the queues)."""
    one, two = latent()(rng), train(16)(rng)

    def run(eng):
        a, de = one(eng)
        b = two(eng)
        return {**{"latent." + k: v for k, v in a.items()}, **b}, de
    return run


# tag, the clean step X1, the step X2 that fails, the clean step X3 behind it
FAIL_CONFIGS = {
    "narrow-16": ("S", train(16), train(16), train(16)),          # the 20-call step: every cooperative form
    "wide-16": ("W", train(16), train(16), train(16)),
    "narrow-33": ("S", train(33), train(33), train(33)),          # no cooperative form: another call list
    "narrow-latent": ("S", latent(), latent(), after_latent),
}


def fail_and_follow(monkeypatch, F, C, snap, draws, rng, k, mode, what):
    """One round of the protocol in test_the_step_after_a_failed_step's docstring; ``draws``: what X1, X2 and X3 are drawn
    from.  Returns X3's call list."""
    x1, x2, x3 = (d(rng) for d in draws)
    for eng in (F, C):
        restore(eng, snap)
        x1(eng)
    before = snapshot(F)
    with pytest.raises(InjectedFailure):
        recorded(monkeypatch, lambda: x2(F), k, mode)
    torch.cuda.synchronize()
    for name, v in before[0].items():
        if name != "epoch_acc":
            assert torch.equal(getattr(F, name), v), (what, "the failed step changed", name)
    assert (F.opt_step, F.emb_step) == (before[1]["opt_step"], before[1]["emb_step"]), what
    assert_idle(F, what)
    assert not F._rate_ready and not F.tail_done and not F._wg.sums_done, what
    F.noise_step = C.noise_step
    (out_f, calls_f), (out_c, calls_c) = recorded(monkeypatch, lambda: x3(F)), recorded(monkeypatch, lambda: x3(C))
    torch.cuda.synchronize()
    assert calls_f == calls_c, (what, "the next step left its plan", calls_f, calls_c)
    for name in STATE + ("flat_g", "epoch_acc"):
        assert torch.equal(getattr(F, name), getattr(C, name)), (what, "next step", name)
    assert F.loss_value() == C.loss_value(), what
    tf, tc = tensors_of(out_f), tensors_of(out_c)
    assert sorted(tf) == sorted(tc), what
    for name in tf:
        assert torch.equal(tf[name], tc[name]), (what, "next step returned", name)
    assert [getattr(F, c) for c in COUNTERS] == [getattr(C, c) for c in COUNTERS], what
    assert_idle(F, what)
    return calls_f


@pytest.mark.parametrize("config", list(FAIL_CONFIGS))
def test_the_step_after_a_failed_step(gpu, monkeypatch, config):
    """After any exception out of train_step / latent_step the engine is in the state "no step in flight", and its next
    step is the bits of an engine that never failed (TrainEngine._abandon_step).

    The call list is recorded from one clean step.  Then, for every call k of it in mode "instead", and for every k but the
    last in mode "after" (the last call holds the optimiser; after it the step has happened -- the wide decoder's optimiser
    is two launches, the slab reduction with fused Adam and the finals launch, and ONE call for that reason:
    nvf_wgrad_reduce_sums_fused_flush_tail), with ONE engine F reused over
    all of them -- failures follow failures -- and a control engine C that never fails:

      1. F and C are brought to the same snapshot (parameters, moments, latent table and its moments, the three step
         counters, epoch_acc) and both run the clean step X1;
      2. F attempts X2 (other ids) with the injection: InjectedFailure comes out of it;
      3. on F the parameters, moments, latent table, opt_step and emb_step are the bits from before the attempt, nothing
         is pending in the context, every arrival counter is zero, the WgradBatch holds no job and no slab, and
         _rate_ready / tail_done / sums_done are clear; noise_step is put back (the engine leaves it bumped);
      4. F and C run the clean step X3 (other ids again, optimiser included): the same list of library calls on both
         (a silent fall-back off the fused path would show here), and flat_g, parameters, moments, the latent table, the
         loss, every returned tensor and epoch_acc bit for bit; the counters equal.

    These injections cannot hang by construction.  A step is host-launched; mode "instead" leaves a WHOLE launch out and
    mode "after" a whole launch in; and every cooperating producer and its consumer sit in ONE launch (plan: the stem's
    forward workgroups in nvf_step_head_stem wait for nothing; the heads' forward -> loss hand-over is inside
    nvf_heads3_fwd_loss_bwd_data; the conv0^T partials -> per-block stem stage -> latent tail hand-over is inside
    nvf_wgrad_trunk_partial, which nvf_stem_bwd_queue and nvf_latent_tail_queue only prepare on the host; the step tail's
    arrival counter is inside the last launch) -- no launch waits for a launch that never comes."""
    t0 = time.perf_counter()
    tag, *draws = FAIL_CONFIGS[config]
    _, F, *_ = make(tag, gpu, nblk=NBLK)
    _, C, *_ = make(tag, gpu, nblk=NBLK)
    for eng in (F, C):
        eng.enable_epoch_stats()
    snap = snapshot(F)
    rng = np.random.default_rng(17)
    _, calls = recorded(monkeypatch, lambda: draws[1](rng)(F))
    torch.cuda.synchronize()
    print(f"[{config}] {len(calls)} calls: {calls}")
    # (narrow-16: the 20 calls of test_the_narrow_training_step_is_these_library_calls + the two of the epoch statistics)
    assert config != "narrow-16" or len([c for c in calls if not c.startswith("nvf_metrics")]) == 20, calls
    rounds = [("instead", k) for k in range(len(calls))] + [("after", k) for k in range(len(calls) - 1)]
    for mode, k in rounds:
        what = (config, mode, "call %d" % k, calls[k])
        fail_and_follow(monkeypatch, F, C, snap, draws, rng, k, mode, what)
    print(f"[wall] failed step {config}: {len(rounds)} rounds, {time.perf_counter() - t0:.2f} s")


def test_the_step_after_a_failed_eval_forward(gpu, monkeypatch):
    """The same injection on eval_forward, at its first and its last call: the training step behind it is the bits of an
    engine that never failed."""
    _, F, *_ = make("S", gpu, nblk=NBLK)
    _, C, *_ = make("S", gpu, nblk=NBLK)
    for eng in (F, C):
        eng.enable_epoch_stats()
    snap = snapshot(F)
    rng = np.random.default_rng(23)
    _, calls = recorded(monkeypatch, lambda: evaluate(rng)(F))
    last = len(calls) - 1
    assert last >= 2, calls
    for mode, k in (("instead", 0), ("after", 0), ("instead", last), ("after", last)):
        what = ("eval_forward", mode, "call %d" % k, calls[k])
        fail_and_follow(monkeypatch, F, C, snap, (train(16), evaluate, train(16)), rng, k, mode, what)
