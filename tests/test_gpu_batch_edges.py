"""The merged weight-gradient launches and the bias sums one past their batch-size switch points.

The library picks slab counts and launch forms by batch size: 512 slabs per region (kMaxSlabs / _HEADS_SLABS), per-job
workgroup caps of 64 / 128 / 256 / 512, bias sums in ceil(B / 128)-block groups above 128 blocks (kSumChunks).  The rest
of the suite stays at or below 256 blocks; here every launch runs at 512 / 513 / 600 blocks (sums: 127 .. 600) and ALL
its outputs are held to float64 references that use no kernel of this project (tests/wgrad_ref64.py: one float64 einsum
per tap over shifted slices, torch's float64 matmul on the device; tests/test_modules_cpu.py pins it to torch's
autograd).  Inputs as in the Winograd tests: relu(randn * 0.7) activations, 60 %-dense randn output gradients.

Tolerances are the suite's: weight gradients 2e-5 of max |dW| (test_conv_weight_gradient, test_wgrad_k4_wino), bias /
channel sums 1e-5 (test_channel_sum), bit-equality where the existing tests claim it for the same pair of paths.  Every
case prints its largest error next to the error of the per-layer kernel (ops.wgrad) or of torch's fp32 sum on the same
inputs.  A job that reports more slabs than its region holds writes over its neighbours (errors of order 1): every
launch's job list is also checked against the regions allocated for it.
"""
import pytest
import torch

from tests.wgrad_ref64 import wgrad_ref64, channel_sum_ref64

pytestmark = pytest.mark.gpu

ENDS = (512, 513, 600)
# p, q, k, stride, pad of the narrow trunk's five gradients, in add_trunk5's order
TRUNK5 = (("conv2", "g5", "y4", 4, 1, 0), ("up2", "y3", "g4", 5, 2, 0), ("conv1", "g3", "y2", 4, 1, 0),
          ("up1", "y1", "g2", 5, 2, 0), ("conv0", "h0", "g1", 5, 2, 2))
HEADS = (("dl0", "y1"), ("dl1", "y3"), ("dl2", "y5"))
SUMS = ("g4", "g2", "g1", "dl2", "dl1", "dl0")          # the bias sums that ride in the engine's five-gradient launch


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd import ops as _ops
    return _ops


def rel_err(a, b):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1).to(a.device)
    return float((a - b).abs().max() / max(b.abs().max().item(), 1e-12))


class Inputs:
    def __init__(self, seed):
        self.g = torch.Generator(device="cuda").manual_seed(seed)

    def act(self, *s):
        return torch.relu(torch.randn(*s, device="cuda", generator=self.g) * 0.7)

    def grad(self, *s):
        return torch.randn(*s, device="cuda", generator=self.g) * (torch.rand(*s, device="cuda", generator=self.g) < 0.6)


def cube(B, c, n):
    return (B, c, n, n, n)


@pytest.fixture(scope="module")
def big(ops):
    """The tensors of a narrow decoder's backward pass at 600 blocks (a batch of B is their first B blocks) and the float64
    references of every output of the five-gradient launch at 512 / 513 / 600 blocks, built once."""
    B = ENDS[-1]
    r = Inputs(8100)
    t = {"g5": r.grad(*cube(B, 8, 32)), "y4": r.act(*cube(B, 8, 35)), "y3": r.act(*cube(B, 8, 16)),
         "g4": r.grad(*cube(B, 8, 35)), "g3": r.grad(*cube(B, 8, 16)), "y2": r.act(*cube(B, 8, 19)),
         "y1": r.act(*cube(B, 16, 8)), "g2": r.grad(*cube(B, 8, 19)),
         "h0": torch.randn(*cube(B, 8, 4), device="cuda", generator=r.g) * 0.7, "g1": r.grad(*cube(B, 16, 8)),
         "y5": r.act(*cube(B, 8, 32)), "dl0": r.grad(*cube(B, 1, 8)), "dl1": r.grad(*cube(B, 1, 16)),
         "dl2": r.grad(*cube(B, 1, 32))}
    ref = {e: {} for e in ENDS}
    for name, p, q, k, s, pad in TRUNK5:
        for e, dw in zip(ENDS, wgrad_ref64(t[p], t[q], k, s, pad, ENDS)):
            ref[e][name] = dw
    for h, (dl, x) in enumerate(HEADS):
        for e, dw in zip(ENDS, wgrad_ref64(t[dl], t[x], 3, 1, 1, ENDS)):
            ref[e]["head%d" % h] = dw
    for name in ("g5", "g3") + SUMS:
        for e, s in zip(ENDS, channel_sum_ref64(t[name], ENDS)):
            ref[e]["sum_" + name] = s
    torch.cuda.synchronize()
    yield t, ref
    t.clear()
    ref.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def layer_err(ops, big):
    """Error of the per-layer kernels (ops.wgrad: nvf_wgrad, other kernels with their own capped slabs, pinned to torch by
    test_conv_weight_gradient) against the same float64 references on the same inputs -- printed next to every merged
    launch's error -- and of torch's fp32 sums for the bias gradients."""
    t, ref = big
    out = {}
    for e in ENDS:
        for name, p, q, k, s, pad in TRUNK5:
            out[e, name] = rel_err(ops.wgrad(t[p][:e], t[q][:e], k, s, pad), ref[e][name])
        for h, (dl, x) in enumerate(HEADS):
            out[e, "head%d" % h] = rel_err(ops.wgrad(t[dl][:e], t[x][:e], 3, 1, 1), ref[e]["head%d" % h])
        for name in ("g5", "g3") + SUMS:
            out[e, "sum_" + name] = rel_err(t[name][:e].sum(dim=(0, 2, 3, 4)), ref[e]["sum_" + name])
    return out


def assert_jobs_fit(wg, caps=None):
    """Every pending reduction job's slabs end before the next region of the workspace begins (and before the workspace's
    used part ends), and none reports more than ``caps`` slabs."""
    assert wg.jobs
    jobs = sorted(wg.jobs)
    end = wg.ws.data_ptr() + wg.offset
    for (base, _, nslab, jtotal), nxt in zip(jobs, jobs[1:] + [None]):
        limit = nxt[0] if nxt is not None else end
        assert wg.ws.data_ptr() <= base and base + nslab * jtotal * 4 <= limit, (nslab, jtotal, limit - base)
        assert nslab > 0 and (caps is None or nslab <= caps), (nslab, jtotal)


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def check(what, got, want, bound, base=None):
    err = rel_err(got, want)
    print(f"{what}: rel err {err:.2e} (bound {bound:.0e}" + (f", per-layer / torch fp32: {base:.2e})" if base is not None else ")"))
    assert torch.isfinite(got).all(), what
    assert err < bound, (what, err, base)


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("form", ["plain", "bias", "heads", "sums"])
@pytest.mark.parametrize("B", ENDS)
def test_five_gradient_launch_at_and_past_the_slab_cap(ops, big, layer_err, B, form, direct):
    """WgradBatch.add_trunk5 in its four forms at 512 (the last batch at which conv0 runs on the matrix cores with one slab
    per block), 513 and 600 blocks, with a default context and with the direct forms, in a fresh default (128 MiB)
    workspace: the five dW, conv2's and conv1's bias gradients, the three heads' dW and the riding channel sums against
    float64.  Before the cap on conv0's matrix-core path its slabs 513.. landed on the bias and head regions that follow
    it in the workspace (written by other workgroups of the same launch): the capacity check and the heads' dW / bias
    gradients are what catch that.  Measured on an MI355X (largest over the 24 cases; the per-layer kernel on the same
    inputs in brackets): dW 7.7e-6 (conv2 at 600 blocks in the Winograd form; 1.3e-6), conv0's dW 2.2e-7, heads' dW 1.3e-6,
    bias gradients 7.1e-7, riding sums 5.9e-7 -- nothing needed a bound wider than the suite's 2e-5 / 1e-5."""
    t, ref = big
    ctx = ops.StepCtx()
    ctx.set_direct(direct)
    wg = ops.WgradBatch(torch.device("cuda"), ctx=ctx)
    ps = [t[p][:B] for _, p, q, k, s, pad in TRUNK5]
    qs = [t[q][:B] for _, p, q, k, s, pad in TRUNK5]
    outs = [nan(*ref[B][name].shape) for name, *_ in TRUNK5]
    bias = (nan(8), nan(8)) if form != "plain" else None
    heads = sums = None
    if form in ("heads", "sums"):
        heads = ([t[dl][:B] for dl, x in HEADS], [t[x][:B] for dl, x in HEADS], [nan(1, t[x].shape[1], 3, 3, 3) for dl, x in HEADS])
    if form == "sums":
        sums = ([t[n][:B] for n in SUMS], [nan(t[n].shape[1]) for n in SUMS])
        ctx.begin()
    wg.add_trunk5(ps, qs, outs, bias_outs=bias, heads=heads, sums=sums)
    assert len(wg.jobs) == {"plain": 5, "bias": 7, "heads": 10, "sums": 10}[form]
    assert_jobs_fit(wg, caps=512)
    wg.finish()
    if form == "sums":
        assert wg.sums_done
        torch.cuda.synchronize()
        assert all(torch.isnan(o).all() for o in sums[1])       # the final pass waits for the flush
        ctx.flush()
    torch.cuda.synchronize()
    for (name, *_), o in zip(TRUNK5, outs):
        check(f"B={B} {form} {name} dW", o, ref[B][name], 2e-5, layer_err[B, name])
    if bias is not None:
        check(f"B={B} {form} conv2 db", bias[0], ref[B]["sum_g5"], 1e-5, layer_err[B, "sum_g5"])
        check(f"B={B} {form} conv1 db", bias[1], ref[B]["sum_g3"], 1e-5, layer_err[B, "sum_g3"])
    if heads is not None:
        for h, o in enumerate(heads[2]):
            check(f"B={B} {form} head{h} dW", o, ref[B]["head%d" % h], 2e-5, layer_err[B, "head%d" % h])
    if sums is not None:
        for n, o in zip(SUMS, sums[1]):
            check(f"B={B} {form} sum {n}", o, ref[B]["sum_" + n], 1e-5, layer_err[B, "sum_" + n])


def test_latent_tail_rides_in_the_five_gradient_launch_at_600_blocks(ops, big, layer_err):
    """A queued latent tail as the first workgroup of a 600-block five-gradient launch: its outputs are the bits of
    nvf_latent_rate + nvf_gdn_bwd + nvf_wgrad (test_latent_tail_inside_the_slab_reduction_launch makes this comparison at
    B <= 40; the bias gradient to summation order), and the five dW of the launch are still right."""
    t, ref = big
    B, c = 600, 3
    g = torch.Generator(device="cuda").manual_seed(8200)
    R = lambda *s: torch.randn(*s, device="cuda", generator=g)
    lat, h, e, dx0 = R(B, c, 2, 2, 2) * 3, R(B, c, 2, 2, 2), R(B, c, 2, 2, 2), R(B, c, 2, 2, 2) * 0.1
    sigma, mu = torch.rand(c, device="cuda", generator=g) + 0.5, R(c) * 0.1
    beta, gamma = torch.rand(c, device="cuda", generator=g) + 0.5, torch.rand(c, c, device="cuda", generator=g) * 0.2
    ids = torch.arange(B, device="cuda") * 3 + 1
    g_dev = torch.tensor([0.37], device="cuda")
    for mode in ("train", "eval"):
        _, _, dlat_r, ds_r, dm_r = ops.latent_rate(lat, sigma, mu, mode, block_ids=ids, want_grad=True, g_dev=g_dev,
                                                   g_host=1.5, seed=9, step=4, dx_addend=dx0)
        dh_r, db_r, dg_r = ops.gdn_bwd(h, beta, gamma, dlat_r, False)
        dw_r = ops.wgrad(dh_r, e, 1, 1, 0)
        bias_r = dh_r.double().sum(dim=(0, 2, 3, 4))
        ctx = ops.StepCtx()
        wg = ops.WgradBatch(torch.device("cuda"), ctx=ctx)
        dlat, dh = torch.full_like(lat, float("nan")), torch.full_like(h, float("nan"))
        ds, dm, dbeta, dgamma = nan(c), nan(c), nan(c), nan(c, c)
        dw, dbias = nan(c, c, 1, 1, 1), nan(c)
        ops.latent_tail_queue(ctx, lat, sigma, mu, mode, ids, dx0, dlat, ds, dm, g_dev, 1.5, 9, 4, None, h, beta, gamma,
                              dh, dbeta, dgamma, e, dw, dbias)
        assert ctx.tail_pending()
        outs = [nan(*ref[B][name].shape) for name, *_ in TRUNK5]
        wg.add_trunk5([t[p] for _, p, *_ in TRUNK5], [t[q] for _, p, q, *_ in TRUNK5], outs)
        assert not ctx.tail_pending()
        assert_jobs_fit(wg, caps=512)
        wg.finish()
        torch.cuda.synchronize()
        for what, got, want in (("dlat", dlat, dlat_r), ("dsigma", ds, ds_r), ("dmu", dm, dm_r), ("dh", dh, dh_r),
                                ("dbeta", dbeta, db_r), ("dgamma", dgamma, dg_r), ("dw", dw, dw_r)):
            assert torch.equal(got, want), (mode, what, rel_err(got, want))
        check(f"tail {mode} bias", dbias, bias_r, 1e-5)
        for (name, *_), o in zip(TRUNK5, outs):
            check(f"tail {mode} {name} dW", o, ref[B][name], 2e-5, layer_err[B, name])


@pytest.mark.parametrize("B", [513, 600])
def test_three_and_two_gradient_launches_past_the_slab_cap(ops, big, layer_err, B):
    """nvf_wgrad_trunk_partial with three jobs (conv2 / up2 / conv1; default forms, direct forms, and z split 2 + conv1 in the Winograd
    form) and nvf_wgrad_up1_conv0_partial (the capped tile jobs) at 513 and 600 blocks against float64."""
    t, ref = big
    for what, setup in (("default", lambda c: None), ("direct", lambda c: c.set_direct(True)),
                        ("zsplit2+wino1", lambda c: c.set_wgrad_forms(2, True))):
        ctx = ops.StepCtx()
        setup(ctx)
        wg = ops.WgradBatch(torch.device("cuda"), ctx=ctx)
        outs = [nan(*ref[B][name].shape) for name, *_ in TRUNK5]
        wg.add_mfma3([t[p][:B] for _, p, *_ in TRUNK5[:3]], [t[q][:B] for _, p, q, *_ in TRUNK5[:3]], outs[:3])
        wg.add_up1_conv0([t[p][:B] for _, p, *_ in TRUNK5[3:]], [t[q][:B] for _, p, q, *_ in TRUNK5[3:]], outs[3:])
        assert len(wg.jobs) == 5
        assert_jobs_fit(wg, caps=512)
        wg.finish()
        torch.cuda.synchronize()
        for (name, *_), o in zip(TRUNK5, outs):
            check(f"B={B} {what} {name} dW", o, ref[B][name], 2e-5, layer_err[B, name])


@pytest.mark.parametrize("B", [513, 600])
def test_narrow_heads_launch_past_the_slab_cap(ops, big, layer_err, B):
    """nvf_heads3_wgrad_partial with the narrow decoder's heads (16 x 8^3, 8 x 16^3, 8 x 32^3) at the default 512 slabs
    and at 256."""
    t, ref = big
    for max_slabs in (512, 256):
        wg = ops.WgradBatch(torch.device("cuda"))
        outs = [nan(1, t[x].shape[1], 3, 3, 3) for dl, x in HEADS]
        wg.add_heads3([t[dl][:B] for dl, x in HEADS], [t[x][:B] for dl, x in HEADS], outs, max_slabs=max_slabs)
        assert_jobs_fit(wg, caps=max_slabs)
        wg.finish()
        torch.cuda.synchronize()
        for h, o in enumerate(outs):
            check(f"B={B} slabs={max_slabs} head{h} dW", o, ref[B]["head%d" % h], 2e-5, layer_err[B, "head%d" % h])


def test_wide_heads_launch_past_the_slab_cap(ops):
    """nvf_heads3_wgrad_partial with the wide decoder's heads (32 x 8^3 as two groups of 16 rows, 16 x 16^3, 16 x 32^3) at
    513 and 600 blocks."""
    r = Inputs(8300)
    shapes = [(32, 8), (16, 16), (16, 32)]
    xs = [r.act(*cube(600, c, s)) for c, s in shapes]
    dls = [r.grad(*cube(600, 1, s)) for c, s in shapes]
    refs = [wgrad_ref64(dl, x, 3, 1, 1, (513, 600)) for dl, x in zip(dls, xs)]
    try:
        for i, B in enumerate((513, 600)):
            wg = ops.WgradBatch(torch.device("cuda"))
            outs = [nan(1, c, 3, 3, 3) for c, s in shapes]
            wg.add_heads3([d[:B] for d in dls], [x[:B] for x in xs], outs)
            assert_jobs_fit(wg, caps=512)
            wg.finish()
            torch.cuda.synchronize()
            for h, o in enumerate(outs):
                base = rel_err(ops.wgrad(dls[h][:B], xs[h][:B], 3, 1, 1), refs[h][i])
                check(f"B={B} wide head{h} dW", o, refs[h][i], 2e-5, base)
    finally:
        del xs, dls, refs
        torch.cuda.empty_cache()


@pytest.mark.parametrize("w,B", [(32, 513), (16, 513), (16, 600)])
def test_wide_winograd_weight_gradient_past_the_slab_cap(ops, w, B):
    """wgrad16_k4_wino_partial (the wide decoder's conv2 / conv1, 16 -> 16 channels) at 513 and 600 blocks: at most 256
    slabs whatever the batch (w = 16 only at 600 blocks: [600, 16, 35^3] would be 1.6 GB per tensor).  Measured: 1.13e-5
    at w = 32, 513 blocks (the direct per-layer kernel on the same inputs: 2.4e-6)."""
    r = Inputs(8400 + w + B)
    x, gy = r.act(*cube(B, 16, w + 3)), r.grad(*cube(B, 16, w))
    want = wgrad_ref64(gy, x, 4, 1, 0)[0]
    try:
        wb = ops.WgradBatch(torch.device("cuda"))
        base = wb.reserve(256 * 16384 * 4)
        n = ops.wgrad16_k4_wino_partial(gy, x, base)
        assert 0 < n <= 256
        dw = nan(16 * 16 * 64)
        wb.add_job(base, dw, n, 16384)
        assert_jobs_fit(wb, caps=256)
        wb.finish()
        torch.cuda.synchronize()
        check(f"B={B} w={w} wide wino dW", dw.view(16, 16, 4, 4, 4), want, 2e-5, rel_err(ops.wgrad(gy, x, 4, 1, 0), want))
    finally:
        del x, gy, want
        torch.cuda.empty_cache()


SUM_SHAPES = ((8, 6), (16, 5), (1, 16), (3, 2))


@pytest.mark.parametrize("B", [127, 128, 129, 130, 255, 257, 600])
def test_bias_sums_across_the_chunk_count(ops, B):
    """multi_channel_sum, WgradBatch.finish_with_sums and channel_sum around kSumChunks = 128: up to 128 blocks one
    workgroup per (block, channel); above, groups of ceil(B / 128) blocks -- at 129 and 130 groups of two with 63 / 64 empty
    trailing groups, whose partials must still be written (as zeros) for the final pass.  Outputs are pre-filled with NaN.
    Against float64 sums (1e-5, test_channel_sum's bound); the deferred final passes give the immediate ones' bits
    (test_deferred_final_passes_equal_immediate_ones).
    The inputs are 60 %-dense randn + 0.25: an fp32 sum is accurate relative to sum |x|, and the bound is relative to
    |sum x|, so zero-mean inputs would test the seed's luck on the one-channel tensor, not the kernel (with zero mean the
    [128, 1, 16^3] sum came out at 3.7e-4 of a total that had cancelled to nothing, torch's own fp32 sum at 4.8e-5).  With
    the offset a dropped or doubled block is an error of 1 / B >= 1.6e-3 and an unwritten partial a NaN."""
    r = Inputs(8500 + B)
    xs = [r.grad(*cube(B, c, n)) + 0.25 for c, n in SUM_SHAPES]
    want = [channel_sum_ref64(x)[0] for x in xs]
    base = [rel_err(x.sum(dim=(0, 2, 3, 4)), s) for x, s in zip(xs, want)]
    h0, g1 = torch.randn(*cube(B, 8, 4), device="cuda", generator=r.g), r.grad(*cube(B, 16, 8))
    dw_want = wgrad_ref64(h0, g1, 5, 2, 2)[0]
    got = {}
    for defer in (False, True):
        # (a context's queue holds ONE deferred sum job, and its partials live in the context's workspace: one context each)
        ctx, ctx2 = ops.StepCtx(), ops.StepCtx()
        if defer:
            ctx.begin()
            ctx2.begin()
        outs = [nan(c) for c, n in SUM_SHAPES]
        ops.multi_channel_sum(xs, outs, ctx=ctx)
        wg = ops.WgradBatch(torch.device("cuda"), nbytes=64 << 20, ctx=ctx2)
        dw, outs2 = nan(8, 16, 5, 5, 5), [nan(c) for c, n in SUM_SHAPES]
        wg.add(h0, g1, 5, 2, 2, 0, dw)
        assert_jobs_fit(wg, caps=512)
        wg.finish_with_sums(xs, outs2)
        if defer:
            torch.cuda.synchronize()
            assert all(torch.isnan(o).all() for o in outs + outs2)
            ctx.flush()
            ctx2.flush()
        torch.cuda.synchronize()
        got[defer] = outs + outs2 + [dw]
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)
    outs, outs2, dw = got[False][:4], got[False][4:8], got[False][8]
    check(f"B={B} conv0 dW (nvf_wgrad_partial)", dw, dw_want, 2e-5)
    for i, (c, n) in enumerate(SUM_SHAPES):
        check(f"B={B} multi_channel_sum [{c},{n}^3]", outs[i], want[i], 1e-5, base[i])
        check(f"B={B} finish_with_sums [{c},{n}^3]", outs2[i], want[i], 1e-5, base[i])
        one = ops.channel_sum(xs[i], out=nan(c))
        check(f"B={B} channel_sum [{c},{n}^3]", one, want[i], 1e-5, base[i])
        two = ops.channel_sum(xs[i], out=one.clone(), accumulate=True)
        check(f"B={B} channel_sum accumulate [{c},{n}^3]", two, 2 * want[i], 1e-5, base[i])


def test_slab_counts_beyond_a_region_are_refused(ops):
    """The second line of defence: WgradBatch raises when a launch reports more slabs than the region it allocated."""
    with pytest.raises(RuntimeError):
        ops.WgradBatch._check_slabs("test", [512, 513], (512, 512))
    ops.WgradBatch._check_slabs("test", [512, 1], (512, 512))
