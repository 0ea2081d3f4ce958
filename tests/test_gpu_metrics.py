"""nvf_metrics / nvf_metrics3 (csrc/pointwise.hip, metrics_final_body in csrc/finals.h) against an exact reference.

The six sums of a term are tp, ap, tn, an at thh_acc and sse, denom at thh_sse (utils/loss.py:74-84, 113-121 of the
reference: `(p > thh)` is strict, occupied means `gt.bool()`).  Reference here: the five counts are int64 sums of boolean
masks (numpy, or torch on the device for the large cases), sse is a float64 sum of the float64 squares.  Counts must be
EXACT -- above 2^24, where a float32 cannot hold every integer, the true count rounded once -- and sse agrees to the 1e-5
test_focal_losses_match_reference_goldens puts on it.  ops.metrics and ops.metrics3 are never each other's reference."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
WG = 2048          # elements per workgroup of metrics_kernel (256 threads x 8)
MAXWG = 1024       # kLossMaxWG: above WG * MAXWG elements a term's workgroups walk a grid-stride loop
SSE_RTOL = 1e-5
_worst_sse = [0.0]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd import ops as _ops
    return _ops


def make_term(seed, n, occupancy, with_dist=True):
    """(p, gt, dist) of one term as float32 numpy arrays: its own seed and occupancy, so no two terms share a count."""
    rng = np.random.default_rng(seed)
    p = rng.random(n, dtype=np.float32)
    gt = (rng.random(n, dtype=np.float32) < occupancy).astype(np.float32)
    dist = (rng.random(n, dtype=np.float32) * 8).astype(np.float32) if with_dist else None
    return p, gt, dist


def ref6(p, gt, dist, thh_acc, thh_sse):
    """([tp, ap, tn, an, denom] as Python ints, sse as float64) of one term; thresholds compared as float32, like the kernel."""
    ta, ts = np.float32(thh_acc), np.float32(thh_sse)
    occ = gt != 0
    with np.errstate(invalid="ignore"):
        hi, lo, sel = p > ta, p <= ta, p > ts
    counts = [int((hi & occ).sum(dtype=np.int64)), int(occ.sum(dtype=np.int64)),
              int((lo & ~occ).sum(dtype=np.int64)), int((~occ).sum(dtype=np.int64)), int(sel.sum(dtype=np.int64))]
    sse = 0.0 if dist is None else float(np.square(dist.astype(np.float64))[sel].sum())
    return counts, sse


def check6(got, counts, sse, what, has_dist=True):
    """got: six float32 numbers of one term against ref6's."""
    got = np.asarray(got, np.float64)
    assert [got[0], got[1], got[2], got[3], got[5]] == [float(c) for c in counts], (what, got.tolist(), counts, sse)
    if not has_dist:
        assert got[4] == 0.0, (what, got[4])
        return
    err = abs(got[4] - sse) / sse if sse > 0 else abs(got[4])
    _worst_sse[0] = max(_worst_sse[0], err)
    assert err <= SSE_RTOL, (what, got[4], sse, err)


def cu(x):
    return None if x is None else torch.from_numpy(x).cuda()


LENGTHS = [1, 255, 257, 2047, 2048, 2049, WG * MAXWG - 1, WG * MAXWG, WG * MAXWG + 1, 65 * 32768]


@pytest.mark.parametrize("n", LENGTHS)
def test_one_term_at_every_length(ops, n):
    """One thread short of a wave / a workgroup, one workgroup and its neighbours, the 1024-workgroup cap and its
    neighbours (the first length at which a workgroup takes a second trip through the grid-stride loop), and 65 blocks of
    32^3, the first whole-block batch past the cap.  Both entry points."""
    p, gt, dist = make_term(1000 + n % 977, n, 0.07)
    counts, sse = ref6(p, gt, dist, 0.5, 0.6)
    P, G, D = cu(p), cu(gt), cu(dist)
    check6(ops.metrics(P, G, D, 0.5, 0.6).cpu().numpy(), counts, sse, ("metrics", n))
    check6(ops.metrics3([P], [G], [D], 0.5, 0.6).cpu().numpy(), counts, sse, ("metrics3", n))
    print(f"n = {n}: worst sse relative error so far {_worst_sse[0]:.2e} (bound {SSE_RTOL:.0e})")


@pytest.mark.parametrize("B", [5, 65])
def test_three_terms_of_different_lengths_in_one_launch(ops, B):
    """The engine's launch: the main output (B x 32^3), head 0 (B x 8^3), head 1 (B x 16^3).  At B = 65 term 0 sits at the
    1024-workgroup cap while terms 1 and 2 use 17 and 130 workgroups, so most workgroups of rows 1 and 2 return early and
    every term's partial sums must land at its own row offset.  A term without `dist` has sse exactly 0 and still counts
    its denominator."""
    ns = (B * 32768, B * 512, B * 4096)
    terms = [make_term(10 * B + t, n, occ) for t, (n, occ) in enumerate(zip(ns, (0.03, 0.4, 0.15)))]
    refs = [ref6(p, gt, None, 0.5, 0.6) for p, gt, _ in terms]
    refs_d = [ref6(p, gt, d, 0.5, 0.6) for p, gt, d in terms]
    assert len({tuple(c) for c, _ in refs}) == 3
    P, G, D = [cu(t[0]) for t in terms], [cu(t[1]) for t in terms], [cu(t[2]) for t in terms]
    for which in (0, 1):                      # the term that carries a distance map
        dists = [D[t] if t == which else None for t in range(3)]
        got = ops.metrics3(P, G, dists, 0.5, 0.6).cpu().numpy()
        assert got.shape == (18,)
        for t in range(3):
            counts, sse = refs_d[t] if t == which else refs[t]
            check6(got[6 * t:6 * t + 6], counts, sse, (B, which, t), has_dist=t == which)
    # two terms; the short one first, so the row of term 1 is the long one
    out = torch.full((12,), -3.0, device="cuda")
    got = ops.metrics3([P[1], P[0]], [G[1], G[0]], [None, D[0]], 0.5, 0.6, out=out).cpu().numpy()
    check6(got[0:6], *refs[1], (B, "two terms", 0), has_dist=False)
    check6(got[6:12], *refs_d[0], (B, "two terms", 1))
    # ... and a swapped pairing is a different answer (the data can tell the terms apart)
    assert refs[0][0] != refs[2][0] and refs[1][0] != refs[2][0]


def f32(x):
    return np.float32(x)


SPECIAL_P = [f32(0.0), np.nextafter(f32(0.5), f32(0)), f32(0.5), np.nextafter(f32(0.5), f32(1)),
             np.nextafter(f32(0.6), f32(0)), f32(0.6), np.nextafter(f32(0.6), f32(1)), f32(1.0), f32(np.nan)]
SPECIAL_GT = [f32(0.0), f32(-0.0), f32(1.0), f32(0.5)]


def test_threshold_edges_nan_and_signed_zero(ops):
    """`>` is strict at both thresholds; a NaN probability is neither a positive nor a negative hit and selects no squared
    distance; occupied means gt != 0, so -0.0 is empty and 0.5 is occupied."""
    combos = [(p, g) for p in SPECIAL_P for g in SPECIAL_GT]
    p = np.array([c[0] for c in combos], np.float32)
    gt = np.array([c[1] for c in combos], np.float32)
    dist = np.full(len(combos), 2.0, np.float32)
    # by hand: above 0.5 are 5 of the 9 values, at or below it 3, NaN is neither; above 0.6 are 2; 2 of the 4 gt occupied
    want = [5 * 2, 9 * 2, 3 * 2, 9 * 2, 2 * 4]
    counts, sse = ref6(p, gt, dist, 0.5, 0.6)
    assert counts == want and sse == 4.0 * 8
    check6(ops.metrics(cu(p), cu(gt), cu(dist), 0.5, 0.6).cpu().numpy(), want, 32.0, "36 combinations")
    # the same 36 pairs scattered over the workgroups of two terms of a three-term launch
    n = 5 * WG + 17
    terms = [make_term(77 + t, n, 0.2) for t in range(2)]
    for t, (tp, tg, td) in enumerate(terms):
        at = (np.arange(len(combos)) * 293 + 11 + 1000 * t) % n
        assert len(set(at.tolist())) == len(combos) and len(set((at // WG).tolist())) >= 5
        tp[at], tg[at] = p, gt
    ps = [terms[0], make_term(99, 300, 0.5), terms[1]]
    got = ops.metrics3([cu(t[0]) for t in ps], [cu(t[1]) for t in ps], [cu(ps[0][2]), None, cu(ps[2][2])],
                       0.5, 0.6).cpu().numpy()
    check6(got[0:6], *ref6(*ps[0], 0.5, 0.6), "edges, term 0")
    check6(got[6:12], *ref6(ps[1][0], ps[1][1], None, 0.5, 0.6), "edges, term 1", has_dist=False)
    check6(got[12:18], *ref6(*ps[2], 0.5, 0.6), "edges, term 2")
    # swapped thresholds give other counts on this data: the kernel cannot have used one threshold for both
    assert ref6(*ps[0], 0.6, 0.5)[0] != ref6(*ps[0], 0.5, 0.6)[0]


@pytest.mark.parametrize("fill", [0.0, 1.0])
def test_all_empty_and_all_full_ground_truth(ops, fill):
    n = 3 * WG + 5
    p, _, dist = make_term(5, n, 0.5)
    gt = np.full(n, fill, np.float32)
    counts, sse = ref6(p, gt, dist, 0.5, 0.6)
    got = ops.metrics(cu(p), cu(gt), cu(dist), 0.5, 0.6).cpu().numpy()
    check6(got, counts, sse, fill)
    if fill == 0.0:
        assert got[0] == 0 and got[1] == 0 and got[3] == n and got[2] > 0
    else:
        assert got[2] == 0 and got[3] == 0 and got[1] == n and got[0] > 0
    got3 = ops.metrics3([cu(p)] * 2, [cu(gt)] * 2, [None, cu(dist)], 0.5, 0.6).cpu().numpy()
    check6(got3[6:12], counts, sse, (fill, "metrics3"))


def test_accumulate_over_blocks_with_their_own_thresholds(ops):
    """The loop of NVFPCC.py encode under a per-block threshold (--thh_mode block-count): one accumulating call per block,
    both thresholds that block's.  Counts exact, sse to 1e-5 of the float64 sum; a prefilled `out` is added to, and
    without `accumulate` it is overwritten."""
    nb = 7
    p, gt, dist = (x.reshape(nb, 1, 32, 32, 32) for x in make_term(31, nb * 32768, 0.05))
    thh = torch.tensor([0.35 + 0.07 * b for b in range(nb)], dtype=torch.float32)
    P, G, D = cu(p), cu(gt), cu(dist)
    m = torch.zeros(6, device="cuda")
    for b, t in enumerate(thh.tolist()):
        ops.metrics(P[b:b + 1], G[b:b + 1], D[b:b + 1], t, t, out=m, accumulate=True)
    per = [ref6(p[b].reshape(-1), gt[b].reshape(-1), dist[b].reshape(-1), thh[b].item(), thh[b].item()) for b in range(nb)]
    counts = [sum(c[k] for c, _ in per) for k in range(5)]
    sse = sum(s for _, s in per)
    check6(m.cpu().numpy(), counts, sse, "per-block thresholds")
    # one threshold for all blocks is another answer
    assert ref6(p.reshape(-1), gt.reshape(-1), dist.reshape(-1), 0.5, 0.5)[0] != counts
    pre = torch.tensor([10.0, 20.0, 30.0, 40.0, 0.5, 60.0], device="cuda")
    m2 = pre.clone()
    ops.metrics(P[3:4], G[3:4], D[3:4], 0.5, 0.6, out=m2, accumulate=True)
    c3, s3 = ref6(p[3].reshape(-1), gt[3].reshape(-1), dist[3].reshape(-1), 0.5, 0.6)
    check6(m2.cpu().numpy(), [c3[0] + 10, c3[1] + 20, c3[2] + 30, c3[3] + 40, c3[4] + 60], s3 + 0.5, "prefilled")
    ops.metrics(P[3:4], G[3:4], D[3:4], 0.5, 0.6, out=m2, accumulate=False)
    check6(m2.cpu().numpy(), c3, s3, "overwritten")


def test_deferred_three_term_final_pass_equals_the_immediate_one(ops):
    """metrics3 queued through StepCtx.begin / flush (the training step's route, nvf_finals_flush) gives the bits of the
    immediate call, and `out` is untouched until the flush.  B = 40: term 0 has 640 workgroups, past one trip of the final
    pass's 16-row groups and past 512."""
    B = 40
    ns = (B * 32768, B * 512, B * 4096)
    terms = [make_term(300 + t, n, occ) for t, (n, occ) in enumerate(zip(ns, (0.03, 0.4, 0.15)))]
    P, G = [cu(t[0]) for t in terms], [cu(t[1]) for t in terms]
    dists = [cu(terms[0][2]), None, None]
    now = ops.metrics3(P, G, dists, 0.5, 0.6)
    ctx = ops.StepCtx()
    ctx.begin()
    out = torch.full((18,), -7.0, device="cuda")
    ops.metrics3(P, G, dists, 0.5, 0.6, out=out, ctx=ctx)
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    ctx.flush()
    torch.cuda.synchronize()
    assert torch.equal(out, now), (out, now)
    for t in range(3):
        counts, sse = ref6(terms[t][0], terms[t][1], terms[t][2] if t == 0 else None, 0.5, 0.6)
        check6(now[6 * t:6 * t + 6].cpu().numpy(), counts, sse, ("deferred", t), has_dist=t == 0)


@pytest.mark.parametrize("blocks", [917, 2048])
def test_counts_beyond_two_to_the_24_are_rounded_once(ops, blocks):
    """917 blocks of 32^3 (a whole 10-bit cloud resident: 30.0 M voxels) and 2048 blocks (67 M): the empty-voxel counts are
    far past 2^24, where float32 holds every second / fourth integer.  Every count must be the true count rounded ONCE to
    float32, |got - true| <= ulp(true) / 2 -- below 2^24 that is equality.  Per-workgroup partials are exact (a
    workgroup sees at most n / 1024 elements), so any excess is the final pass's.  Reference: int64 sums on the device.
    Measured figures: profiles/metrics_parity.md."""
    n = blocks * 32768
    g = torch.Generator(device="cuda").manual_seed(917)
    p = torch.rand(n, device="cuda", generator=g)
    gt = (torch.rand(n, device="cuda", generator=g) < 0.03).float()
    occ = gt != 0
    true = [int(((p > 0.5) & occ).sum()), int(occ.sum()), int(((p <= 0.5) & ~occ).sum()), int((~occ).sum()), None,
            int((p > 0.6).sum())]
    del occ
    for name, got in (("metrics", ops.metrics(p, gt, None, 0.5, 0.6)), ("metrics3", ops.metrics3([p], [gt], [None], 0.5, 0.6))):
        got = got.cpu().numpy()
        assert got[4] == 0.0
        errs = {}
        for k, label in ((0, "tp"), (1, "ap"), (2, "tn"), (3, "an"), (5, "denom")):
            ulp = float(np.spacing(np.float32(true[k])))
            errs[label] = (int(got[k]) - true[k], ulp)
        print(f"{blocks} blocks, {name}: got - true (ulp of true): " + ", ".join(f"{l} {e:+d} ({u:g})" for l, (e, u) in errs.items()))
        for label, (e, ulp) in errs.items():
            assert 2 * abs(e) <= ulp, (blocks, name, label, e, ulp)
