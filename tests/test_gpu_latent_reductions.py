"""The reductions over a whole batch on the latent side -- the latent rate, the GDN backward's parameter gradients, the
latent tail, the focal sums -- held to float64 ABOVE the batch sizes at which each kernel changes its code path.

The reference is the oracle (oracle/nvf_oracle.py: entropy_coder, gdn3d, floor_ste) in float64 with autograd on the CPU,
and float64 einsums for the 1x1x1 weight / bias gradient (tests/latent_inputs.py); it uses no kernel of this project.
tests/test_latent_inputs_cpu.py proves without a GPU that every case lands on the path its comment names and that the
inputs meet the conditions the bounds rely on.

Bounds.  Elementwise outputs keep the suite's figures (x_rounded as bits; dx rtol 1e-4 + 1e-5 max|dx|; GDN y, dx 1e-5).
Sums follow the rule of tests/test_gpu_trained_state.py: err < max(t, 3 * d32) with t the suite's figure for the
quantity and d32 the float32 CPU oracle's own distance from float64 on the same inputs; every case prints the two side
by side.  Measured: profiles/latent_reductions_parity.md."""
import functools

import pytest
import torch

from oracle import nvf_oracle as O
from tests import latent_inputs as L
from tests.test_gpu_ops import focal_reference64

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    from nvfpcc_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.cuda().contiguous()


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check_sums(tag, got, r64, r32, figures):
    """figures: name -> t.  Prints every row, then asserts the rule on each."""
    rows = []
    for name, t in figures.items():
        err, d32 = L.max_rel(got[name], r64[name]), L.max_rel(r32[name], r64[name])
        print(L.fmt_row(tag, name, err, d32, t))
        rows.append((name, err, L.bound(t, d32)))
    for name, err, b in rows:
        assert torch.isfinite(got[name]).all(), (tag, name)
        assert err < b, (tag, name, err, b)


# ---- 1. latent rate past the path switch -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rate_inputs(c, B):
    return L.rate_inputs(c, B)


def _rate_call(ops, inp, mode, lo, hi, g_dev, g_host):
    kmode, u = L.rate_noise(inp, mode)
    return ops.latent_rate(dev(inp["x"][lo:hi]), dev(inp["sigma"]), dev(inp["mu"]), kmode,
                           u=dev(u[lo:hi]) if mode == "train_u" else None, block_ids=dev(inp["ids"][lo:hi]),
                           want_grad=True, g_dev=dev(g_dev), g_host=g_host, seed=L.RATE_SEED, step=L.RATE_STEP,
                           dx_addend=dev(inp["addend"][lo:hi]))


@pytest.mark.parametrize("mode", L.RATE_MODES)
@pytest.mark.parametrize("c,B,path", L.RATE_CASES)
def test_latent_rate_on_both_sides_of_the_path_switch(ops, c, B, path, mode):
    """ops.latent_rate at the last size of the LDS path and on the channel-major loop path behind it (see RATE_CASES):
    eval, train with a given u, train with the counter noise of permuted, non-contiguous block ids; one channel with
    negative sigma, a dx_addend, the upstream gradient once as a negative device scalar and once as a host factor.

    dx is also bit for bit what the op gives on 16-block slices: the two paths must not differ per element.  (They did
    in the last bit until rate_term spelled out how its pdf difference is rounded: profiles/latent_reductions_parity.md.)"""
    assert L.rate_path(c, B) == path
    inp = _rate_inputs(c, B)
    kmode, u = L.rate_noise(inp, mode)
    assert float(L.likelihood64(inp["x"], inp["sigma"], inp["mu"], kmode, u).min()) > 5e-3
    for variant, g_dev, g_host in (("g_dev", torch.tensor([-0.37]), 1.0), ("g_host", None, 0.37)):
        g = g_host * (float(g_dev[0]) if g_dev is not None else 1.0)
        tag = f"rate c={c} B={B} {path} {mode} {variant}"
        r64 = L.rate_ref(inp["x"], inp["sigma"], inp["mu"], kmode, u, g, inp["addend"], F64)
        r32 = L.rate_ref(inp["x"], inp["sigma"], inp["mu"], kmode, u, g, inp["addend"], F32)
        xr, bits, dx, ds, dm = _rate_call(ops, inp, mode, 0, B, g_dev, g_host)
        torch.cuda.synchronize()
        # elementwise: the rounded latents as bits, dx per element
        assert torch.equal(bits_of(xr), bits_of(torch.round(inp["x"])))
        assert torch.equal(xr.cpu().double(), r64["rounded"])
        assert torch.isfinite(dx).all()
        scale = float(r64["dx"].abs().max())
        worst = float(((dx.cpu().double() - r64["dx"]).abs() / (1e-4 * r64["dx"].abs() + 1e-5 * scale)).max())
        print(f"[{tag}] dx: worst element at {worst:.3f} of rtol 1e-4 + 1e-5 max|dx|")
        assert torch.allclose(dx.cpu().double(), r64["dx"], rtol=1e-4, atol=1e-5 * scale)
        # ... and bit for bit what the same op gives on mini-batches of the same blocks (the LDS path's copy of the
        # element arithmetic)
        for lo in range(0, B, L.SLICE):
            hi = min(lo + L.SLICE, B)
            xr_s, _, dx_s, _, _ = _rate_call(ops, inp, mode, lo, hi, g_dev, g_host)
            assert torch.equal(bits_of(dx_s), bits_of(dx[lo:hi])), (tag, lo)
            assert torch.equal(bits_of(xr_s), bits_of(xr[lo:hi])), (tag, lo)
        # the sums
        check_sums(tag, {"bits": bits, "dsigma": ds, "dmu": dm}, r64, r32, {"bits": 1e-5, "dsigma": 1e-4, "dmu": 1e-4})


# ---- 2. GDN backward across its forms ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gdn_inputs(c, spatial, B, below):
    return L.gdn_inputs(c, spatial, B, below)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("c,spatial,B,below,what", L.GDN_CASES)
def test_gdn_backward_in_every_form(ops, c, spatial, B, below, what, inverse):
    """ops.gdn_fwd / ops.gdn_bwd in the forms nvf_gdn_bwd chooses from (see GDN_CASES): one workgroup or slabs +
    gdn_bwd_final, 8 / 4 / 1 threads per voxel, one or two tiles per workgroup; below-bound parameters where the case
    table says so (then gdn_bwd_final applies the LowerBound rule)."""
    inp = _gdn_inputs(c, spatial, B, below)
    tag = f"gdn c={c} s={spatial} B={B} {'IGDN' if inverse else 'GDN'}"
    r64 = L.gdn_ref(inp["x"], inp["beta"], inp["gamma"], inp["gy"], inverse, F64)
    r32 = L.gdn_ref(inp["x"], inp["beta"], inp["gamma"], inp["gy"], inverse, F32)
    x, beta, gamma, gy = dev(inp["x"]), dev(inp["beta"]), dev(inp["gamma"]), dev(inp["gy"])
    y = ops.gdn_fwd(x, beta, gamma, inverse)
    db = torch.full_like(beta, float("nan"))
    dg = torch.full_like(gamma, float("nan"))
    dx, db2, dg2 = ops.gdn_bwd(x, beta, gamma, gy, inverse, dbeta_out=db, dgamma_out=dg)
    torch.cuda.synchronize()
    assert db2.data_ptr() == db.data_ptr() and dg2.data_ptr() == dg.data_ptr()
    for t in (y, dx, db, dg):
        assert torch.isfinite(t).all(), tag
    ey, edx = float((y.cpu().double() - r64["y"]).abs().max()), L.max_rel(dx, r64["dx"])
    print(f"[{tag}] {what}: y {ey:.2e} abs | dx {edx:.2e} of max (bounds 1e-5)")
    assert ey < 1e-5 and edx < 1e-5
    check_sums(tag, {"dbeta": db, "dgamma": dg}, r64, r32, {"dbeta": 1e-4, "dgamma": 1e-4})
    assert torch.equal(db.cpu() == 0, r64["dbeta"] == 0)
    assert torch.equal(dg.cpu() == 0, r64["dgamma"] == 0)


# ---- 3. the latent tail above its tested sizes -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_inputs(c, B, below):
    return L.tail_inputs(c, B, below)


TAIL_FIGURES = {"dlat": 1e-4, "dsigma": 1e-4, "dmu": 1e-4, "dh": 1e-5, "dbeta": 1e-4, "dgamma": 1e-4, "dw": 2e-5,
                "db": 1e-5}


@pytest.mark.parametrize("mode", ["eval", "train_counter"])
@pytest.mark.parametrize("c,B,below", L.TAIL_CASES)
def test_latent_tail_against_the_float64_chain(ops, c, B, below, mode):
    """nvf_latent_tail_queue riding on a slab reduction (one real weight-gradient job and one bias-sum job as carrier,
    as in test_latent_tail_inside_the_slab_reduction_launch) past the rate's LDS path and over 2 .. 38 GDN chunks:
    every output against rate gradient -> GDN backward -> 1x1x1 weight / bias gradient in float64."""
    assert L.rate_path(c, B) == "loop"
    inp = _tail_inputs(c, B, below)
    kmode, u = L.rate_noise(inp, mode)
    g = L.TAIL_G_DEV * L.TAIL_G_HOST
    tag = f"tail c={c} B={B} {mode}"
    args = [inp[k] for k in ("x", "h", "e", "sigma", "mu", "beta", "gamma")]
    r64 = L.tail_chain(*args, kmode, u, g, inp["addend"], F64)
    r32 = L.tail_chain(*args, kmode, u, g, inp["addend"], F32)
    lat, h, e, sigma, mu, beta, gamma = [dev(t) for t in args]
    ids, dx0, g_dev = dev(inp["ids"]), dev(inp["addend"]), dev(torch.tensor([L.TAIL_G_DEV]))
    gp = L.gen(77)
    p, q = dev(torch.randn(2, 8, 16, 16, 16, generator=gp)), dev(torch.randn(2, 8, 19, 19, 19, generator=gp))
    dw_other_r = ops.wgrad(p, q, 4, 1, 0)
    ctx = ops.StepCtx()
    wb = ops.WgradBatch(torch.device("cuda"), ctx=ctx)
    nan = float("nan")
    dw_other, pb = torch.full_like(dw_other_r, nan), torch.full((8,), nan, device="cuda")
    wb.add(p, q, 4, 1, 0, 0, dw_other)
    out = {"dlat": torch.full_like(lat, nan), "dsigma": torch.full_like(sigma, nan), "dmu": torch.full_like(mu, nan),
           "dh": torch.full_like(h, nan), "dbeta": torch.full_like(beta, nan), "dgamma": torch.full_like(gamma, nan),
           "dw": torch.full((c, c, 1, 1, 1), nan, device="cuda"), "db": torch.full((c,), nan, device="cuda")}
    ops.latent_tail_queue(ctx, lat, sigma, mu, kmode, ids, dx0, out["dlat"], out["dsigma"], out["dmu"], g_dev,
                          L.TAIL_G_HOST, L.RATE_SEED, L.RATE_STEP, None, h, beta, gamma, out["dh"], out["dbeta"],
                          out["dgamma"], e, out["dw"], out["db"])
    wb.finish_with_sums([p], [pb])
    torch.cuda.synchronize()
    check_sums(tag, out, r64, r32, TAIL_FIGURES)
    assert torch.equal(out["dbeta"].cpu() == 0, r64["dbeta"] == 0)
    assert torch.equal(out["dgamma"].cpu() == 0, r64["dgamma"] == 0)
    # the carrier's own jobs came through
    assert torch.equal(dw_other, dw_other_r)
    assert L.max_rel(pb, p.double().sum(dim=(0, 2, 3, 4)).cpu()) < 1e-4


# ---- 4. the focal sums past their workgroup cap ------------------------------------------------------------------
BLOCK = 32 ** 3
FOCAL_TERMS = {"surf": (0.9, 1.0), "plain": (0.85, 0.0)}        # (alpha, beta); 'surf' is the distance-weighted term


def _focal_refs(p, gt, dist, alpha, beta):
    ref64, _, _ = focal_reference64(p, gt, dist, alpha, beta)
    ref32 = float(O.focal_dense(p, gt, alpha) if dist is None else O.surf_focal_dense(p, gt, dist, beta, alpha))
    return ref64, abs(ref32 - ref64) / abs(ref64)


@pytest.mark.parametrize("n", L.FOCAL_CASES)
def test_focal_loss_past_its_workgroup_cap(ops, n):
    """nvf_focal_loss adds workgroups up to 1024 (n = 64 blocks of 32^3) and grid-strides beyond."""
    p, gt, dist = L.focal_inputs(n)
    pd, gd, dd = dev(p), dev(gt), dev(dist)
    for name, (alpha, beta) in FOCAL_TERMS.items():
        ds, dsd = (dist, dd) if name == "surf" else (None, None)
        ref64, d32 = _focal_refs(p, gt, ds, alpha, beta)
        loss, dp = ops.focal_loss(pd, gd, dsd, alpha, beta=beta, want_grad=True)
        err = abs(float(loss) - ref64) / abs(ref64)
        print(L.fmt_row(f"focal n={n} grid-stride={L.focal_workgroups(n, 2048)[1]}", name, err, d32, 2e-5))
        assert err < L.bound(2e-5, d32)
        assert torch.isfinite(dp).all()
        for lo in range(0, n, 16 * BLOCK):
            hi = min(lo + 16 * BLOCK, n)
            _, dp_s = ops.focal_loss(pd[lo:hi], gd[lo:hi], None if dsd is None else dsd[lo:hi], alpha, beta=beta,
                                     want_grad=True)
            assert torch.equal(bits_of(dp_s), bits_of(dp[lo:hi])), (name, lo)


@pytest.mark.parametrize("blocks", L.FOCAL_MULTI_BLOCKS)
def test_focal_loss_multi_past_its_workgroup_cap(ops, blocks):
    """nvf_focal_loss_multi (one distance-weighted and one plain term) adds workgroups up to 1024 float4 groups of 256
    threads (32 blocks) and grid-strides beyond."""
    n = blocks * BLOCK
    p, gt, dist = L.focal_inputs(n)
    p2, gt2, _ = L.focal_inputs(n, seed_base=9800)
    pd, gd, dd, p2d, gt2d = dev(p), dev(gt), dev(dist), dev(p2), dev(gt2)
    out = torch.full((4,), float("nan"), device="cuda")
    (a1, b1), (a0, b0) = FOCAL_TERMS["surf"], FOCAL_TERMS["plain"]
    dps = ops.focal_loss_multi([(pd, gd, dd, a1, b1), (p2d, gt2d, None, a0, b0)], out, chain_sigmoid=False)
    torch.cuda.synchronize()
    for k, (name, args) in enumerate((("surf", (p, gt, dist, a1, b1)), ("plain", (p2, gt2, None, a0, b0)))):
        ref64, d32 = _focal_refs(*args)
        err = abs(float(out[k]) - ref64) / abs(ref64)
        print(L.fmt_row(f"focal_multi blocks={blocks} grid-stride={L.focal_workgroups(n, 1024)[1]}", name, err, d32, 2e-5))
        assert err < L.bound(2e-5, d32)
        assert torch.isfinite(dps[k]).all()
    for lo in range(0, n, 16 * BLOCK):
        hi = min(lo + 16 * BLOCK, n)
        out_s = torch.empty(4, device="cuda")
        dps_s = ops.focal_loss_multi([(pd[lo:hi], gd[lo:hi], dd[lo:hi], a1, b1), (p2d[lo:hi], gt2d[lo:hi], None, a0, b0)],
                                     out_s, chain_sigmoid=False)
        assert torch.equal(bits_of(dps_s[0]), bits_of(dps[0][lo:hi])), lo
        assert torch.equal(bits_of(dps_s[1]), bits_of(dps[1][lo:hi])), lo
