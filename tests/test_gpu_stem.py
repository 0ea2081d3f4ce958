"""The fused stem at the C ABI -- nvf_stem_fwd, nvf_stem_latent_fwd, nvf_stem_bwd, nvf_stem_bwd_partial through
nvfpcc_amd.ops -- held to float64 at every latent width ch = 1 .. 8 of both tuned decoders, on both sides of the latent
workgroup's path switch (which moves with the entry point) and past stem_bwd_kernel's cap of 256 workgroups.

The reference is torch's conv_transpose3d and the oracle's gdn3d / latent_gen / entropy_coder in float64 with autograd on
the CPU (tests/stem_inputs.py); it uses no kernel of this project.  tests/test_stem_inputs_cpu.py proves without a GPU
that every case lands on the path its comment names and that the inputs meet the conditions the comparisons rely on.

Bounds: err < max(t, 3 * d32), err and d32 as max |difference| / max |float64 reference|, d32 the float32 CPU reference's
own distance from float64 on the same inputs; t = 1e-5 for a0, h0, y1, da0, dx0 (and h, lat, bits of the latent front),
1e-4 for the parameter gradients -- the figures at the top of tests/test_gpu_ops.py.  Every row is printed.
Measured: profiles/stem_parity.md."""
import ctypes
import functools

import pytest
import torch

from tests import latent_inputs as L
from tests import stem_inputs as S

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
ACT = {"a0": 1e-5, "h0": 1e-5, "y1": 1e-5}
BWD_DATA = {"da0": 1e-5, "dx0": 1e-5}
BWD_PARAMS = {"dbeta": 1e-4, "dgamma": 1e-4, "dw_up0": 1e-4}
ALL_BWD = S.STEM_CASES + S.STEM_BWD_EDGES


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


def same_bits(a, b):
    return torch.equal(bits_of(a), bits_of(b))


def check_rows(tag, got, r64, r32, figures):
    """figures: name -> t.  Prints every row, then asserts the rule on each."""
    rows = []
    for name, t in figures.items():
        err, d32 = L.max_rel(got[name], r64[name]), L.max_rel(r32[name], r64[name])
        print(L.fmt_row(tag, name, err, d32, t))
        rows.append((name, err, L.bound(t, d32)))
    for name, err, b in rows:
        assert torch.isfinite(got[name]).all(), (tag, name)
        assert err < b, (tag, name, err, b)


# ---- inputs and references: computed once, shared, never written to -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_case(case):
    inp = S.stem_inputs(*case)
    return inp, S.stem_ref(inp, F64), S.stem_ref(inp, F32)


@functools.lru_cache(maxsize=None)
def _latent_case(c0, c, B):
    inp = S.latent_stem_inputs(c0, c, B)
    refs = {}
    for mode in S.LATENT_MODES:
        r64 = S.latent_stem_ref(inp, mode, F64)
        refs[mode] = (r64, S.latent_stem_ref(inp, mode, F32, x0=r64["x_rounded"]))
    return inp, refs


def _weights(ops, inp):
    """The layouts the kernels take: up0 / conv0 forward [ci][125][co] and backward [co][125][ci], biases, IGDN."""
    w0f, w0b = ops.pack_convT_weight(dev(inp["w_up0"]))
    w1f, w1b = ops.pack_convT_weight(dev(inp["w_conv0"]))
    return {"w0f": w0f, "w0b": w0b, "w1f": w1f, "w1b": w1b, "b0": dev(inp["b_up0"]), "b1": dev(inp["b_conv0"]),
            "beta": dev(inp["beta"]), "gamma": dev(inp["gamma"])}


def _stem_fwd(ops, w, x0):
    return ops.stem_fwd(x0, w["w0f"], w["b0"], w["beta"], w["gamma"], w["w1f"], w["b1"])


def _tag(case):
    c0, c1, ch, B, below = case
    return f"stem {c0},{c1} ch={ch} B={B}" + (" below" if below else "")


# ---- a, b: the forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.STEM_CASES, ids=_tag)
def test_stem_forward_against_float64(ops, case):
    """ops.stem_fwd at every ch = 1 .. 8 of both decoders: a0, h0, y1 against float64.  For the narrow decoder also
    against the per-layer kernels (convT k5 s2 pad 2 -> IGDN -> convT + ReLU), whose bits stem.hip's top comment claims."""
    c0, c1, ch, B, below = case
    inp, r64, r32 = _stem_case(case)
    w, x0 = _weights(ops, inp), dev(inp["x0"])
    a0, h0, y1 = _stem_fwd(ops, w, x0)
    torch.cuda.synchronize()
    check_rows(_tag(case) + " fwd", {"a0": a0, "h0": h0, "y1": y1}, r64, r32, ACT)
    if (c0, c1) == S.NARROW:
        a0_l = ops.convT3d_k5s2_fwd(x0, w["w0f"], w["b0"], c0, 2, ops.ACT_NONE)
        h0_l = ops.gdn_fwd(a0_l, w["beta"], w["gamma"], True)
        y1_l = ops.convT3d_k5s2_fwd(h0_l, w["w1f"], w["b1"], c1, 2, ops.ACT_RELU)
        assert same_bits(a0, a0_l) and same_bits(h0, h0_l) and same_bits(y1, y1_l), _tag(case)


# ---- c: the latent front in the same launch --------------------------------------------------------------------------
LATENT_FIGURES = dict(h=1e-5, lat=1e-5, bits=1e-5, **ACT)


@pytest.mark.parametrize("mode", S.LATENT_MODES)
@pytest.mark.parametrize("c0,c,B,p_lat,p_stem", S.LATENT_STEM_CASES)
def test_latent_front_and_stem_in_one_launch(ops, c0, c, B, p_lat, p_stem, mode):
    """ops.stem_latent_fwd against ops.latent_fwd then ops.stem_fwd, bit for bit in all seven outputs, on both sides of
    either entry point's path switch (LATENT_STEM_CASES: between the two switches the latent workgroups run different
    code at different block sizes); eval and train with the counter noise of permuted, non-contiguous block ids; against
    float64; and block by block against batch-1 calls."""
    assert S.fwd_path(c, B, S.LATENT_FWD_SCRATCH) == p_lat and S.fwd_path(c, B, S.STEM_SCRATCH[c0]) == p_stem
    inp, refs = _latent_case(c0, c, B)
    r64, r32 = refs[mode]
    kmode, _ = S.latent_noise_of(inp, mode)
    tag = f"latent+stem {c0},{2 * c0} c={c} B={B} {p_lat}/{p_stem} {mode}"
    w = _weights(ops, inp)
    e, ids = dev(inp["e"]), dev(inp["ids"])
    lw, _ = ops.pack_conv_weight(dev(inp["lat_w"]))
    lat_args = (lw, dev(inp["lat_b"]), dev(inp["lat_beta"]), dev(inp["lat_gamma"]), dev(inp["sigma"]), dev(inp["mu"]), kmode)
    stem_args = (w["w0f"], w["b0"], w["beta"], w["gamma"], w["w1f"], w["b1"])
    noise = dict(seed=S.NOISE_SEED, step=S.NOISE_STEP)
    names = ("h", "lat", "x_rounded", "bits", "a0", "h0", "y1")
    one = dict(zip(names, ops.stem_latent_fwd(e, *lat_args, *stem_args, block_ids=ids, **noise)))
    two = dict(zip(names[:4], ops.latent_fwd(e, *lat_args, block_ids=ids, **noise)))
    two.update(zip(names[4:], _stem_fwd(ops, w, two["x_rounded"])))
    torch.cuda.synchronize()
    # against float64 first: a difference between the two entry points is then known to be one of rounding
    assert torch.equal(one["x_rounded"].cpu().double(), r64["x_rounded"]), tag
    check_rows(tag, one, r64, r32, LATENT_FIGURES)
    differ = [k for k in names if not same_bits(one[k], two[k])]
    assert not differ, (tag, differ, float(one["bits"]), float(two["bits"]))
    # batch invariance: block i of this call is a batch-1 call on that block
    alone = [ops.stem_latent_fwd(e[i:i + 1], *lat_args, *stem_args, block_ids=ids[i:i + 1], **noise) for i in range(B)]
    for k in ("x_rounded", "a0", "h0", "y1"):
        got = torch.cat([r[names.index(k)] for r in alone])
        assert same_bits(got, one[k]), (tag, k)


# ---- d: the backward -------------------------------------------------------------------------------------------------
def _stem_bwd(ops, w, g1, x0, a0, want_w, ch, c0):
    if not want_w:
        return (*ops.stem_bwd(g1, x0, a0, w["w1b"], w["w0b"], w["beta"], w["gamma"]), None, None, None)
    nan = float("nan")
    db, dg = torch.full_like(w["beta"], nan), torch.full_like(w["gamma"], nan)
    dw = torch.full((ch, c0, 5, 5, 5), nan, device="cuda")
    da0, dx0 = ops.stem_bwd(g1, x0, a0, w["w1b"], w["w0b"], w["beta"], w["gamma"], dbeta_out=db, dgamma_out=dg, dw_up0=dw)
    return da0, dx0, db, dg, dw


@pytest.mark.parametrize("case", ALL_BWD, ids=_tag)
def test_stem_backward_against_float64(ops, case):
    """ops.stem_bwd from g1 = dL/d(conv0's pre-activation): da0, dx0 and the three parameter gradients against float64;
    without the parameter outputs the same bits of da0 / dx0; the LowerBound rule's zero pattern exactly.  Past 256 blocks
    (a workgroup walks several and carries its sums) also against the sum of two disjoint sub-batch calls."""
    c0, c1, ch, B, below = case
    inp, r64, r32 = _stem_case(case)
    w, x0, g1 = _weights(ops, inp), dev(inp["x0"]), dev(inp["g1"])
    a0, _, _ = _stem_fwd(ops, w, x0)
    da0, dx0, db, dg, dw = _stem_bwd(ops, w, g1, x0, a0, True, ch, c0)
    da0_n, dx0_n, _, _, _ = _stem_bwd(ops, w, g1, x0, a0, False, ch, c0)
    torch.cuda.synchronize()
    got = {"da0": da0, "dx0": dx0, "dbeta": db, "dgamma": dg, "dw_up0": dw}
    check_rows(_tag(case) + " bwd", got, r64, r32, {**BWD_DATA, **BWD_PARAMS})
    assert same_bits(da0_n, da0) and same_bits(dx0_n, dx0)
    assert torch.equal(db.cpu() == 0, r64["dbeta"] == 0) and torch.equal(dg.cpu() == 0, r64["dgamma"] == 0)
    assert below == bool((r64["dbeta"] == 0).any() or (r64["dgamma"] == 0).any())
    if B > S.STEM_MAX_SLABS:
        k = B // 2 + 1
        parts = [_stem_bwd(ops, w, g1[lo:hi], x0[lo:hi], a0[lo:hi], True, ch, c0) for lo, hi in ((0, k), (k, B))]
        torch.cuda.synchronize()
        split = {"da0": torch.cat([p[0] for p in parts]), "dx0": torch.cat([p[1] for p in parts]),
                 "dbeta": parts[0][2] + parts[1][2], "dgamma": parts[0][3] + parts[1][3], "dw_up0": parts[0][4] + parts[1][4]}
        for name in got:
            err = L.max_rel(got[name], split[name].cpu().double())
            print(f"[{_tag(case)} bwd] {name}: {err:.2e} from the sum of two sub-batch calls (bound 2e-6)")
            assert err < 2e-6, (name, err)


# ---- e: the backward whose finals are shared ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["deferred", "deferred+conv0", "immediate"])
@pytest.mark.parametrize("case", ALL_BWD, ids=_tag)
def test_stem_backward_partial_through_the_slab_reduction(ops, case, form):
    """ops.stem_bwd_partial: up0's weight-gradient slabs as a job of a WgradBatch, the IGDN parameter gradients as a
    deferred final pass of a step context (or, without a context, launched at once).  After the reduction and the flush:
    the bits of nvf_stem_bwd ("Same sums, same order").  With h0 / dw_conv0: conv0's weight gradient against float64, and
    against ops.wgrad on the same tensors to rounding."""
    c0, c1, ch, B, below = case
    with_conv0, deferred = form == "deferred+conv0", form != "immediate"
    inp, r64, r32 = _stem_case(case)
    w, x0, g1 = _weights(ops, inp), dev(inp["x0"]), dev(inp["g1"])
    a0, h0, _ = _stem_fwd(ops, w, x0)
    da0, dx0, db, dg, dw = _stem_bwd(ops, w, g1, x0, a0, True, ch, c0)
    nan = float("nan")
    db_p, dg_p, dw_p = torch.full_like(db, nan), torch.full_like(dg, nan), torch.full_like(dw, nan)
    dw1 = torch.full((c0, c1, 5, 5, 5), nan, device="cuda") if with_conv0 else None
    ctx = ops.StepCtx() if deferred else None
    wb = ops.WgradBatch(torch.device("cuda"), nbytes=1 << 20, ctx=ctx)
    if deferred:
        ctx.begin()
    da0_p, dx0_p = ops.stem_bwd_partial(g1, x0, a0, w["w1b"], w["w0b"], w["beta"], w["gamma"], db_p, dg_p, dw_p, wb, ctx=ctx,
                                        h0=h0 if with_conv0 else None, dw_conv0=dw1)
    assert len(wb.jobs) == (2 if with_conv0 else 1) and wb.jobs[0][2] == min(B, S.STEM_MAX_SLABS)
    wb.finish()
    if deferred:
        ctx.flush()
    torch.cuda.synchronize()
    for name, a, b in (("da0", da0_p, da0), ("dx0", dx0_p, dx0), ("dbeta", db_p, db), ("dgamma", dg_p, dg), ("dw_up0", dw_p, dw)):
        assert same_bits(a, b), (_tag(case), name)
    if with_conv0:
        check_rows(_tag(case) + " partial", {"dw_conv0": dw1}, r64, r32, {"dw_conv0": 1e-4})
        err = L.max_rel(dw1, ops.wgrad(h0, g1, 5, 2, 2).cpu().double())
        print(f"[{_tag(case)} partial] dw_conv0: {err:.2e} from ops.wgrad (bound 2e-5)")
        assert err < 2e-5


# ---- f: refusals -------------------------------------------------------------------------------------------------------
def _raw_buffers(B, ch, c0, c1):
    """Device buffers large enough for any accepted shape near (B, ch, c0, c1): inputs of ones, outputs of NaN."""
    n_in = max(B * 16 * 512 * 2, 16 * 125 * 32)
    ones = torch.ones(n_in, device="cuda")
    outs = [torch.full((B * 32 * 512,), float("nan"), device="cuda") for _ in range(7)]
    return ones, outs


@pytest.mark.parametrize("ch,c0,c1", [(0, 8, 16), (9, 8, 16), (9, 16, 32), (3, 8, 8), (3, 16, 16), (3, 4, 8)])
def test_stem_entry_points_refuse_other_shapes(ops, ch, c0, c1):
    """ch outside 1 .. 8 and channel pairs other than (8, 16) / (16, 32): NVF_EINVAL from all four entry points, and no
    output is touched (the ops wrappers raise on it: there is no fall-back)."""
    from nvfpcc_amd._lib import lib, CONSTANTS, NvfError
    h, B = lib(), 3
    ones, outs = _raw_buffers(B, ch, c0, c1)
    p, o = ones.data_ptr(), [t.data_ptr() for t in outs]
    ws = torch.full((max(int(h.nvf_stem_bwd_workspace_for(B, 8, 16, 32)), 4) // 4,), float("nan"), device="cuda")
    ids = torch.arange(B, device="cuda")
    slabs, nsl = ctypes.c_void_p(), ctypes.c_int(-1)
    rc = {"nvf_stem_fwd": h.nvf_stem_fwd(p, p, p, p, p, p, p, o[0], o[1], o[2], B, ch, c0, c1, None),
          "nvf_stem_latent_fwd": h.nvf_stem_latent_fwd(p, p, p, p, p, ids.data_ptr(), p, p, o[0], o[1], o[2], o[3], 1, 0, 0,
                                                       None, p, p, p, p, p, p, o[4], o[5], o[6], B, ch, c0, c1, None),
          "nvf_stem_bwd": h.nvf_stem_bwd(p, p, p, p, p, p, p, o[0], o[1], o[2], o[3], o[4], ws.data_ptr(), ws.numel() * 4,
                                         B, ch, c0, c1, None),
          "nvf_stem_bwd_partial": h.nvf_stem_bwd_partial(p, p, p, p, p, p, p, o[0], o[1], o[2], o[3], ctypes.byref(slabs),
                                                         ctypes.byref(nsl), ws.data_ptr(), ws.numel() * 4, B, ch, c0, c1,
                                                         None, None, None, None)}
    torch.cuda.synchronize()
    assert rc == dict.fromkeys(rc, CONSTANTS["NVF_EINVAL"]), rc
    assert all(torch.isnan(t).all() for t in outs) and torch.isnan(ws).all()
    assert slabs.value is None and nsl.value == -1
    if ch > 0:
        x0 = torch.zeros(B, ch, 2, 2, 2, device="cuda")
        with pytest.raises(NvfError, match="NVF_EINVAL"):
            ops.stem_fwd(x0, ones, ones[:c0], ones[:c0], ones[:c0 * c0], ones, ones[:c1])


@pytest.mark.parametrize("ch,c0,c1", [(1, 8, 16), (8, 8, 16), (5, 16, 32)])
def test_stem_backward_refuses_a_workspace_one_float_short(ops, ch, c0, c1):
    """nvf_stem_bwd / nvf_stem_bwd_partial with one float less than nvf_stem_bwd_workspace_for states: NVF_EWORKSPACE,
    nothing written; with exactly that size they run."""
    from nvfpcc_amd._lib import lib, CONSTANTS
    h, B = lib(), 3
    case = (c0, c1, ch, B, False)
    inp = S.stem_inputs(*case)
    w, x0, g1 = _weights(ops, inp), dev(inp["x0"]), dev(inp["g1"])
    a0, _, _ = _stem_fwd(ops, w, x0)
    need = int(h.nvf_stem_bwd_workspace_for(B, ch, c0, c1))
    assert need > 0 and need % 4 == 0
    nan = float("nan")
    ws = torch.full((need // 4,), nan, device="cuda")
    outs = [torch.full_like(a0, nan), torch.full_like(x0, nan), torch.full_like(w["beta"], nan),
            torch.full_like(w["gamma"], nan), torch.full((ch, c0, 5, 5, 5), nan, device="cuda")]
    ins = [t.data_ptr() for t in (g1, x0, a0, w["w1b"], w["w0b"], w["beta"], w["gamma"])]
    o = [t.data_ptr() for t in outs]
    slabs, nsl = ctypes.c_void_p(), ctypes.c_int(-1)
    rc = [h.nvf_stem_bwd(*ins, *o, ws.data_ptr(), need - 4, B, ch, c0, c1, None),
          h.nvf_stem_bwd_partial(*ins, *o[:4], ctypes.byref(slabs), ctypes.byref(nsl), ws.data_ptr(), need - 4, B, ch, c0, c1,
                                 None, None, None, None)]
    torch.cuda.synchronize()
    assert rc == [CONSTANTS["NVF_EWORKSPACE"]] * 2, rc
    assert all(torch.isnan(t).all() for t in outs) and torch.isnan(ws).all() and slabs.value is None and nsl.value == -1
    assert h.nvf_stem_bwd(*ins, *o, ws.data_ptr(), need, B, ch, c0, c1, None) == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in outs)
    da0, dx0, db, dg, dw = _stem_bwd(ops, w, g1, x0, a0, True, ch, c0)
    for a, b in zip(outs, (da0, dx0, db, dg, dw)):
        assert same_bits(a, b)
