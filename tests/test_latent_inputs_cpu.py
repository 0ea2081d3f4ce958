"""The inputs and references of tests/test_gpu_latent_reductions.py, checked without a GPU: the input conditions the
device tests rely on, the float64 chain against plain autograd, and the kernels' switch points restated in Python with
every case-table entry landing on the path its comment names."""
import pytest
import torch

from oracle import nvf_oracle as O
from tests import latent_inputs as L


# ---- switch points ---------------------------------------------------------------------------------------------
def test_restated_constants():
    assert L.RATE_SCRATCH == 3 * 8 * (128 + 16) == 3456
    assert (L.RATE_VT, L.RATE_NVW) == (1024, 16)
    assert (L.GDN_THREADS, L.GDN_MAX_SLABS, L.LOSS_MAX_WG) == (128, 256, 1024)


def test_rate_cases_land_on_the_path_they_name():
    for c, B, path in L.RATE_CASES:
        assert L.rate_path(c, B) == path, (c, B)
    # each c of the table has its last LDS size and the first loop size next to it
    for c, last in ((8, 16), (3, 46), (1, 128)):
        assert L.rate_path(c, last) == "lds" and L.rate_path(c, last + 1) == "loop"
        assert (c, last, "lds") in L.RATE_CASES and (c, last + 1, "loop") in L.RATE_CASES
    # c = 1 is the only place the nel <= 1024 clause decides: the scratch alone would still take 129 blocks
    assert 3 * 1 * (129 * 8 + L.RATE_NVW) <= L.RATE_SCRATCH and 129 * 8 > L.RATE_VT
    assert 3 * 2 * (129 * 8 + L.RATE_NVW) > L.RATE_SCRATCH
    # 129 blocks: eight elements past one stride of the loop path
    assert 129 * 8 - L.RATE_VT == 8
    # a slice of the bit-for-bit comparison stays on the LDS path for every c, and so does every tested size of the
    # existing op-level tests
    for c in (1, 3, 8):
        assert L.rate_path(c, L.SLICE) == "lds"
    for c, B in ((3, 7), (8, 7), (3, 9), (8, 9), (3, 16), (8, 5), (3, 40)):
        assert L.rate_path(c, B) == "lds"
    # the tail's cases and the two added cases of test_latent_fwd_equals_the_three_kernels are past it
    for c, B, _ in L.TAIL_CASES:
        assert L.rate_path(c, B) == "loop"
    assert L.rate_path(8, 17) == "loop" and L.rate_path(3, 47) == "loop"


def test_gdn_cases_land_on_the_form_they_name():
    form = {(c, s, B): L.gdn_form(c, s, B) for c, s, B, _, _ in L.GDN_CASES}
    f = form[8, 8, 16]
    assert f["finishes_itself"] and f["nvox"] == 128
    f = form[8, 8, 17]
    assert (f["nslab"], f["last_live"], f["cg"]) == (2, 8, 8) and not f["finishes_itself"]
    f = form[3, 8, 47]
    assert (f["cg"], f["nslab"]) == (1, 3)
    assert form[12, 64, 3]["cg"] == 4 and form[12, 64, 3]["nslab"] == 2
    f = form[32, 64, 5]
    assert (f["cg"], 32 // f["cg"], f["own_slots"]) == (8, 4, 2)
    f = form[16, 64, 254]
    assert (f["nslab"], f["cg"], f["tiles"]) == (127, 8, 1) and f["nvox"] == 16256
    f = form[16, 64, 255]
    assert (f["nslab"], f["cg"], f["tiles"]) == (128, 1, 1)
    f = form[16, 64, 513]
    assert (f["per"], f["tiles"], f["cg"], f["nslab"]) == (256, 2, 1, 129) and f["nvox"] > 32768
    assert (f["last_live"], f["last_tiles"]) == (64, 1)          # the last workgroup's second tile is never walked
    f = form[32, 64, 600]
    assert (f["per"], f["tiles"], f["cg"], f["own_slots"]) == (256, 2, 1, 9)
    # all three kernel forms, both ends (one workgroup / gdn_bwd_final), the multi-tile loop
    assert {f["cg"] for f in form.values()} == {1, 4, 8}
    assert any(f["tiles"] > 1 for f in form.values()) and any(f["finishes_itself"] for f in form.values())
    # below-bound parameters reach gdn_bwd_final (more than one slab) in every case that has them
    for c, s, B, below, _ in L.GDN_CASES:
        if below:
            assert form[c, s, B]["nslab"] > 1 and c >= 4
    # the existing oracle test (B = 5 at 2^3 and 4^3) never left one tile per workgroup or met 128 slabs
    for c, s in ((3, 8), (8, 64), (16, 64), (8, 8), (4, 8)):
        f = L.gdn_form(c, s, 5)
        assert f["tiles"] == 1 and f["nslab"] <= 3


def test_tail_cases():
    for c, B, below in L.TAIL_CASES:
        assert c <= 8 and B * 8 > L.GDN_THREADS          # more than one 128-voxel chunk of gdn_bwd_one_workgroup
        assert not below or c == 8


def test_focal_cases_straddle_the_workgroup_cap():
    assert L.focal_workgroups(64 * 32768, 256 * 8) == (1024, False)
    assert L.focal_workgroups(65 * 32768, 256 * 8) == (1024, True)
    assert L.focal_workgroups(65 * 32768 + 3, 256 * 8) == (1024, True)
    assert L.focal_workgroups(32 * 32768, 256 * 4) == (1024, False)
    assert L.focal_workgroups(33 * 32768, 256 * 4) == (1024, True)
    assert L.FOCAL_CASES == [64 * 32768, 65 * 32768, 65 * 32768 + 3] and L.FOCAL_MULTI_BLOCKS == [32, 33]
    assert (65 * 32768 + 3) % 4 == 3                      # and not a multiple of a float4 group


# ---- input conditions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,B,path", L.RATE_CASES)
def test_rate_inputs_are_bulk(c, B, path):
    inp = L.rate_inputs(c, B)
    assert int((inp["sigma"] < 0).sum()) == 1 and 0.6 <= float(inp["sigma"].abs().min()) <= float(inp["sigma"].abs().max()) <= 1.4
    ids = inp["ids"].tolist()
    assert len(set(ids)) == B and (B == 1 or ids != sorted(ids)) and max(ids) >= B        # permuted, non-contiguous
    for mode in L.RATE_MODES:
        kmode, u = L.rate_noise(inp, mode)
        assert float(L.likelihood64(inp["x"], inp["sigma"], inp["mu"], kmode, u).min()) > 5e-3, mode
    assert not torch.equal(inp["u"], inp["u_counter"])
    assert 0.0 <= float(inp["u_counter"].min()) and float(inp["u_counter"].max()) < 1.0


@pytest.mark.parametrize("c,B,below", L.TAIL_CASES)
def test_tail_inputs_are_bulk_and_normed(c, B, below):
    inp = L.tail_inputs(c, B, below)
    for mode in ("eval", "train_counter"):
        kmode, u = L.rate_noise(inp, mode)
        assert float(L.likelihood64(inp["x"], inp["sigma"], inp["mu"], kmode, u).min()) > 5e-3, mode
    assert float(L.gdn_norm64(inp["h"], inp["beta"], inp["gamma"]).min()) > L.GDN_MIN_NORM
    assert bool((inp["beta"] < O.BETA_BOUND).any()) == below and bool((inp["gamma"] < O.GAMMA_BOUND).any()) == below


@pytest.mark.parametrize("c,spatial,B,below,what", L.GDN_CASES)
def test_gdn_norms_are_bounded_away_from_zero(c, spatial, B, below, what):
    inp = L.gdn_inputs(c, spatial, B, below)
    assert inp["x"].numel() <= 1_300_000
    nrm = L.gdn_norm64(inp["x"], inp["beta"], inp["gamma"])
    assert float(nrm.min()) > L.GDN_MIN_NORM, float(nrm.min())
    assert bool((inp["beta"] < O.BETA_BOUND).any()) == below and bool((inp["gamma"] < O.GAMMA_BOUND).any()) == below


# ---- the references ----------------------------------------------------------------------------------------------
def test_float64_chain_equals_plain_autograd():
    """tail_chain hands each stage's gradient to the next by hand; one autograd graph over conv -> GDN -> rate must give
    the same numbers (float64: to rounding)."""
    c, B = 8, 5
    inp = L.tail_inputs(c, B, True)
    g = L.gen(1)
    w = (0.5 * torch.randn(c, c, 1, 1, 1, generator=g)).double().requires_grad_(True)
    b = (0.1 * torch.randn(c, generator=g)).double().requires_grad_(True)
    e = inp["e"].double()
    beta, gamma = inp["beta"].double().requires_grad_(True), inp["gamma"].double().requires_grad_(True)
    sigma = inp["sigma"].double().view(1, c, 1, 1, 1).requires_grad_(True)
    mu = inp["mu"].double().view(1, c, 1, 1, 1).requires_grad_(True)
    gfac = L.TAIL_G_DEV * L.TAIL_G_HOST
    for mode in ("eval", "train_counter"):
        kmode, u = L.rate_noise(inp, mode)
        for t in (w, b, beta, gamma, sigma, mu):
            t.grad = None
        h = torch.nn.functional.conv3d(e, w, b)
        h.retain_grad()
        lat = O.gdn3d(h, beta, gamma, False)
        lat.retain_grad()
        _, bits = O.entropy_coder({"entropy_coder.sigma": sigma, "entropy_coder.mu": mu}, lat, kmode, u.double())
        (gfac * bits + (inp["addend"].double() * lat).sum()).backward()
        ch = L.tail_chain(lat.detach(), h.detach(), e, sigma.detach().reshape(-1), mu.detach().reshape(-1),
                          beta.detach(), gamma.detach(), kmode, u, gfac, inp["addend"], torch.float64)
        for name, ref in (("dlat", lat.grad), ("dsigma", sigma.grad), ("dmu", mu.grad), ("dh", h.grad),
                          ("dbeta", beta.grad), ("dgamma", gamma.grad), ("dw", w.grad), ("db", b.grad)):
            assert L.max_rel(ch[name], ref) < 1e-12, (mode, name)
            assert float(ref.abs().max()) > 0
        assert torch.equal(ch["dbeta"] == 0, beta.grad == 0) and torch.equal(ch["dgamma"] == 0, gamma.grad == 0)


def test_float32_oracle_is_near_the_float64_one():
    """The d32 of the tolerance rule is a float32 rounding distance, not a second algorithm: on a small case it is far
    below the suite's figures."""
    inp = L.rate_inputs(8, 17)
    r64 = L.rate_ref(inp["x"], inp["sigma"], inp["mu"], "train", inp["u"], 0.37, inp["addend"], torch.float64)
    r32 = L.rate_ref(inp["x"], inp["sigma"], inp["mu"], "train", inp["u"], 0.37, inp["addend"], torch.float32)
    assert r32["dx"].dtype == torch.float32 and r64["dx"].dtype == torch.float64
    assert torch.equal(r32["rounded"].double(), r64["rounded"])
    assert abs(float(r32["bits"]) - float(r64["bits"])) < 1e-5 * float(r64["bits"])
    for k in ("dx", "dsigma", "dmu"):
        assert L.max_rel(r32[k], r64[k]) < 1e-4, k
    assert L.bound(1e-4, 1e-6) == 1e-4 and L.bound(1e-4, 1e-3) == 3e-3


def test_focal_inputs():
    p, gt, dist = L.focal_inputs(4099)
    assert p.dtype == torch.float32 and 0.02 <= float(p.min()) and float(p.max()) <= 0.98
    assert 0.2 < float(gt.mean()) < 0.3 and set(gt.unique().tolist()) == {0.0, 1.0}
