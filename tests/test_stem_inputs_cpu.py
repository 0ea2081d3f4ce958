"""The inputs and references of tests/test_gpu_stem.py, checked without a GPU: the kernels' switch points restated in
Python with every case-table entry landing on the pair of paths its comment names, the input conditions the device
tests rely on, and the float32 reference against the float64 one."""
import functools

import pytest
import torch

from oracle import nvf_oracle as O
from tests import latent_inputs as L
from tests import stem_inputs as S

F64, F32 = torch.float64, torch.float32
ALL_STEM = S.STEM_CASES + S.STEM_BWD_EDGES


@functools.lru_cache(maxsize=None)
def _refs(case):
    inp = S.stem_inputs(*case)
    return inp, S.stem_ref(inp, F64), S.stem_ref(inp, F32)


# ---- switch points ---------------------------------------------------------------------------------------------
def test_restated_constants():
    assert S.LATENT_FWD_SCRATCH == 1152 and S.STEM_SCRATCH == {8: 8000, 16: 16000}
    assert S.STEM_THREADS == {8: 512, 16: 1024} and S.STEM_MAX_SLABS == 256 and S.STEM_MAX_CH == 8
    # the stem's copy of the condition with the rate's scratch is the rate's own condition
    for c in range(1, 9):
        for B in (1, 16, 17, 46, 47, 128, 129):
            assert S.fwd_path(c, B, S.LATENT_FWD_SCRATCH) == L.rate_path(c, B)


def test_last_lds_batch_of_either_entry_point():
    """The issue's table: the last batch on the LDS path, by caller."""
    last = lambda c, scratch: max(B for B in range(1, 200) if S.fwd_path(c, B, scratch) == "lds")
    assert [last(8, S.LATENT_FWD_SCRATCH), last(8, S.STEM_SCRATCH[8])] == [16, 123]
    assert [last(8, S.LATENT_FWD_SCRATCH), last(8, S.STEM_SCRATCH[16])] == [16, 128]
    assert [last(3, S.LATENT_FWD_SCRATCH), last(3, S.STEM_SCRATCH[8])] == [46, 128]
    assert [last(5, S.LATENT_FWD_SCRATCH), last(1, S.LATENT_FWD_SCRATCH)] == [26, 128]
    assert 8 * (8 * 123 + 16) == S.STEM_SCRATCH[8]            # the narrow stem's scratch is filled to the last float


def test_latent_stem_cases_land_on_the_paths_they_name():
    cases = {(c0, c, B): (a, b) for c0, c, B, a, b in S.LATENT_STEM_CASES}
    assert len(cases) == len(S.LATENT_STEM_CASES) == 17
    for (c0, c, B), (a, b) in cases.items():
        assert S.fwd_path(c, B, S.LATENT_FWD_SCRATCH) == a, (c0, c, B)
        assert S.fwd_path(c, B, S.STEM_SCRATCH[c0]) == b, (c0, c, B)
        assert (a, b) != ("lds", "loop")                       # the stem's scratch is never the smaller one
    # nvf_latent_fwd's switch: a case on both sides for c = 8, 5, 3
    for c, last in ((8, 16), (5, 26), (3, 46)):
        assert cases[8, c, last] == ("lds", "lds") and cases[8, c, last + 1] == ("loop", "lds")
    # the narrow stem's own switch (its scratch decides): c = 8 only
    assert cases[8, 8, 123] == ("loop", "lds") and cases[8, 8, 124] == ("loop", "loop")
    assert 8 * 124 <= L.RATE_VT and 8 * (8 * 124 + L.RATE_NVW) > S.STEM_SCRATCH[8]
    # the nel <= 1024 clause: decides for the stem at c = 3 (narrow) and c = 8 (wide), for both entry points at c = 1
    assert cases[8, 3, 128] == ("loop", "lds") and cases[8, 3, 129] == ("loop", "loop")
    assert cases[16, 8, 128] == ("loop", "lds") and cases[16, 8, 129] == ("loop", "loop")
    assert cases[8, 1, 128] == ("lds", "lds") and cases[8, 1, 129] == ("loop", "loop")
    for c0, c in ((8, 3), (16, 8), (8, 1)):
        assert c * (8 * 129 + L.RATE_NVW) <= S.STEM_SCRATCH[c0] and 8 * 129 > L.RATE_VT
    # between the two switch points the entry points run different code: that is where most cases sit
    assert sum(1 for v in cases.values() if v == ("loop", "lds")) >= 8
    # the one equality test before these (5 blocks) had both on the LDS path
    for c0, c in ((8, 3), (16, 8)):
        assert S.fwd_path(c, 5, S.LATENT_FWD_SCRATCH) == S.fwd_path(c, 5, S.STEM_SCRATCH[c0]) == "lds"


def test_stem_case_tables():
    assert len(S.STEM_CASES) == 16
    for c0, c1 in (S.NARROW, S.WIDE):
        rows = [r for r in S.STEM_CASES if r[:2] == (c0, c1)]
        assert [r[2] for r in rows] == list(range(1, 9))
        assert [r[3] for r in rows] == [1, 5, 1, 5, 1, 5, 1, 5]
        assert [r[2] for r in rows if r[4]] == [2, 7]
    assert [r[:4] for r in S.STEM_BWD_EDGES] == [(8, 16, 5, 256), (8, 16, 5, 257), (16, 32, 2, 257), (8, 16, 8, 513)]
    assert S.bwd_blocks_per_workgroup(256) == (256, 1, 1)
    assert S.bwd_blocks_per_workgroup(257) == (256, 2, 1)      # workgroup 0 alone carries its sums over two blocks
    assert S.bwd_blocks_per_workgroup(513) == (256, 3, 2)
    assert all(S.bwd_blocks_per_workgroup(B)[1] == 1 for _, _, _, B, _ in S.STEM_CASES)
    assert max(B * c1 * 512 for _, c1, _, B, _ in ALL_STEM) == 257 * 32 * 512 < 4.3e6     # g1: 17 MB


# ---- input conditions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_STEM, ids=str)
def test_stem_inputs(case):
    c0, c1, ch, B, below = case
    inp = S.stem_inputs(*case)
    assert inp["x0"].shape == (B, ch, 2, 2, 2) and inp["w_up0"].shape == (ch, c0, 5, 5, 5)
    assert inp["w_conv0"].shape == (c0, c1, 5, 5, 5) and inp["g1"].shape == (B, c1, 8, 8, 8)
    assert torch.equal(inp["x0"], torch.round(inp["x0"])) and len(inp["x0"].unique()) >= 3
    assert bool((inp["beta"] < O.BETA_BOUND).any()) == below and bool((inp["gamma"] < O.GAMMA_BOUND).any()) == below


@pytest.mark.parametrize("case", [c for c in S.STEM_CASES if c[4]], ids=str)
def test_below_bound_entries_are_decided_away_from_rounding(case):
    """Every below-bound entry receives a summed gradient of at least 1e-3 of its tensor's largest, at least one of
    them is blocked (gradient >= 0: the step would lower the parameter further) and at least one passes; the reference's
    zero pattern is exactly the blocked entries."""
    inp, r64, _ = _refs(case)
    sums = S.igdn_param_sums64(inp)
    assert L.max_rel(sums["h0"], r64["h0"]) < 1e-12            # the restated IGDN is the oracle's
    assert float(inp["gamma"][2, 3]) < 0 and len(S.BELOW_ENTRIES) == 4
    blocked = []
    for name, idx in S.BELOW_ENTRIES:
        hat, bound = inp[name][idx], O.BETA_BOUND if name == "beta" else O.GAMMA_BOUND
        assert float(hat) < bound, (name, idx)
        s = float(sums[name][idx])
        assert abs(s) >= S.BELOW_MIN_SHARE * float(sums[name].abs().max()), (name, idx, s)
        blocked.append(s >= 0)
        assert (float(r64["d" + name][idx]) == 0.0) == (s >= 0), (name, idx)
    assert any(blocked) and not all(blocked), blocked
    zeros = int((r64["dbeta"] == 0).sum()) + int((r64["dgamma"] == 0).sum())
    assert zeros == sum(blocked)


@pytest.mark.parametrize("c0,c,B,p_lat,p_stem", S.LATENT_STEM_CASES)
def test_latent_inputs(c0, c, B, p_lat, p_stem):
    inp = S.latent_stem_inputs(c0, c, B)
    ids = inp["ids"].tolist()
    assert len(set(ids)) == B and ids != sorted(ids) and max(ids) >= B          # permuted, non-contiguous
    assert int((inp["sigma"] < 0).sum()) == 1
    assert inp["w_up0"].shape == (c, c0, 5, 5, 5) and inp["w_conv0"].shape == (c0, 2 * c0, 5, 5, 5)
    r64, r32 = S.latent_ref(inp, "eval", F64), S.latent_ref(inp, "eval", F32)
    xr = r64["x_rounded"]
    assert float(xr.abs().max()) >= 2 and len(xr.unique()) >= 3
    # no latent sits where float32 and float64 could round to different integers
    assert S.half_distance(r64["lat"]) > S.LATENT_HALF_MARGIN
    assert float((r32["lat"].double() - r64["lat"]).abs().max()) < 0.1 * S.LATENT_HALF_MARGIN
    assert torch.equal(r32["x_rounded"].double(), xr)
    for mode in S.LATENT_MODES:
        kmode, u = S.latent_noise_of(inp, mode)
        assert float(L.likelihood64(r64["lat"], inp["sigma"], inp["mu"], kmode, u).min()) > 5e-3, mode
    assert 0.0 <= float(inp["u_counter"].min()) and float(inp["u_counter"].max()) < 1.0


# ---- the references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_STEM, ids=str)
def test_float32_reference_is_near_the_float64_one(case):
    """The d32 of the tolerance rule is a float32 rounding distance, not a second algorithm."""
    _, r64, r32 = _refs(case)
    assert set(r64) == {"a0", "h0", "y1", "da0", "dx0", "dbeta", "dgamma", "dw_up0", "db_up0", "dw_conv0"}
    for k, ref in r64.items():
        assert ref.dtype == F64 and r32[k].dtype == F32 and float(ref.abs().max()) > 0, k
        assert L.max_rel(r32[k], ref) < 1e-4, (k, L.max_rel(r32[k], ref))
    assert torch.equal(r32["dbeta"] == 0, r64["dbeta"] == 0) and torch.equal(r32["dgamma"] == 0, r64["dgamma"] == 0)


@pytest.mark.parametrize("c0,c,B", [(8, 8, 17), (16, 3, 47), (8, 1, 129)])
def test_float32_latent_reference_is_near_the_float64_one(c0, c, B):
    inp = S.latent_stem_inputs(c0, c, B)
    for mode in S.LATENT_MODES:
        r64 = S.latent_stem_ref(inp, mode, F64)
        r32 = S.latent_stem_ref(inp, mode, F32, x0=r64["x_rounded"])
        for k in ("h", "lat", "bits", "a0", "h0", "y1"):
            assert L.max_rel(r32[k], r64[k]) < 1e-4, (mode, k)
        assert torch.equal(r32["x_rounded"].double(), r64["x_rounded"])


def test_db_up0_is_the_bias_gradient():
    """db_up0 = sum da0 is what autograd gives up0's bias."""
    inp = S.stem_inputs(8, 16, 3, 5, False)
    b = inp["b_up0"].double().requires_grad_(True)
    _, _, pre = S.stem_forward(inp["x0"].double(), inp["w_up0"].double(), b, inp["beta"].double(), inp["gamma"].double(),
                               inp["w_conv0"].double(), inp["b_conv0"].double())
    pre.backward(inp["g1"].double())
    assert L.max_rel(S.stem_ref(inp, F64)["db_up0"], b.grad) < 1e-12
