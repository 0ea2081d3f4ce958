"""Case tables, inputs and float64 references of the fused stem (tests/test_gpu_stem.py on the device,
tests/test_stem_inputs_cpu.py without one): up0 -> IGDN -> conv0 + ReLU forward and backward at every latent width
ch = 1 .. 8 of both tuned decoders, and the latent generator + quantiser in front of it.

Everything here is torch on the CPU plus the oracle (oracle/nvf_oracle.py: gdn3d, latent_gen, entropy_coder); no kernel
of this project.  The switch points of the kernels are restated in Python so that the CPU test can prove that every
entry of a case table lands on the code path its comment names:

    latent_fwd_body (csrc/latent_tail.h)    LDS path iff  nel = 8 B <= 1024  and  c (nel + 16) <= scratch_floats, with
        nvf_latent_fwd (csrc/pointwise.hip)        scratch_floats = kTailRateLds / 3 = 1152, 1024 threads
        nvf_stem_latent_fwd (csrc/stem_fwd.h)      scratch_floats = 8 * 125 * C0: 8000 (narrow, 512 threads) or
                                                   16000 (wide, 1024 threads) -- up0's weight region of the LDS
    stem_bwd_kernel (csrc/stem.hip)         min(B, kStemMaxSlabs = 256) workgroups; from B = 257 a workgroup walks blocks
                                            wg, wg + 256, ... and carries own_gdn / own_w across them

Tolerance rule (tests/latent_inputs.py): err < max(t, 3 * d32), t the suite's figure for the quantity, d32 the distance
of the float32 CPU reference from the float64 one on the same inputs -- never a number of the device.
"""
import torch
import torch.nn.functional as F

from oracle import nvf_oracle as O
from tests import latent_inputs as L
from tests.philox_np import latent_noise

# ---- the switch points, restated -------------------------------------------------------------------------------
LATENT_FWD_SCRATCH = L.RATE_SCRATCH // 3                 # nvf_latent_fwd: kTailRateLds / 3
STEM_MAX_CH = 8                                          # MAXCH / kStemFwdMaxCh / kStemMaxCh
STEM_SCRATCH = {8: STEM_MAX_CH * 125 * 8, 16: STEM_MAX_CH * 125 * 16}    # nvf_stem_latent_fwd, by c0
STEM_THREADS = {8: 512, 16: 1024}                        # C0 * 64
STEM_MAX_SLABS = 256                                     # kStemMaxSlabs


def fwd_path(c, B, scratch_floats):
    """'lds' or 'loop': the branch of latent_fwd_body for c latent channels and B blocks of 2^3 latents, given the
    scratch its caller hands it (see rate_path in tests/latent_inputs.py for the rate's own copy of the condition)."""
    nel = 8 * B
    return "lds" if nel <= L.RATE_VT and c * (nel + L.RATE_NVW) <= scratch_floats else "loop"


def bwd_blocks_per_workgroup(B):
    """(workgroups of stem_bwd_kernel, most blocks one of them walks, fewest)."""
    nwg = min(B, STEM_MAX_SLABS)
    return nwg, -(-B // nwg), B // nwg


# ---- case tables -------------------------------------------------------------------------------------------------
NARROW, WIDE = (8, 16), (16, 32)
# (c0, c1, ch, B, below-bound IGDN parameters): every latent width of both decoders, B alternating 1 and 5
STEM_CASES = [(c0, c1, ch, 1 if ch % 2 else 5, ch in (2, 7)) for c0, c1 in (NARROW, WIDE) for ch in range(1, 9)]
# backward only, around stem_bwd_kernel's cap of 256 workgroups
STEM_BWD_EDGES = [
    (8, 16, 5, 256, False),      # the last batch with one block per workgroup
    (8, 16, 5, 257, False),      # workgroup 0 walks blocks 0 and 256, the other 255 one block
    (16, 32, 2, 257, False),     # the same with the wide decoder's 1024 threads
    (8, 16, 8, 513, False),      # workgroup 0 walks three blocks, the others two; the largest tensor of the suite's stem tests
]
# (c0, c, B, path of nvf_latent_fwd, path of nvf_stem_latent_fwd's latent workgroup)
LATENT_STEM_CASES = [
    (8, 8, 16, "lds", "lds"),      # the last batch nvf_latent_fwd keeps in its scratch at c = 8
    (8, 8, 17, "loop", "lds"),     # one past it: the two entry points run different code from here ...
    (8, 8, 123, "loop", "lds"),    # ... to here: 8 * (984 + 16) = 8000 floats, the narrow stem's scratch exactly
    (8, 8, 124, "loop", "loop"),   # one past the narrow stem's switch
    (8, 8, 129, "loop", "loop"),   # nel 1032: eight elements past one 1024 stride
    (8, 5, 26, "lds", "lds"),      # c = 5: 5 * (208 + 16) = 1120 <= 1152
    (8, 5, 27, "loop", "lds"),     # 5 * (216 + 16) = 1160
    (8, 3, 46, "lds", "lds"),      # c = 3: 3 * 384 = 1152
    (8, 3, 47, "loop", "lds"),
    (8, 3, 128, "loop", "lds"),    # nel 1024: the stem's scratch would hold more, the nel <= 1024 clause decides
    (8, 3, 129, "loop", "loop"),
    (8, 1, 128, "lds", "lds"),     # c = 1: the nel <= 1024 clause decides for both entry points
    (8, 1, 129, "loop", "loop"),
    (16, 8, 17, "loop", "lds"),    # wide: 16000 floats of scratch, 1024 threads
    (16, 8, 128, "loop", "lds"),   # its last LDS batch is set by nel <= 1024, not by the scratch
    (16, 8, 129, "loop", "loop"),
    (16, 3, 47, "loop", "lds"),
]
LATENT_MODES = ["eval", "train_counter"]
NOISE_SEED, NOISE_STEP = L.RATE_SEED, L.RATE_STEP

# below-bound IGDN entries of a `below` case: (tensor, index); gamma[4, 4] is the diagonal one, gamma[2, 3] is negative
BELOW_ENTRIES = [("beta", (0,)), ("gamma", (0, 1)), ("gamma", (2, 3)), ("gamma", (4, 4))]
BELOW_MIN_SHARE = 1e-3       # |summed gradient at a below-bound entry| / max over its tensor, at least

# Seeds.  A case's generator is seeded from its shape; the entries below move a case to the next seed that meets the
# input conditions tests/test_stem_inputs_cpu.py asserts (below-bound entries: gradients away from zero, one blocked and
# one passed; latents: no value within LATENT_HALF_MARGIN of a rounding boundary).  Conditions on inputs only: they are
# evaluated with the float64 reference.
STEM_SEED_BUMP = {}
LATENT_SEED_BUMP = {(8, 8, 123): 1, (8, 8, 124): 1, (16, 8, 17): 1, (16, 8, 129): 1}
LATENT_HALF_MARGIN = 2e-5    # float32 latents are ~1e-6 from the float64 ones: rintf() then agrees with round()


def _convT_weight(cin, cout, g):
    """[cin, cout, 5, 5, 5] scaled by fan_in ** -0.5, fan_in = cin * 125 / 8: at stride 2 an output sees one tap in eight."""
    return torch.randn(cin, cout, 5, 5, 5, generator=g) * (cin * 125 / 8) ** -0.5


def igdn_params(c0, g, below):
    """beta_hat / gamma_hat of test_gdn_forward_backward (tests/latent_inputs.gdn_params); ``below`` adds the diagonal
    entry to its three below-bound ones (BELOW_ENTRIES)."""
    beta, gamma = L.gdn_params(c0, g, below)
    if below:
        gamma[4, 4] = 1e-7
    return beta, gamma


def stem_weights(c0, c1, ch, g, below):
    w0, b0 = _convT_weight(ch, c0, g), 0.1 * torch.randn(c0, generator=g)
    beta, gamma = igdn_params(c0, g, below)
    w1, b1 = _convT_weight(c0, c1, g), 0.1 * torch.randn(c1, generator=g)
    return {"w_up0": w0, "b_up0": b0, "beta": beta, "gamma": gamma, "w_conv0": w1, "b_conv0": b1}


def stem_inputs(c0, c1, ch, B, below, seed_base=9900):
    """x0: integer-valued latents over several integers; g1 = dL/d(conv0's pre-activation): randn."""
    key = (c0, c1, ch, B, below)
    g = L.gen(seed_base + 1000 * c0 + 100 * ch + B + 7919 * STEM_SEED_BUMP.get(key, 0))
    inp = stem_weights(c0, c1, ch, g, below)
    inp["x0"] = torch.round(1.5 * torch.randn(B, ch, 2, 2, 2, generator=g))
    inp["g1"] = torch.randn(B, c1, 8, 8, 8, generator=g)
    return inp


def stem_forward(x0, w0, b0, beta, gamma, w1, b1):
    """(a0, h0, pre) in the dtype of the arguments."""
    a0 = F.conv_transpose3d(x0, w0, b0, stride=2, padding=2, output_padding=1)
    h0 = O.gdn3d(a0, beta, gamma, inverse=True)
    return a0, h0, F.conv_transpose3d(h0, w1, b1, stride=2, padding=2, output_padding=1)


def stem_ref(inp, dtype, backward=True):
    """The stem in ``dtype`` with autograd: a0, h0, y1 and -- from g1 = dL/d pre, the kernels' own contract (no ReLU
    mask) -- da0, dx0, dbeta (hat), dgamma (hat), dw_up0, db_up0 = sum da0, dw_conv0."""
    t = {k: inp[k].detach().to(dtype).clone().requires_grad_(backward)
         for k in ("x0", "w_up0", "b_up0", "beta", "gamma", "w_conv0", "b_conv0")}
    a0, h0, pre = stem_forward(t["x0"], t["w_up0"], t["b_up0"], t["beta"], t["gamma"], t["w_conv0"], t["b_conv0"])
    out = {"a0": a0.detach(), "h0": h0.detach(), "y1": torch.relu(pre).detach()}
    if backward:
        a0.retain_grad()
        pre.backward(inp["g1"].to(dtype))
        out.update(da0=a0.grad, dx0=t["x0"].grad, dbeta=t["beta"].grad, dgamma=t["gamma"].grad, dw_up0=t["w_up0"].grad,
                   db_up0=a0.grad.sum(dim=(0, 2, 3, 4)), dw_conv0=t["w_conv0"].grad)
    return out


def igdn_param_sums64(inp):
    """dL/d beta, dL/d gamma of the re-parametrised IGDN parameters (beta = max(beta_hat, bound)^2 - pedestal, the same for
    gamma) in float64: the summed gradient that reaches the LowerBound rule, whose sign decides whether a below-bound
    entry passes (negative: the step would raise the parameter) or is blocked."""
    d = torch.float64
    with torch.no_grad():
        beta = (O.floor_ste(inp["beta"].to(d), O.BETA_BOUND) ** 2 - O.PEDESTAL)
        gamma = (O.floor_ste(inp["gamma"].to(d), O.GAMMA_BOUND) ** 2 - O.PEDESTAL)
    beta.requires_grad_(True)
    gamma.requires_grad_(True)
    c0 = beta.numel()
    a0 = F.conv_transpose3d(inp["x0"].to(d), inp["w_up0"].to(d), inp["b_up0"].to(d), stride=2, padding=2, output_padding=1)
    h0 = a0 * torch.sqrt(F.conv3d(a0 ** 2, gamma.view(c0, c0, 1, 1, 1), beta))
    pre = F.conv_transpose3d(h0, inp["w_conv0"].to(d), inp["b_conv0"].to(d), stride=2, padding=2, output_padding=1)
    pre.backward(inp["g1"].to(d))
    return {"beta": beta.grad, "gamma": gamma.grad, "h0": h0.detach()}


# ---- the latent front ----------------------------------------------------------------------------------------------
def latent_stem_inputs(c0, c, B, seed_base=9950):
    """The latent table e (scaled so the rounded latents span several integers), the 1x1x1 generator and its GDN, the
    entropy model (|sigma| in [1.6, 2.4], one channel negative: the GDN's output stays inside +-3.2), permuted
    non-contiguous block ids with their counter noise rebuilt on the host, and the stem's weights at ch = c."""
    key = (c0, c, B)
    g = L.gen(seed_base + 1000 * c0 + 100 * c + B + 7919 * LATENT_SEED_BUMP.get(key, 0))
    inp = stem_weights(c0, 2 * c0, c, g, False)
    inp["e"] = 1.0 + 1.5 * torch.randn(B, c, 2, 2, 2, generator=g)
    inp["lat_w"] = torch.randn(c, c, 1, 1, 1, generator=g) * 1.5 * c ** -0.5
    inp["lat_b"] = 0.1 * torch.randn(c, generator=g)
    inp["lat_beta"], inp["lat_gamma"] = L.gdn_params(c, g, False)
    sigma = 1.6 + 0.8 * torch.rand(c, generator=g)
    sigma[c // 2] = -sigma[c // 2]
    inp["sigma"], inp["mu"] = sigma, 0.2 * torch.randn(c, generator=g)
    inp["ids"] = 3 * torch.randperm(B, generator=g) + 1
    inp["u_counter"] = torch.from_numpy(latent_noise(NOISE_SEED, NOISE_STEP, inp["ids"].tolist(), c))
    return inp


def latent_noise_of(inp, mode):
    """(kernel mode, the u the reference sees) of one of LATENT_MODES."""
    return ("eval", torch.zeros_like(inp["e"])) if mode == "eval" else ("train", inp["u_counter"])


def latent_ref(inp, mode, dtype):
    """The oracle's latent generator and entropy coder in ``dtype``: h, lat, x_rounded, bits."""
    c = inp["e"].shape[1]
    kmode, u = latent_noise_of(inp, mode)
    with torch.no_grad():
        e, w, b = inp["e"].to(dtype), inp["lat_w"].to(dtype), inp["lat_b"].to(dtype)
        P = {"latent_gen.h_analysis_2.kernel": w, "latent_gen.h_analysis_2.kernel_init": torch.zeros_like(w),
             "latent_gen.h_analysis_2.b": b, "latent_gen.h_analysis_2.b_init": torch.zeros_like(b),
             "latent_gen.gdn_2.beta": inp["lat_beta"].to(dtype), "latent_gen.gdn_2.gamma": inp["lat_gamma"].to(dtype),
             "entropy_coder.sigma": inp["sigma"].to(dtype).view(1, c, 1, 1, 1),
             "entropy_coder.mu": inp["mu"].to(dtype).view(1, c, 1, 1, 1)}
        lat = O.latent_gen(P, e)
        rounded, bits = O.entropy_coder(P, lat, kmode, u.to(dtype))
        return {"h": F.conv3d(e, w, b), "lat": lat, "x_rounded": rounded, "bits": bits}


def latent_stem_ref(inp, mode, dtype, x0=None):
    """latent_ref and, on its rounded latents (or on ``x0``: the float64 ones, so that the float32 column measures the
    stem's rounding and not a flipped integer), the stem's forward."""
    out = latent_ref(inp, mode, dtype)
    stem = dict(inp, x0=out["x_rounded"] if x0 is None else x0)
    out.update(stem_ref(stem, dtype, backward=False))
    return out


def half_distance(lat):
    """Smallest distance of a latent from a rounding boundary (k + 1/2)."""
    return float(((lat - torch.floor(lat)) - 0.5).abs().min())
