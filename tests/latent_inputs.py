"""Case tables, inputs and float64 references of the reductions over a whole batch on the latent side
(tests/test_gpu_latent_reductions.py on the device, tests/test_latent_inputs_cpu.py without one).

Everything here is torch on the CPU plus the oracle (oracle/nvf_oracle.py: entropy_coder, gdn3d, floor_ste through
them); no kernel of this project.  The switch points of the kernels are restated in Python so that the CPU test can
prove that every entry of a case table lands on the code path its comment names:

    latent_rate_body (csrc/latent_tail.h)   LDS path iff  nel = B * spatial <= 1024  and  3 c (nel + 16) <= 3456
    nvf_gdn_bwd (csrc/pointwise.hip)        per = ceil(nvox / 256) rounded up to 128, nslab = ceil(nvox / per);
                                            8 / 4 threads per voxel iff nslab < 128 and c % 8 / c % 4 == 0, else 1
    nvf_focal_loss / nvf_focal_loss_multi   ceil(n / 2048) / ceil(n / 1024) workgroups, at most kLossMaxWG = 1024

Tolerance rule of the sums (the one of tests/test_gpu_trained_state.py): err < max(t, 3 * d32), t the suite's figure
for the quantity, d32 the distance of the float32 CPU oracle from the float64 one on the same inputs -- never a number
of the device.
"""
import torch

from oracle import nvf_oracle as O
from tests.philox_np import latent_noise

# ---- the switch points, restated -------------------------------------------------------------------------------
RATE_VT = 1024                               # kRateVT: threads of the virtual workgroup = stride of the loop path
RATE_NVW = RATE_VT // 64                     # its virtual waves
RATE_SCRATCH = 3 * 8 * (128 + 16)            # kTailRateLds: scratch floats of both callers of latent_rate_body
GDN_THREADS, GDN_MAX_SLABS = 128, 256        # kGdnThreads, kGdnMaxSlabs
LOSS_MAX_WG = 1024                           # kLossMaxWG
SLICE = 16                                   # blocks of a mini-batch: every c <= 8 stays on the LDS path there


def rate_path(c, B, spatial=8):
    """'lds' or 'loop': the branch of latent_rate_body (and, with a third of the scratch and of the terms, of
    latent_fwd_body: c (nel + 16) <= 1152 is the same condition)."""
    nel = B * spatial
    return "lds" if nel <= RATE_VT and 3 * c * (nel + RATE_NVW) <= RATE_SCRATCH else "loop"


def gdn_form(c, spatial, B):
    """What nvf_gdn_bwd launches: voxels per workgroup, workgroups, threads per voxel, 128-voxel tiles per full
    workgroup, live voxels of the last workgroup, tiles the last workgroup walks, own[] slots per thread, and whether
    the one workgroup finishes the parameter gradients itself."""
    nvox = B * spatial
    per = -(-nvox // GDN_MAX_SLABS)
    per = -(-per // GDN_THREADS) * GDN_THREADS
    nslab = -(-nvox // per)
    cg = 8 if nslab < 128 and c % 8 == 0 else 4 if nslab < 128 and c % 4 == 0 else 1
    last = nvox - (nslab - 1) * per
    return {"nvox": nvox, "per": per, "nslab": nslab, "cg": cg, "tiles": per // GDN_THREADS, "last_live": last,
            "last_tiles": -(-last // GDN_THREADS), "own_slots": -(-(c + c * c) // (GDN_THREADS * cg)),
            "finishes_itself": nslab == 1}


def focal_workgroups(n, per_wg):
    """(workgroups, grid-strides?) of nvf_focal_loss (per_wg = 256 * 8) / nvf_focal_loss_multi (256 * 4)."""
    nwg = -(-n // per_wg)
    return min(nwg, LOSS_MAX_WG), nwg > LOSS_MAX_WG


# ---- case tables -------------------------------------------------------------------------------------------------
# (c, B, path) at spatial 8
RATE_CASES = [
    (8, 16, "lds"),      # nel 128: 3*8*144 = 3456 floats, the last size in the scratch
    (8, 17, "loop"),     # nel 136: one block past it
    (8, 129, "loop"),    # nel 1032: virtual lanes 0..7 take a second element, one 1024 stride on
    (8, 600, "loop"),    # the resident batch of a training step: 4800 elements per channel, 38 400 terms
    (3, 46, "lds"),      # nel 368: 3*3*384 = 3456
    (3, 47, "loop"),     # nel 376
    (3, 600, "loop"),
    (1, 128, "lds"),     # nel 1024: the scratch would hold more, the nel <= 1024 clause decides
    (1, 129, "loop"),    # nel 1032
]
RATE_MODES = ["eval", "train_u", "train_counter"]

# (c, spatial, B, below-bound parameters, what it reaches)
GDN_CASES = [
    (8, 8, 16, False, "one workgroup, finishes itself"),
    (8, 8, 17, True, "two slabs, 8 live lanes in the second, gdn_bwd_final; 8 threads per voxel"),
    (3, 8, 47, False, "1 thread per voxel, three slabs"),
    (12, 64, 3, False, "4 threads per voxel"),
    (32, 64, 5, True, "8 threads per voxel, four channels per thread, two own[] slots"),
    (16, 64, 254, False, "127 slabs: last size on the 8-thread form"),
    (16, 64, 255, False, "128 slabs: first size on the 1-thread form"),
    (16, 64, 513, True, "256 voxels per workgroup: two tiles, own[] carried; the last workgroup stops after one"),
    (32, 64, 600, False, "the wide decoder's IGDN at the resident batch: 1-thread form, two tiles, 9 own[] slots"),
]

# (c, B, below-bound parameters); every one past the rate's LDS path and past one GDN chunk of the tail
TAIL_CASES = [(8, 17, True), (3, 47, False), (8, 600, True), (3, 600, False)]

FOCAL_CASES = [64 * 32768, 65 * 32768, 65 * 32768 + 3]      # nvf_focal_loss: 1024 workgroups exactly, then grid-stride
FOCAL_MULTI_BLOCKS = [32, 33]                               # nvf_focal_loss_multi: the same for float4 groups


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- latent rate -------------------------------------------------------------------------------------------------
RATE_SEED, RATE_STEP = 9, 4


def rate_inputs(c, B, seed_base=9100):
    """Bulk latents only: x = mu + |sigma| clamp(N(0,1), +-2.2), |sigma| in [0.6, 1.4], one channel with negative
    sigma; block ids non-contiguous and permuted; the counter noise of those ids rebuilt on the host."""
    g = gen(seed_base + 1000 * c + B)
    sigma = 0.6 + 0.8 * torch.rand(c, generator=g)
    sigma[c // 2] = -sigma[c // 2]                       # abs() path, and the sign in d/dsigma
    mu = 0.3 * torch.randn(c, generator=g)
    z = torch.clamp(torch.randn(B, c, 2, 2, 2, generator=g), -2.2, 2.2)
    x = mu.view(1, c, 1, 1, 1) + sigma.abs().view(1, c, 1, 1, 1) * z
    u = torch.rand(B, c, 2, 2, 2, generator=g)
    addend = 0.1 * torch.randn(B, c, 2, 2, 2, generator=g)
    ids = 3 * torch.randperm(B, generator=g) + 1
    u_counter = torch.from_numpy(latent_noise(RATE_SEED, RATE_STEP, ids.tolist(), c))
    return {"x": x, "sigma": sigma, "mu": mu, "u": u, "u_counter": u_counter, "addend": addend, "ids": ids}


def rate_noise(inp, mode):
    """(kernel mode, the u the reference sees) of one of RATE_MODES."""
    if mode == "eval":
        return "eval", torch.zeros_like(inp["x"])
    return "train", inp["u"] if mode == "train_u" else inp["u_counter"]


def likelihood64(x, sigma, mu, mode, u):
    """Per-element likelihood Phi(up) - Phi(lo) in float64."""
    c = x.shape[1]
    v = (x.double() + (u.double() - 0.5)) if mode == "train" else torch.round(x).double()
    s, m = sigma.abs().double().view(1, c, 1, 1, 1), mu.double().view(1, c, 1, 1, 1)
    cdf = lambda t: 0.5 * (1 + torch.erf(t / 2 ** 0.5))
    return cdf((v - m + 0.5) / s) - cdf((v - m - 0.5) / s)


def rate_ref(x, sigma, mu, mode, u, g, addend, dtype):
    """The oracle's entropy coder with autograd in ``dtype``: rounded, bits, dx = addend + g dbits/dx, g dbits/dsigma,
    g dbits/dmu."""
    c = x.shape[1]
    xs = x.detach().to(dtype).clone().requires_grad_(True)
    s = sigma.detach().to(dtype).view(1, c, 1, 1, 1).clone().requires_grad_(True)
    m = mu.detach().to(dtype).view(1, c, 1, 1, 1).clone().requires_grad_(True)
    rounded, bits = O.entropy_coder({"entropy_coder.sigma": s, "entropy_coder.mu": m}, xs, mode, u.to(dtype))
    (torch.tensor(g, dtype=dtype) * bits).backward()
    dx = xs.grad if addend is None else addend.to(dtype) + xs.grad
    return {"rounded": rounded.detach(), "bits": bits.detach(), "dx": dx, "dsigma": s.grad.reshape(-1),
            "dmu": m.grad.reshape(-1)}


# ---- GDN -----------------------------------------------------------------------------------------------------------
# Input condition of the GDN cases.  The LowerBound of beta alone keeps every norm above sqrt(1e-6) = 1e-3, and with
# beta[0] = 1e-4 channel 0 sits on that floor wherever its voxel's inputs are small; t = -dy x / norm^3 there is 1e9 dy x,
# and one such voxel would decide a whole parameter sum.  The inputs are required to stay five times above the floor.
GDN_MIN_NORM = 5e-3


def gdn_params(c, g, below_bound):
    """beta / gamma of test_gdn_forward_backward; below_bound places entries under the LowerBound of either."""
    beta = torch.sqrt(torch.ones(c) + 2.0 ** -36) + 0.05 * torch.randn(c, generator=g)
    gamma = torch.sqrt(0.1 * torch.eye(c) + 2.0 ** -36) + 0.02 * torch.randn(c, c, generator=g).abs()
    if below_bound:
        beta[0] = 1e-4
        gamma[0, 1] = 1e-7
        gamma[2, 3] = -0.3
    return beta, gamma


def gdn_inputs(c, spatial, B, below_bound, seed_base=9300):
    n = round(spatial ** (1 / 3))
    assert n ** 3 == spatial
    g = gen(seed_base + 1000 * c + B)
    x = torch.randn(B, c, n, n, n, generator=g)
    beta, gamma = gdn_params(c, g, below_bound)
    gy = torch.randn(B, c, n, n, n, generator=g)
    return {"x": x, "beta": beta, "gamma": gamma, "gy": gy}


def gdn_norm64(x, beta, gamma):
    """The GDN norm sqrt(beta + sum_j gamma_cj x_j^2) of every element, float64."""
    with torch.no_grad():
        b = O.floor_ste(beta.double(), O.BETA_BOUND) ** 2 - O.PEDESTAL
        gm = O.floor_ste(gamma.double(), O.GAMMA_BOUND) ** 2 - O.PEDESTAL
        return torch.sqrt(torch.nn.functional.conv3d(x.double() ** 2, gm.view(*gamma.shape, 1, 1, 1), b))


def gdn_ref(x, beta, gamma, gy, inverse, dtype):
    """The oracle's gdn3d with autograd in ``dtype``: y, dx, dbeta_hat, dgamma_hat."""
    x_ = x.detach().to(dtype).clone().requires_grad_(True)
    b_ = beta.detach().to(dtype).clone().requires_grad_(True)
    g_ = gamma.detach().to(dtype).clone().requires_grad_(True)
    y = O.gdn3d(x_, b_, g_, inverse)
    y.backward(gy.detach().to(dtype))
    return {"y": y.detach(), "dx": x_.grad, "dbeta": b_.grad, "dgamma": g_.grad}


# ---- the latent tail -----------------------------------------------------------------------------------------------
TAIL_G_DEV, TAIL_G_HOST = 0.37, 1.5


def tail_inputs(c, B, below_bound, seed_base=9500):
    """The tail's three stages take independent tensors: latents (bulk, as in rate_inputs), the GDN's input h, the 1x1x1
    convolution's input e."""
    inp = rate_inputs(c, B, seed_base)
    g = gen(seed_base + 500 + 1000 * c + B)
    inp["h"] = torch.randn(B, c, 2, 2, 2, generator=g)
    inp["e"] = torch.randn(B, c, 2, 2, 2, generator=g)
    inp["beta"], inp["gamma"] = gdn_params(c, g, below_bound)
    return inp


def tail_chain(lat, h, e, sigma, mu, beta, gamma, mode, u, g, addend, dtype):
    """Rate gradient -> GDN backward (forward direction) -> 1x1x1 weight and bias gradient, every stage in ``dtype``
    from the stage before it."""
    r = rate_ref(lat, sigma, mu, mode, u, g, addend, dtype)
    d = gdn_ref(h, beta, gamma, r["dx"], False, dtype)
    dh = d["dx"]
    c = lat.shape[1]
    dw = torch.einsum("nap,nbp->ab", dh.flatten(2), e.to(dtype).flatten(2)).reshape(c, c, 1, 1, 1)
    return {"dlat": r["dx"], "dsigma": r["dsigma"], "dmu": r["dmu"], "dh": dh, "dbeta": d["dbeta"],
            "dgamma": d["dgamma"], "dw": dw, "db": dh.sum(dim=(0, 2, 3, 4))}


# ---- focal sums ----------------------------------------------------------------------------------------------------
def focal_inputs(n, seed_base=9700):
    """p in (0.02, 0.98), a quarter of the voxels occupied, dist uniform: flat float32 tensors of n elements."""
    g = gen(seed_base + n % 1000)
    p = 0.02 + 0.96 * torch.rand(n, generator=g)
    gt = (torch.rand(n, generator=g) > 0.75).float()
    dist = torch.rand(n, generator=g)
    return p, gt, dist


# ---- comparison ----------------------------------------------------------------------------------------------------
def max_rel(a, b64):
    """max |a - b| / max |b| in float64."""
    a, b64 = a.detach().cpu().double().reshape(-1), b64.detach().double().reshape(-1)
    return float((a - b64).abs().max() / max(float(b64.abs().max()), 1e-300))


def bound(t, d32):
    """The tolerance rule: the suite's figure, or three times what the float32 oracle itself is away from float64."""
    return max(t, 3.0 * d32)


def fmt_row(tag, name, err, d32, t):
    b = bound(t, d32)
    return f"[{tag}] {name}: device {err:.2e} | float32 oracle {d32:.2e} | bound {b:.2e}" + (" (above t)" if b > t else "")
