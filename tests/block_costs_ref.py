"""float64 restatement of the two row sums of nvf_block_costs (csrc/block_costs.hip), in numpy alone: the focal term of
csrc/finals.h (focal_elem, with its clamp at 1e-9) and the Gaussian rate of csrc/latent_tail.h (rate_term, with its floor
at 1e-8), each summed over one block.  Evaluated on the float32 values the device holds (p, gt, dist, the rounded
latents, sigma, mu); no kernel of this project.  Shared by tests/test_gpu_block_costs.py and tests/test_gpu_fit_latents.py."""
import math

import numpy as np

RTOL = 8e-6        # the floor of the project's parity rule (tests/latent_inputs.py: bound(t, d32))
ATOL = 1e-30       # rows that are exactly 0

_erf = np.vectorize(math.erf, otypes=[np.float64])


def focal_rows(p, gt, dist, alpha, beta):
    """[B, V] float32 arrays (dist may be None) -> float64 [B]: sum over a block of -a_t (1 - F)^2 w ln F with
    F = max(p or 1 - p, 1e-9), a_t = alpha or 1 - alpha, w = 1 or dist + gt * beta."""
    p, gt = np.asarray(p, np.float64), np.asarray(gt, np.float64)
    B = p.shape[0]
    p, gt = p.reshape(B, -1), gt.reshape(B, -1)
    occ = gt != 0
    a1 = np.float64(np.float32(alpha))
    F = np.maximum(np.where(occ, p, 1.0 - p), 1e-9)
    at = np.where(occ, a1, 1.0 - a1)
    w = 1.0 if dist is None else np.asarray(dist, np.float64).reshape(B, -1) + np.where(occ, np.float64(np.float32(beta)), 0.0)
    return (-at * (1.0 - F) ** 2 * w * np.log(F)).sum(1)


def rate_rows(x_rounded, sigma, mu):
    """[B, c, ...] rounded latents, sigma / mu [c] -> float64 [B]: sum over a block's symbols of
    -log2 max(Phi((v - mu + .5) / |sigma|) - Phi((v - mu - .5) / |sigma|), 1e-8)."""
    x = np.asarray(x_rounded, np.float64)
    B, c = x.shape[0], x.shape[1]
    x = x.reshape(B, c, -1)
    s = np.abs(np.asarray(sigma, np.float64)).reshape(1, c, 1)
    m = np.asarray(mu, np.float64).reshape(1, c, 1)
    cdf = lambda t: 0.5 * (1.0 + _erf(t / math.sqrt(2.0)))
    like = cdf((x - m + 0.5) / s) - cdf((x - m - 0.5) / s)
    return (-np.log2(np.maximum(like, 1e-8))).sum((1, 2))


def rows(p, gt, dist, alpha, beta, x_rounded, sigma, mu):
    """float64 [B, 2], as nvf_block_costs lays its output out."""
    return np.stack([focal_rows(p, gt, dist, alpha, beta), rate_rows(x_rounded, sigma, mu)], 1)


def deviation(got, ref):
    """(largest |got - ref| / |ref| over the rows with ref != 0, largest |got| over the rows with ref == 0)."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    nz = ref != 0
    rel = float((np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])).max()) if nz.any() else 0.0
    zero = float(np.abs(got[~nz]).max()) if (~nz).any() else 0.0
    return rel, zero


def close(got, ref):
    rel, zero = deviation(got, ref)
    return np.isfinite(np.asarray(got)).all() and rel <= RTOL and zero <= ATOL
