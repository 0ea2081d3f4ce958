"""nvf_block_costs (csrc/block_costs.hip, ops.block_costs): per block the main focal sum and the eval-mode latent bits,
float32 terms added in float64 by one workgroup per block.

Reference: tests/block_costs_ref.py, numpy float64, evaluated on the device's own float32 p and rounded latents.
Tolerance: every term is non-negative and the accumulation is float64, so a row's relative error is bounded by the
per-term float32 error; every row is held to 8e-6 relative (the floor of the project's parity rule), rows that are
exactly 0 to an absolute floor.  Every test prints the largest deviation it found.

Inputs: the eval forward of the two trained fixture decoders (tests/conformance_ref.build_engine) at batch 1, 5 and 12,
and a hand-made batch with the values at which focal_elem and rate_term branch."""
import numpy as np
import pytest
import torch

from tests import block_costs_ref as R
from tests import conformance_ref as C

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.9, 1.0
_ENG = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


def engine(tag, gpu, golden_dir):
    if tag not in _ENG:
        _ENG[tag] = C.build_engine(golden_dir, tag, gpu)[0]
    return _ENG[tag]


def costs(eng, lo, hi):
    """(device rows float64 [hi - lo, 2], reference rows) of blocks [lo, hi) evaluated as ONE batch."""
    from nvfpcc_amd import ops
    a = eng.eval_forward(lo, hi, q=2)
    sigma, mu = (t.detach() for t in eng._ec())
    got = ops.block_costs(a["p2"], eng.gt[lo:hi], eng.dist[lo:hi], ALPHA, BETA, a["x0"], sigma, mu)
    ref = R.rows(a["p2"].cpu().numpy(), eng.gt[lo:hi].cpu().numpy(), eng.dist[lo:hi].cpu().numpy(), ALPHA, BETA,
                 a["x0"].cpu().numpy(), sigma.cpu().numpy(), mu.cpu().numpy())
    return got, ref


@pytest.mark.parametrize("tag", C.TAGS)
def test_rows_of_the_trained_decoders_at_batch_1_5_and_12(tag, gpu, golden_dir):
    """Every row against float64 at the three batch sizes, and batch invariance: row b at batch 12 and at batch 5 is
    bit-equal to the same block alone."""
    eng = engine(tag, gpu, golden_dir)
    alone = torch.cat([costs(eng, b, b + 1)[0] for b in range(C.N_BLOCKS)], 0)
    for batch in (1, 5, 12):
        got, ref = zip(*[costs(eng, lo, min(lo + batch, C.N_BLOCKS)) for lo in range(0, C.N_BLOCKS, batch)])
        got, ref = torch.cat(got, 0), np.concatenate(ref, 0)
        assert got.dtype == torch.float64 and tuple(got.shape) == (C.N_BLOCKS, 2)
        for col, name in enumerate(("focal", "bits")):
            rel, zero = R.deviation(got[:, col].cpu().numpy(), ref[:, col])
            print(f"[block_costs {tag} batch {batch}] {name}: largest relative deviation {rel:.2e} (bound {R.RTOL:.0e}), "
                  f"rows of 0: {zero:.1e}")
        assert R.close(got[:, 0].cpu().numpy(), ref[:, 0]) and R.close(got[:, 1].cpu().numpy(), ref[:, 1]), (tag, batch)
        assert (ref > 0).all(), "a trained block has a positive cost"
        assert torch.equal(got, alone), f"{tag}: a row at batch {batch} is not the row of the block alone"


@pytest.mark.parametrize("tag", C.TAGS)
def test_column_sums_agree_with_eval_sums(tag, gpu, golden_dir):
    """The column sums over the 12 blocks against eval_sums' entries [0] (main focal term) and [21] (latent bits): those
    are float32 sums in another order, 8e-6 relative."""
    eng = engine(tag, gpu, golden_dir)
    got, _ = costs(eng, 0, C.N_BLOCKS)
    sums = eng.eval_sums(q=2).double().cpu().numpy()
    tot = got.sum(0).cpu().numpy()
    for col, k, name in ((0, 0, "focal"), (1, 21, "bits")):
        rel = abs(tot[col] - sums[k]) / abs(sums[k])
        print(f"[block_costs {tag}] sum of {name}: {tot[col]:.9e} against eval_sums[{k}] = {sums[k]:.9e}: {rel:.2e}")
        assert rel <= R.RTOL, (tag, name, rel)


def hand_made(c):
    """7 blocks of 2048 voxels (two strides of the workgroup): p cycles through 0, 1, 1e-10, 0.5 and a denormal beside
    ordinary values; block 0 is empty, block 1 full, block 2 has p == gt (a row of exactly 0 without dist weights); the
    latents of block 3 sit at +-40 (the likelihood floor), the others in the bulk."""
    g = torch.Generator().manual_seed(4100 + c)
    B, V = 7, 2048
    p = 0.02 + 0.96 * torch.rand(B, V, generator=g)
    special = torch.tensor([0.0, 1.0, 1e-10, 0.5, 1e-40])
    assert 0 < float(special[4]) < 1.1754944e-38
    p[:, ::3] = special[torch.arange(p[:, ::3].shape[1]) % 5]
    gt = (torch.rand(B, V, generator=g) > 0.7).float()
    gt[0], gt[1] = 0.0, 1.0
    p[2] = gt[2]
    dist = torch.rand(B, V, generator=g)
    sigma = 0.6 + 0.8 * torch.rand(c, generator=g)
    sigma[c // 2] = -sigma[c // 2]
    mu = 0.3 * torch.randn(c, generator=g)
    x = torch.round(mu.view(1, c, 1, 1, 1) + sigma.abs().view(1, c, 1, 1, 1) * torch.clamp(torch.randn(B, c, 2, 2, 2, generator=g), -2, 2))
    x[3] = 40.0
    x[3, :, 0] = -40.0
    return p, gt, dist, x, sigma, mu


@pytest.mark.parametrize("c", [8, 3])
def test_hand_made_batch(c, gpu):
    from nvfpcc_amd import ops
    p, gt, dist, x, sigma, mu = hand_made(c)
    d = lambda t: None if t is None else t.to(gpu).contiguous()
    for name, ds in (("dist", dist), ("dist = 0", torch.zeros_like(dist)), ("dist = NULL", None)):
        got = ops.block_costs(d(p), d(gt), d(ds), ALPHA, BETA, d(x), d(sigma), d(mu)).cpu().numpy()
        ref = R.rows(p.numpy(), gt.numpy(), None if ds is None else ds.numpy(), ALPHA, BETA, x.numpy(), sigma.numpy(), mu.numpy())
        for col, what in enumerate(("focal", "bits")):
            rel, zero = R.deviation(got[:, col], ref[:, col])
            print(f"[block_costs hand-made c={c} {name}] {what}: largest relative deviation {rel:.2e}, rows of 0: {zero:.1e}")
            assert R.close(got[:, col], ref[:, col]), (name, what, got[:, col], ref[:, col])
        if name == "dist = NULL":
            assert ref[2, 0] == 0 and got[2, 0] == 0, "p == gt: every term is 0"
        if name == "dist = 0":      # the empty block's weights are all dist + 0
            assert ref[0, 0] == 0 and got[0, 0] == 0
        # the floor: 8 c symbols of -log2(1e-8) each
        assert abs(ref[3, 1] - 8 * c * -np.log2(1e-8)) < 1e-9
        # batch invariance on this batch too
        for b in (0, 3, 6):
            one = ops.block_costs(d(p[b:b + 1]), d(gt[b:b + 1]), None if ds is None else d(ds[b:b + 1]), ALPHA, BETA,
                                  d(x[b:b + 1]), d(sigma), d(mu)).cpu().numpy()
            assert np.array_equal(one[0], got[b]), (name, b)


def test_refusals(gpu):
    """Every refusal of include/nvf_hip.h returns NVF_EINVAL and launches nothing."""
    from nvfpcc_amd._lib import CONSTANTS, lib
    E = CONSTANTS["NVF_EINVAL"]
    B, V, c, sp = 2, 2048, 8, 8
    p, gt, dist = (torch.rand(B, V, device=gpu) for _ in range(3))
    x, sigma, mu = torch.zeros(B, c, 2, 2, 2, device=gpu), torch.ones(c, device=gpu), torch.zeros(c, device=gpu)
    out = torch.zeros(B, 2, dtype=torch.float64, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(p=p.data_ptr(), gt=gt.data_ptr(), dist=dist.data_ptr(), alpha=ALPHA, beta=BETA, x=x.data_ptr(),
              sigma=sigma.data_ptr(), mu=mu.data_ptr(), out=out.data_ptr(), batch=B, voxels=V, c=c, spatial=sp)

    def call(**kw):
        a = dict(ok, **kw)
        return lib().nvf_block_costs(a["p"], a["gt"], a["dist"], a["alpha"], a["beta"], a["x"], a["sigma"], a["mu"], a["out"],
                                     a["batch"], a["voxels"], a["c"], a["spatial"], s)
    assert call() == 0 and call(dist=None) == 0
    for k in ("p", "gt", "x", "sigma", "mu", "out"):
        assert call(**{k: None}) == E, k
    assert call(batch=0) == E and call(batch=-1) == E
    assert call(voxels=V + 4) == E and call(voxels=1000) == E and call(voxels=0) == E
    assert call(c=9) == E and call(c=8, spatial=9) == E and call(c=65, spatial=1) == E
    assert call(p=p.data_ptr() + 4) == E and call(dist=dist.data_ptr() + 8) == E      # 16-byte loads
    x64, s64, m64 = torch.zeros(B, 64, device=gpu), torch.ones(64, device=gpu), torch.zeros(64, device=gpu)
    assert call(c=8, spatial=8) == 0 and call(c=64, spatial=1, x=x64.data_ptr(), sigma=s64.data_ptr(), mu=m64.data_ptr()) == 0
    torch.cuda.synchronize()
