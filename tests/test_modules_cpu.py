"""Host-side logic of the operator mirror, checked on CPU: construction, seed plumbing, state-dict
layout (keys, order, shapes, values) against the oracle, which is itself pinned to the reference."""
import numpy as np
import pytest
import torch

from nvfpcc_amd import network
from nvfpcc_amd.model import Net
from nvfpcc_amd.seeds import synthetic_seed
from oracle import nvf_oracle as O
from tests.golden_inputs import CONFIGS


@pytest.mark.parametrize("tag", ["S", "W"])
def test_state_dict_equals_reference_layout(tag):
    cfg = CONFIGS[tag]
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", cfg["ch"], ",".join(str(c) for c in cfg["channels"]), verbose=False)
    P, used = O.build_state(cfg["ch"], cfg["channels"], synthetic_seed())
    sd = net.state_dict()
    assert list(sd.keys()) == list(P.keys())
    assert network.seed_ptr == used
    for k in P:
        assert sd[k].shape == P[k].shape, k
        assert torch.equal(sd[k], P[k]), k
    assert [n for n, _ in net.named_parameters()] == O.trainable_keys(P)
    assert len(list(net.parameters())) == 28


def test_seed_pointer_keeps_advancing_like_the_reference():
    network.reset_seed(synthetic_seed())
    Net(None, "Gaussian", 3, "8,16,8,8", verbose=False)
    assert network.seed_ptr == 52127
    b = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False)
    assert network.seed_ptr == 104254
    network.reset_seed(synthetic_seed())
    a = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False)
    assert not torch.equal(a.reconstructor.up0.kernel_init, b.reconstructor.up0.kernel_init)


def test_bits_bookkeeping():
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False)
    assert net.entropy_coder.get_bits() == 192
    assert O.decoder_aux_bits((8, 16, 8, 8)) == (16 * 2 + 8 * 2 + 8 * 2) * 32 + 32 + (256 + 16) * 32


def test_forward_refuses_cpu():
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.ones(1, 3, 2, 2, 2), "eval", 2)


def test_dataset_permutation_and_epoch_order(tmp_path):
    from nvfpcc_amd.dataloader import LoadedVoxelDataset
    from nvfpcc_amd.synth import write_dataset
    prefix = str(tmp_path / "toy")
    gts, dists = write_dataset(prefix, 7)
    ds = LoadedVoxelDataset(prefix + "_l5_origins.npy", prefix + "_l5_gt_grid.npy", prefix + "_l5_dist.npy")
    assert len(ds) == 7 and ds.N == gts.sum()
    idx, g, d = ds[3]
    assert idx.item() == (3 * 2113) % 7 and idx.dtype == torch.int64
    assert torch.equal(g, torch.from_numpy(gts[idx.item()]).float()) and g.dtype == torch.float32
    assert sorted(ds.epoch_order(0, True).tolist()) == list(range(7))
    assert ds.epoch_order(0, False).tolist() == [(i * 2113) % 7 for i in range(7)]
    ds2 = LoadedVoxelDataset(prefix + "_l5_origins.npy", prefix + "_l5_gt_grid.npy", prefix + "_l5_dist.npy",
                             shuffle=False)
    assert ds2[3][0].item() == 3


@pytest.mark.parametrize("a,b,k,stride,pad,n", [(8, 8, 4, 1, 0, 7), (8, 8, 5, 2, 0, 4), (16, 8, 5, 2, 0, 3), (8, 16, 5, 2, 2, 4),
                                               (1, 8, 3, 1, 1, 6)])
def test_shifted_slice_reference_equals_torch_autograd(a, b, k, stride, pad, n):
    """tests/wgrad_ref64.py (the float64 reference of the batch-edge GPU tests) against torch's own float64 convolution
    backward, for every (k, stride, pad) the decoder has and as running sums over batch prefixes with a chunk smaller than a
    prefix.  Stride-1 layers: p = dY, q = X of F.conv3d (dw as [out, in]); stride 2: p = X, q = dY of F.conv_transpose3d."""
    import torch.nn.functional as F
    from tests.wgrad_ref64 import wgrad_ref64, channel_sum_ref64
    g = torch.Generator().manual_seed(a + 3 * b + k)
    B, ends = 5, [2, 3, 5]
    if stride == 1:
        x = torch.randn(B, b, n + k - 1 - 2 * pad, n + k - 1 - 2 * pad, n + k - 1 - 2 * pad, generator=g)
        gy = torch.randn(B, a, n, n, n, generator=g)
        p, q = gy, x
    else:
        x = torch.randn(B, a, n, n, n, generator=g)
        m = 2 * (n - 1) + 5 - 2 * pad + (1 if pad else 0)          # output_padding 1 on the padded layers (4^3 -> 8^3)
        gy = torch.randn(B, b, m, m, m, generator=g)
        p, q = x, gy
    got = wgrad_ref64(p, q, k, stride, pad, ends=ends, chunk_bytes=1)
    sums = channel_sum_ref64(q, ends)
    for e, dw, s in zip(ends, got, sums):
        if stride == 1:
            w = torch.zeros(a, b, k, k, k, dtype=torch.float64, requires_grad=True)
            F.conv3d(x[:e].double(), w, None, 1, pad).backward(gy[:e].double())
        else:
            w = torch.zeros(a, b, 5, 5, 5, dtype=torch.float64, requires_grad=True)
            F.conv_transpose3d(x[:e].double(), w, None, 2, pad, 1 if pad else 0).backward(gy[:e].double())
        assert (dw - w.grad).abs().max().item() < 1e-12 * max(w.grad.abs().max().item(), 1.0)
        assert torch.allclose(s, q[:e].double().sum(dim=(0, 2, 3, 4)), rtol=1e-13, atol=1e-12)
