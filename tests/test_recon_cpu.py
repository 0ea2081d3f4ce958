"""recon.eval_batches without a device: which slices it cuts and what it hands to the net.  The stand-in net records its
arguments and returns the slice it was given."""
import pytest
import torch

from nvfpcc_amd.recon import eval_batches


class RecordingNet:
    def __init__(self):
        self.calls = []

    def reconstruct(self, x, q):
        self.calls.append(("reconstruct", x, q))
        return x

    def reconstruct_lod(self, x, lod, q, return_p):
        self.calls.append(("reconstruct_lod", x, lod, q, return_p))
        return x


def latents(n=5):
    return torch.arange(n * 3 * 8, dtype=torch.float32).reshape(n, 3, 2, 2, 2)


@pytest.mark.parametrize("batch,want", [(2, [(0, 2), (2, 4), (4, 5)]), (0, [(i, i + 1) for i in range(5)]),
                                        (-3, [(i, i + 1) for i in range(5)]), (7, [(0, 5)]), (5, [(0, 5)])])
def test_slices_are_consecutive_and_at_most_batch_blocks(batch, want):
    net, lat = RecordingNet(), latents()
    got = list(eval_batches(net, lat, batch))
    assert [(lo, hi) for lo, hi, _ in got] == want
    assert len(net.calls) == len(want)
    for (lo, hi, out), call in zip(got, net.calls):
        assert call[0] == "reconstruct" and call[2] == 2
        assert out is call[1] and torch.equal(out, lat[lo:hi])


def test_no_blocks_no_calls():
    net = RecordingNet()
    assert list(eval_batches(net, latents(0), 4)) == [] and net.calls == []


def test_every_slice_is_contiguous_also_of_a_strided_tensor():
    net = RecordingNet()
    wide = torch.arange(5 * 6 * 8, dtype=torch.float32).reshape(5, 6, 2, 2, 2)
    lat = wide[:, ::2]                          # every other channel: a block's slice is not contiguous
    assert not lat[0:2].is_contiguous()
    for lo, hi, out in eval_batches(net, lat, 2):
        assert out.is_contiguous() and torch.equal(out, lat[lo:hi])
    assert all(c[1].is_contiguous() for c in net.calls)


@pytest.mark.parametrize("lod,q,return_p", [(1, 2, False), (2, 0, True), (1, 0, True)])
def test_a_coarse_level_goes_to_reconstruct_lod_with_its_arguments(lod, q, return_p):
    net = RecordingNet()
    list(eval_batches(net, latents(), 2, lod, q, return_p))
    assert [c[0] for c in net.calls] == ["reconstruct_lod"] * 3
    assert all(c[2:] == (lod, q, return_p) for c in net.calls)


def test_level_zero_never_calls_reconstruct_lod_and_passes_q():
    net = RecordingNet()
    list(eval_batches(net, latents(), 2, lod=0, q=0, return_p=True))
    assert [(c[0], c[2]) for c in net.calls] == [("reconstruct", 0)] * 3


def test_the_loop_is_lazy_and_leaves_gradients_to_the_caller():
    net, lat = RecordingNet(), latents().requires_grad_()
    it = eval_batches(net, lat, 2)
    assert net.calls == []
    _, _, out = next(it)
    assert len(net.calls) == 1 and out.requires_grad
