"""The full-batch passes in bounded chunks (TrainEngine.latent_step_chunked, the chunked eval_sums) against the single
pass, on the 24 synthetic blocks and the narrow decoder: chunks of 7 are 7 + 7 + 7 + 3, a ragged tail.

Each route is held to 8e-6 of the float64 oracle by the project's parity rule, so two routes differ by at most twice that."""
import numpy as np
import pytest
import torch

from tests.test_gpu_engine import gpu, make  # noqa: F401  (gpu: the module's device fixture)

pytestmark = pytest.mark.gpu
N = 24
TOL = 2 * 8e-6


def state(eng):
    return eng.emb.clone(), eng.emb_m.clone(), eng.emb_v.clone()


@pytest.mark.parametrize("q", [1, 2])
def test_chunks_of_7_give_the_single_pass_gradient(q, gpu):
    _, one = make("S", gpu, N)[:2]
    _, chunked = make("S", gpu, N)[:2]
    assert all(torch.equal(a, b) for a, b in zip(state(one), state(chunked))) and torch.equal(one.flat_p, chunked.flat_p)
    before = state(chunked)
    _, de_ref = one.latent_step(q, 0, N, update=False)
    de = chunked.latent_step_chunked(q, 0, N, chunk=7, update=False)
    assert (one.noise_step, one.emb_step) == (chunked.noise_step, chunked.emb_step) == (1, 0)
    assert de.shape == de_ref.shape == (N, 3, 2, 2, 2)
    err = (de.double() - de_ref.double()).abs().max().item()
    top = de_ref.double().abs().max().item()
    print("q=%d max|de - de_ref| = %.3e, max|de_ref| = %.3e, ratio %.3e, bit-equal: %s" % (q, err, top, err / top, torch.equal(de, de_ref)))
    assert top > 0 and err <= TOL * top, (err, top)
    assert all(torch.equal(a, b) for a, b in zip(state(chunked), before)), "update=False moves no latent"
    # every chunk saw the same draw: the rows of a chunk are the bits of a pass over that chunk alone at that counter
    _, alone = make("S", gpu, N)[:2]
    _, de_tail = alone.latent_step(q, 21, N, update=False)
    assert alone.noise_step == 1 and torch.equal(de[21:], de_tail)


def test_update_is_one_adam_step_over_all_rows(gpu):
    from nvfpcc_amd import ops
    _, eng = make("S", gpu, N)[:2]
    _, twin = make("S", gpu, N)[:2]
    emb, m, v = state(eng)
    de = eng.latent_step_chunked(1, 0, N, chunk=7, update=True)
    assert (eng.noise_step, eng.emb_step) == (1, 1)
    assert torch.equal(de, twin.latent_step_chunked(1, 0, N, chunk=7, update=False))
    ops.adam_step(emb.view(-1), de.contiguous().view(-1), m.view(-1), v.view(-1), eng.lr_emb, 1)
    torch.cuda.synchronize()
    assert torch.equal(eng.emb, emb) and torch.equal(eng.emb_m, m) and torch.equal(eng.emb_v, v)
    assert bool((eng.emb != twin.emb).flatten(1).any(1).all()), "all 24 rows moved"
    # a second step draws again and is Adam's step 2
    eng.latent_step_chunked(2, 0, N, chunk=7)
    assert (eng.noise_step, eng.emb_step) == (2, 2)


@pytest.mark.parametrize("chunk", [24, 100])
def test_a_chunk_that_holds_the_shard_is_latent_step(chunk, gpu):
    _, one = make("S", gpu, N)[:2]
    _, chunked = make("S", gpu, N)[:2]
    for q in (1, 2):
        _, de_ref = one.latent_step(q, 0, N)
        de = chunked.latent_step_chunked(q, 0, N, chunk=chunk)
        assert torch.equal(de, de_ref)
        assert all(torch.equal(a, b) for a, b in zip(state(one), state(chunked)))
        assert (one.noise_step, one.emb_step) == (chunked.noise_step, chunked.emb_step)
    # a sub-range, as a rank's shard is
    _, de_ref = one.latent_step(2, 5, 17)
    assert torch.equal(chunked.latent_step_chunked(2, 5, 17, chunk=chunk), de_ref) and torch.equal(one.emb, chunked.emb)


def test_default_chunk_is_the_measured_resident_batch(gpu):
    import inspect
    from nvfpcc_amd import engine
    assert engine.LATENT_CHUNK == 4096
    assert inspect.signature(engine.TrainEngine.latent_step_chunked).parameters["chunk"].default == 4096
    with pytest.raises(ValueError):
        make("S", gpu, 2)[1].latent_step_chunked(2, chunk=0)


def test_eval_sums_in_chunks_of_7(gpu, monkeypatch):
    from nvfpcc_amd import engine
    _, eng = make("S", gpu, N)[:2]
    whole = eng.eval_sums()
    monkeypatch.setattr(engine, "LATENT_CHUNK", 24)
    assert torch.equal(eng.eval_sums(), whole)          # a chunk that holds the shard: the single pass, its bits
    monkeypatch.setattr(engine, "LATENT_CHUNK", 7)
    chunked = eng.eval_sums()
    assert chunked.dtype == whole.dtype == torch.float32 and chunked.shape == whole.shape == (22,)
    w, c = whole.double().cpu().numpy(), chunked.double().cpu().numpy()
    print("whole  ", w.tolist())
    print("chunked", c.tolist())
    assert w[3:21].min() >= 0 and w[[4, 6, 10, 12, 16, 18]].min() > 0         # occupied and empty voxels at every level
    np.testing.assert_array_equal(c[3:21], w[3:21])
    for k in (0, 1, 2, 21):
        assert w[k] > 0 and abs(c[k] - w[k]) <= TOL * abs(w[k]), (k, c[k], w[k])
    # a sub-range whose length is no multiple of the chunk, and an empty one
    part = eng.eval_sums(3, 20).double().cpu().numpy()
    monkeypatch.setattr(engine, "LATENT_CHUNK", 4096)
    ref = eng.eval_sums(3, 20).double().cpu().numpy()
    np.testing.assert_array_equal(part[3:21], ref[3:21])
    assert all(abs(part[k] - ref[k]) <= TOL * abs(ref[k]) for k in (0, 1, 2, 21))
    assert torch.equal(eng.eval_sums(9, 9), torch.zeros(22, device=gpu))
