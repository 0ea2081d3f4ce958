"""The decode route holds the occupancy probabilities p of a block to ONE set of float32 bits, whatever batch the block
is decoded in and wherever it sits in that batch.  rc_enc.ply == rc_dec.ply, the thresholds and counts of thh_pack,
decode --lod and above all --lossless (rANS contexts are cut from the bits of p) rest on it, and --batchsize is chosen
freely and separately for encode and decode.

The library picks kernels by batch inside that route: nvf_convT3d_k5s2_fwd and nvf_conv3d_gather (csrc/conv_direct.hip)
change tile instantiations between 64 and 65 blocks, and the engine's _conv / _dx_convT pick matrix-core variants by
batch.  So every test here straddles 64 | 65:

  1. op level    the kernels picked at 64 and at 65 blocks against the one-thread-per-output kernels, against batch 1,
                 and against guard bands around the output (an edge tile that overruns the last block);
  2. net level   Net.reconstruct at EVERY batch from 1 to 130 (and 257) against batch 1, four decoders; the full forward,
                 the level-of-detail forward and the engine's eval forward at 66 blocks;
  3. product     recon.reconstruct_points (float threshold, per-block counts, lod) and the lossless round trip with
                 encode and decode batches on either side of the switch.

Every comparison is bit equality: no tolerance anywhere.  The one-thread-per-output kernels are pinned to torch by
tests/test_gpu_ops.py at batch 2, so no float64 reference is needed here."""
import numpy as np
import pytest
import torch

from nvfpcc_amd.seeds import synthetic_seed
from nvfpcc_amd.synth import make_blocks, make_origins
from tests import occ_rans_ref as R
from tests.golden_inputs import CONFIGS, make_emb, perturb_state_
from tests.test_gpu_ops import CONVT_CASES

pytestmark = pytest.mark.gpu
GUARD = 4096                    # floats before and after an output written through out=
NAN_BITS = 0x7FC0BEEF           # a quiet NaN with a payload no kernel produces
SWITCH = (64, 65)               # the last batch of the small-batch kernels and the first of the large-batch ones
N_SWEEP, N_PRODUCT, N_BEYOND = 130, 66, 257

# tag -> (latent channels, channel string, seed of perturb_state_): BASELINE's two decoders (tests/golden_inputs.py), the
# reference's default (--ch 8 with the narrow string) and a string off the tuned tables (generic kernels throughout)
DECODERS = {"S": (CONFIGS["S"]["ch"], CONFIGS["S"]["channels"], CONFIGS["S"]["param_seed"]),
            "W": (CONFIGS["W"]["ch"], CONFIGS["W"]["channels"], CONFIGS["W"]["param_seed"]),
            "default": (8, (8, 16, 8, 8), 121),
            "offgrid": (4, (4, 8, 4, 4), 131)}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def ops(gpu):
    from nvfpcc_amd import ops as _ops
    return _ops


# ---------------------------------------------------------------- 1. op level
def guarded(shape, dev):
    """A float32 view of `shape` inside a larger buffer pre-filled with NAN_BITS: GUARD floats before it and after it
    (the offset, 16 KiB, keeps the 256-byte alignment of the allocation)."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device=dev)
    view = buf.view(torch.float32)[GUARD:GUARD + n].view(shape)
    assert view.data_ptr() % 256 == 0 and view.is_contiguous()
    return buf, view


def check_both_sides_of_the_switch(ops, call, inputs, out_shape, B, what):
    """call(out=, **inputs) -> y.  (a) the default dispatch equals the one-thread-per-output kernel at the same batch;
    (b) blocks 0 and B - 1 alone, at batch 1, equal their rows; (c) the launch wrote nothing outside its output."""
    dev = next(t for t in inputs.values() if t is not None).device
    buf, view = guarded((B,) + tuple(out_shape), dev)
    try:
        ops.set_naive(False)
        y = call(out=view, **inputs)
        ops.set_naive(True)
        y_naive = call(out=None, **inputs)
    finally:
        ops.set_naive(False)
    assert y.data_ptr() == view.data_ptr()
    lo, hi = buf[:GUARD], buf[GUARD + view.numel():]
    assert bool((lo == NAN_BITS).all()), f"{what} B={B}: wrote in front of its output"
    assert bool((hi == NAN_BITS).all()), f"{what} B={B}: wrote past the end of its output"
    assert not bool((buf[GUARD:GUARD + view.numel()] == NAN_BITS).any()), f"{what} B={B}: left outputs unwritten"
    assert torch.equal(y, y_naive), f"{what} B={B}: tiled and one-thread-per-output kernels differ"
    for b in (0, B - 1):
        one = call(out=None, **{k: (None if v is None else v[b:b + 1].contiguous()) for k, v in inputs.items()})
        assert torch.equal(one[0], y[b]), f"{what}: block {b} of batch {B} differs from the same block at batch 1"


@pytest.mark.parametrize("B", SWITCH)
@pytest.mark.parametrize("cin,cout,pad,opad,n", CONVT_CASES)
def test_transposed_conv_kernels_on_either_side_of_64_blocks(ops, gpu, cin, cout, pad, opad, n, B):
    """ops.convT3d_k5s2_fwd, ReLU + bias, the decoders' eight layer shapes (the variant is keyed on the extents)."""
    g = torch.Generator().manual_seed(900 + cin * 100 + cout + pad)
    x = torch.randn(B, cin, n, n, n, generator=g).to(gpu)
    w = (torch.randn(cin, cout, 5, 5, 5, generator=g) / (cin * 125 / 8) ** 0.5).to(gpu)
    bias = torch.randn(cout, generator=g).to(gpu)
    wf, _ = ops.pack_convT_weight(w, want_bwd=False)
    no = 2 * n + (3 if pad == 0 else 0)

    def call(x, out):
        return ops.convT3d_k5s2_fwd(x, wf, bias, cout, pad, ops.ACT_RELU, out=out)

    check_both_sides_of_the_switch(ops, call, {"x": x}, (cout, no, no, no), B, f"convT {cin}->{cout} {n}^3")


# (name, cin, cout, k, stride, pad, extent in, extent out, backward-data form): cin / cout as nvf_conv3d_gather sees them
GATHER_CASES = [
    ("conv2 forward", 8, 8, 4, 1, 0, 35, 32, False),
    ("conv1 forward", 8, 8, 4, 1, 0, 19, 16, False),
    ("conv2 backward-data", 8, 8, 4, 1, 3, 32, 35, True),
    ("conv1 backward-data", 8, 8, 4, 1, 3, 16, 19, True),
    ("wide conv2 forward", 16, 16, 4, 1, 0, 35, 32, False),
    ("wide conv2 backward-data", 16, 16, 4, 1, 3, 32, 35, True),
    ("up2 backward-data", 8, 8, 5, 2, 0, 35, 16, True),
    ("up1 backward-data", 8, 16, 5, 2, 0, 19, 8, True),
    ("conv0 backward-data", 16, 8, 5, 2, 2, 8, 4, True),
]


@pytest.mark.parametrize("B", SWITCH)
@pytest.mark.parametrize("name,cin,cout,k,stride,pad,n,no,bwd", GATHER_CASES, ids=[c[0].replace(" ", "_") for c in GATHER_CASES])
def test_gather_conv_kernels_on_either_side_of_64_blocks(ops, gpu, name, cin, cout, k, stride, pad, n, no, bwd, B):
    """ops.conv3d_gather: the forward forms with ReLU + bias, the backward-data forms with an addend and a ReLU mask
    (relu(randn): about half its entries are exactly 0, as a real mask's are)."""
    g = torch.Generator().manual_seed(7000 + cin * 100 + cout * 10 + k + n)
    x = torch.randn(B, cin, n, n, n, generator=g).to(gpu)
    w = (torch.randn(cin * k ** 3 * cout, generator=g) / (cin * k ** 3 / stride ** 3) ** 0.5).to(gpu)   # packed [cin][k^3][cout]
    shape = (cout, no, no, no)
    if bwd:
        bias, act = None, ops.ACT_NONE
        addend = torch.randn((B,) + shape, generator=g).to(gpu)
        mask = torch.relu(torch.randn((B,) + shape, generator=g)).to(gpu)
    else:
        bias, act = torch.randn(cout, generator=g).to(gpu), ops.ACT_RELU
        addend = mask = None

    def call(x, addend, mask, out):
        return ops.conv3d_gather(x, w, bias, cout, k, stride, pad, (no, no, no), act, addend=addend, mask=mask, out=out)

    check_both_sides_of_the_switch(ops, call, {"x": x, "addend": addend, "mask": mask}, shape, B, name)


# ---------------------------------------------------------------- 2. net level
_DECODERS = {}


def decoder(tag, gpu):
    """(net, latents [N_BEYOND, ch, 2, 2, 2] on the device, p of the first N_SWEEP blocks decoded ONE AT A TIME): built
    once per module, left unchanged by every test."""
    if tag not in _DECODERS:
        from nvfpcc_amd import network
        from nvfpcc_amd.model import Net
        ch, channels, seed = DECODERS[tag]
        g = torch.Generator().manual_seed(4000 + seed)
        lat = torch.round(2 * torch.randn(N_BEYOND, ch, 2, 2, 2, generator=g)).to(gpu)
        try:
            network.reset_seed(synthetic_seed())
            net = Net(None, "Gaussian", ch, ",".join(str(c) for c in channels), verbose=False)
            sd = net.state_dict()
            perturb_state_(sd, seed)
            net.load_state_dict(sd)
            net = net.to(gpu)
            with torch.no_grad():
                singles = torch.cat([net.reconstruct(lat[i:i + 1].contiguous(), 2) for i in range(N_SWEEP)], 0)
        except NotImplementedError as e:
            _DECODERS[tag] = e
        else:
            _DECODERS[tag] = (net, lat, singles)
    if isinstance(_DECODERS[tag], NotImplementedError):
        pytest.skip(str(_DECODERS[tag]))
    return _DECODERS[tag]


def layer_outputs(net, lat):
    """{layer: output} of one decoder forward, in the order the layers ran."""
    rec, seen, hooks = net.reconstructor, {}, []
    for name in ("activation",) + tuple(rec._order):
        hooks.append(getattr(rec, name).register_forward_hook(lambda m, i, o, name=name: seen.__setitem__(name, o)))
    try:
        with torch.no_grad():
            rec(lat, 2)
    finally:
        for h in hooks:
            h.remove()
    return seen


def first_differing_layer(net, lat, row):
    """The first layer of the decoder whose output for block `row` of `lat` is not the one it gives that block alone."""
    full, one = layer_outputs(net, lat), layer_outputs(net, lat[row:row + 1].contiguous())
    for name, t in full.items():
        if not torch.equal(t[row], one[name][0]):
            return name
    return None


def assert_rows(net, lat, got, want, rows, what):
    """got[r] == want[r] for r in rows, bit for bit; a failure names the first layer that differs."""
    for r in rows:
        if not torch.equal(got[r], want[r]):
            pytest.fail(f"{what}: block {r} of a batch of {lat.shape[0]} differs from the same block decoded alone; "
                        f"first layer that differs: {first_differing_layer(net, lat, r)}")


@pytest.mark.parametrize("tag", list(DECODERS))
def test_reconstruct_gives_the_bits_of_batch_1_at_every_batch_up_to_130(tag, gpu):
    """A dense sweep: it catches a switch point nobody listed."""
    net, lat, singles = decoder(tag, gpu)
    with torch.no_grad():
        for B in range(1, N_SWEEP + 1):
            part = lat[:B].contiguous()
            out = net.reconstruct(part, 2)
            rows = range(B) if B in (64, 65, 66, N_SWEEP) else sorted({0, B - 1})
            assert_rows(net, part, out, singles, rows, f"{tag}: Net.reconstruct")


@pytest.mark.parametrize("tag", ["S", "W"])
def test_reconstruct_at_257_blocks(tag, gpu):
    """Past every threshold of the tuned tables."""
    net, lat, singles = decoder(tag, gpu)
    with torch.no_grad():
        out = net.reconstruct(lat, 2)
        last = net.reconstruct(lat[N_BEYOND - 1:].contiguous(), 2)
    assert out.shape[0] == N_BEYOND
    assert_rows(net, lat, out, singles, (0, 64, N_SWEEP - 1), f"{tag}: Net.reconstruct")
    assert_rows(net, lat, out, {N_BEYOND - 1: last[0]}, (N_BEYOND - 1,), f"{tag}: Net.reconstruct")


@pytest.mark.parametrize("tag", ["S", "W"])
def test_full_forward_at_66_blocks_equals_batch_1(tag, gpu):
    """net(emb, "eval", 2): the output, both coarse heads and the rounded latents."""
    net, _, _ = decoder(tag, gpu)
    emb = make_emb(N_PRODUCT, DECODERS[tag][0], CONFIGS[tag]["emb_seed"]).to(gpu)

    def forward(e):
        out, cls, _, _ = net(e, "eval", 2)
        return {"out": out, "cls0": cls[0], "cls1": cls[1], "rounded": net.entropy_coder(net.latent_gen(e), "eval")[0]}

    with torch.no_grad():
        full = forward(emb)
        for b in range(N_PRODUCT):
            one = forward(emb[b:b + 1].contiguous())
            for k, t in full.items():
                if not torch.equal(one[k][0], t[b]):
                    where = "the latent generator" if k == "rounded" else first_differing_layer(net, full["rounded"], b)
                    pytest.fail(f"{tag}: {k} of block {b} at batch {N_PRODUCT} differs from batch 1; first layer that "
                                f"differs: {where}")


@pytest.mark.parametrize("lod", [1, 2])
@pytest.mark.parametrize("tag", ["S", "W"])
def test_lod_forward_at_66_blocks_equals_batch_1_and_the_full_forwards_heads(tag, lod, gpu):
    net, lat, _ = decoder(tag, gpu)
    lat = lat[:N_PRODUCT].contiguous()
    with torch.no_grad():
        heads = net.reconstructor(lat, 2)[1]
        x, p = net.reconstruct_lod(lat, lod, 2, return_p=True)
        assert torch.equal(p, heads[2 - lod]), f"{tag} lod {lod}: not the bits of the full forward's head"
        for b in range(N_PRODUCT):
            x1, p1 = net.reconstruct_lod(lat[b:b + 1].contiguous(), lod, 2, return_p=True)
            if not (torch.equal(x1[0], x[b]) and torch.equal(p1[0], p[b])):
                pytest.fail(f"{tag} lod {lod}: block {b} at batch {N_PRODUCT} differs from batch 1; first layer that "
                            f"differs: {first_differing_layer(net, lat, b)}")


@pytest.mark.parametrize("tag", ["S", "W"])
def test_engine_eval_forward_at_66_blocks_equals_batch_1(tag, gpu):
    """TrainEngine.eval_forward (fused stem, explicit matrix-core variants chosen by batch) across 64 | 65: for the wide
    decoder tests/test_gpu_engine.py stops at 37 blocks."""
    from tests.test_gpu_engine import make
    net, eng, gt, dist, emb = make(tag, gpu, nblk=N_PRODUCT)
    p_all = {k: v.clone() for k, v in eng.eval_forward(q=2).items() if k in ("p0", "p1", "p2")}
    for b in (0, 63, 64, 65):
        one = eng.eval_forward(lo=b, hi=b + 1, q=2)
        for k, t in p_all.items():
            assert torch.equal(one[k][0], t[b]), f"{tag}: engine eval_forward: {k} of block {b} at batch {N_PRODUCT} differs from batch 1"


# ---------------------------------------------------------------- 3. product level
BATCHES = (66, 65, 64, 1)


@pytest.fixture(scope="module")
def occupancy():
    return make_blocks(N_PRODUCT)[0]


@pytest.mark.parametrize("tag", ["S", "W"])
def test_points_are_the_same_at_batches_on_either_side_of_the_switch(tag, gpu, occupancy):
    """recon.reconstruct_points with one float threshold and with per-block counts (thh_out too), and
    reconstruct_points_lod, at batch 66, 65, 64 and 1."""
    from nvfpcc_amd import recon
    net, lat, _ = decoder(tag, gpu)
    lat = lat[:N_PRODUCT].contiguous()
    origins = make_origins(N_PRODUCT)
    block_counts = occupancy.reshape(N_PRODUCT, -1).astype(bool).sum(1)

    def by_threshold(b):
        pts, counts = recon.reconstruct_points(net, lat, origins, 0.5, batch=b)
        return {"points": pts, "counts": counts}

    def by_counts(b):
        used = []
        pts, counts = recon.reconstruct_points(net, lat, origins, None, batch=b, block_counts=block_counts, thh_out=used)
        return {"points": pts, "counts": counts, "thh_out": torch.cat(used).cpu().numpy().view(np.uint32)}

    def by_lod(lod):
        def run(b):
            pts, counts = recon.reconstruct_points_lod(net, lat, origins, lod, 0.5, batch=b)
            return {"points": pts, "counts": counts}
        return run

    for what, run, grid in (("threshold 0.5", by_threshold, 32), ("block_counts", by_counts, 32), ("lod 1", by_lod(1), 16),
                            ("lod 2", by_lod(2), 8)):
        want = run(BATCHES[0])
        assert want["counts"].shape == (N_PRODUCT,) and want["points"].shape == (int(want["counts"].sum()), 3)
        # (a threshold that keeps every voxel of the cloud, or none, would compare nothing)
        assert 0 < want["counts"].sum() < N_PRODUCT * grid ** 3
        if what == "block_counts":
            assert (want["counts"] >= block_counts).all()
        for b in BATCHES[1:]:
            got = run(b)
            for k, v in want.items():
                assert np.array_equal(got[k], v), f"{tag}, {what}: {k} at batch {b} differ from batch {BATCHES[0]}"


@pytest.mark.parametrize("tag", ["S", "W"])
def test_lossless_round_trip_with_encode_and_decode_batches_across_the_switch(tag, gpu, occupancy):
    """One voxel whose p falls into another context makes the decoder raise or desynchronise: encode at 66, decode at 1, 64 and
    65; encode at 1, decode at 66; and the packs written at encode batch 1, 64 and 66 are the same bytes."""
    from nvfpcc_amd import lossless_pack as lp
    net, lat, _ = decoder(tag, gpu)
    lat = lat[:N_PRODUCT].contiguous()
    gt = torch.from_numpy(occupancy).float().to(gpu)
    rows = occupancy.reshape(N_PRODUCT, -1)
    want_words = R.occupancy_words(rows)
    want_counts = rows.astype(bool).sum(1).tolist()

    def decodes(pack, batch):
        words, counts = lp.decode_occupancy(net, lat, pack, batch=batch)
        assert np.array_equal(words.cpu().numpy().view(np.uint64), want_words), f"{tag}: decode at batch {batch}"
        assert counts.tolist() == want_counts

    packs = {b: lp.encode_occupancy(net, lat, gt, batch=b, group=64)[0] for b in (66, 64, 1)}
    for b in (1, 64, 65):
        decodes(packs[66], b)
    decodes(packs[1], 66)
    assert packs[1] == packs[66] and packs[64] == packs[66], f"{tag}: the pack depends on the encode batch"
