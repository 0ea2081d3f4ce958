"""The lossless occupancy coder on the device (csrc/occ_rans.hip through nvfpcc_amd.ops) against the numpy reference
(tests/occ_rans_ref.py): histogram, encoder and decoder are integer arithmetic and must agree exactly.  Blocks are
32^3; 1 to 5 of them, so the suite spends seconds here."""
import numpy as np
import pytest
import torch

from tests import occ_rans_ref as R
from tests.test_lossless_cpu import adversarial_p

pytestmark = pytest.mark.gpu
VOX = 32768


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def cloud():
    """Five blocks of adversarial probabilities (exactly 0, 1 and 0.5, denormals, -0.0, the whole exponent range), an
    all-empty and an all-full block among them; left unchanged by every test."""
    rng = np.random.default_rng(11)
    p = adversarial_p(rng, 5)
    gt = rng.random(p.shape) < np.where(p > 0.5, 0.9, 0.1)
    gt[1] = False
    gt[3] = True
    f1 = R.table(*R.histogram(p, gt))
    return p, gt, f1


def to_dev(p, gt, f1, dev):
    shape = (p.shape[0], 1, 32, 32, 32)
    return (torch.from_numpy(p).reshape(shape).to(dev), torch.from_numpy(gt.astype(np.float32)).reshape(shape).to(dev),
            torch.from_numpy(np.asarray(f1, np.int32)).to(dev))


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_histogram_equals_bincount_and_accumulates(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, _ = cloud
    p = p.copy()
    p[0, :7] = [np.nan, -1e-9, 1.0000001, 2.0, -np.inf, np.inf, -0.0]       # six input errors; -0.0 is none
    p[4, 100] = np.nan
    want_cnt, want_occ = R.histogram(p, gt)
    pd, gd, _ = to_dev(p, gt, np.zeros(256), dev)
    cnt, occ, bad = ops.occ_ctx_hist(pd, gd)
    assert np.array_equal(u64(cnt), want_cnt.astype(np.uint64)) and np.array_equal(u64(occ), want_occ.astype(np.uint64))
    assert int(bad.item()) == 7 == int(R.bad(p).sum())
    # streamed: two calls into the same sums
    acc = ops.occ_ctx_hist(pd[:2].contiguous(), gd[:2].contiguous())
    acc = ops.occ_ctx_hist(pd[2:].contiguous(), gd[2:].contiguous(), *acc)
    assert torch.equal(acc[0], cnt) and torch.equal(acc[1], occ) and torch.equal(acc[2], bad)
    # one saturated block: every voxel in one context
    ones = torch.ones((1, 1, 32, 32, 32), device=dev)
    cnt, occ, bad = ops.occ_ctx_hist(ones, ones)
    assert int(cnt[255]) == VOX == int(occ[255]) and int(cnt.sum()) == VOX and int(bad.item()) == 0


def check_against_reference(dev, p, gt, f1, group):
    from nvfpcc_amd import ops
    pd, gd, fd = to_dev(p, gt, f1, dev)
    states, words, gt_words = ops.occ_rans_encode(pd, gd, fd, group)
    ref = R.encode(p, gt, f1, group)
    assert states.shape == (len(ref), 64) and len(words) == len(ref)
    for g, (s, w) in enumerate(ref):
        assert np.array_equal(u64(states[g]), s), (group, g)
        assert np.array_equal(u32(words[g]), w), (group, g)
    assert np.array_equal(u64(gt_words), R.occupancy_words(gt))
    nwords = torch.tensor([w.numel() for w in words], dtype=torch.int32, device=dev)
    flat = torch.cat(words) if words else torch.zeros(0, dtype=torch.int32, device=dev)
    occ_words, counts, status = ops.occ_rans_decode(pd, fd, states, flat, nwords, group)
    assert status.tolist() == [0] * len(ref)
    assert torch.equal(occ_words, gt_words)
    assert counts.tolist() == gt.reshape(gt.shape[0], -1).sum(1).tolist()
    return states, flat, nwords, occ_words, counts


@pytest.mark.parametrize("blocks", [1, 3, 5])
@pytest.mark.parametrize("group", [1, 2, 64])
def test_encoder_is_byte_identical_and_decoder_inverts_it(dev, cloud, blocks, group):
    p, gt, f1 = cloud
    check_against_reference(dev, p[:blocks], gt[:blocks], f1, group)


def test_table_with_the_extreme_frequencies(dev, cloud):
    """Entries 1 and 65535: the rarest symbol costs 16 bits, the likeliest almost nothing; and symbols that contradict
    such an entry still round-trip."""
    p, gt, _ = cloud
    f1 = np.where(np.arange(256) % 2 == 0, 1, 65535)
    f1[6:10] = [65535, 1, 40000, 3]
    check_against_reference(dev, p[:3], gt[:3], f1, 2)


def test_points_from_bits32_equals_nonzero_in_order(dev, cloud):
    """points_from_bits at d = 32 walks a block's 512 words in chunks of 64: besides the cloud, one block whose only set
    bits lie in words 64..511 (its first chunk is empty and skipped) and one whose bits straddle words 63 / 64."""
    from nvfpcc_amd import ops
    gt = np.concatenate([cloud[1], np.zeros((2, VOX), bool)])
    gt[5, [64 * 64, 64 * 64 + 63, 64 * 200 + 17, 64 * 511, VOX - 1]] = True
    gt[6, 64 * 63 + 60:64 * 64 + 5] = True
    g = torch.from_numpy(gt).reshape(7, 32, 32, 32).to(dev)
    words = torch.from_numpy(R.occupancy_words(gt).view(np.int64)).to(dev)
    assert not words[5, :64].any() and words[6, 63] != 0 and words[6, 64] != 0
    counts = g.reshape(7, -1).sum(1).to(torch.int32)
    origins = torch.tensor([[0, 0, 0], [32, 64, 96], [992, 0, 4064], [2048, 32, 32], [4064, 4064, 4064], [64, 32, 0],
                            [0, 96, 128]], dtype=torch.int32, device=dev)
    nz = torch.nonzero(g)
    want = nz[:, 1:].to(torch.int32) + origins[nz[:, 0]]
    got = ops.points_from_bits(words, counts, origins, 32, 0)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert torch.equal(ops.points_from_bits(words, counts, None, 32, 0), nz[:, 1:].to(torch.int32))
    # a block without points in the middle, and a single block
    assert int(counts[1]) == 0 and int(counts[3]) == VOX
    assert torch.equal(ops.points_from_bits(words[2:3].contiguous(), counts[2:3].contiguous(), origins[2:3].contiguous(), 32, 0),
                       want[int(counts[:2].sum()):int(counts[:3].sum())])


def test_damaged_streams_raise_and_the_next_good_stream_decodes(dev, cloud):
    """The decoder's bounds logic, with well-formed launches: a flipped word, a truncated word list and a word count
    that is too large each end in a non-zero status (ValueError through lossless_pack.check_status), and the process
    goes on to decode the good stream."""
    from nvfpcc_amd import lossless_pack as lp, ops
    p, gt, f1 = cloud
    group = 2
    pd, gd, fd = to_dev(p, gt, f1, dev)
    states, flat, nwords, good_words, good_counts = check_against_reference(dev, p, gt, f1, group)
    assert flat.numel() > 64

    def decode(words, nw):
        out = ops.occ_rans_decode(pd, fd, states, words, nw, group)
        torch.cuda.synchronize()
        return out

    def good():
        w, c, s = decode(flat, nwords)
        lp.check_status(s.cpu().numpy())
        assert torch.equal(w, good_words) and torch.equal(c, good_counts)

    flipped = flat.clone()
    flipped[5] ^= 0x00010000
    _, _, s = decode(flipped, nwords)
    assert s[0].item() != 0 and s[1:].tolist() == [0, 0]          # the other groups read their own words
    with pytest.raises(ValueError, match="group 0 is damaged"):
        lp.check_status(s.cpu().numpy())
    good()

    # the word list cut short: the last group wants words beyond the buffer and gets zeros
    cut = flat[:flat.numel() - 9].contiguous()
    _, _, s = decode(cut, nwords)
    assert s[:2].tolist() == [0, 0] and s[2].item() & ops.OCC_RANS_PAST_END
    with pytest.raises(ValueError, match="group 2 is damaged.*past the end"):
        lp.check_status(s.cpu().numpy())
    good()

    # a word count too large: group 0 ends with words left over, and the groups behind it start in the wrong place
    more = nwords.clone()
    more[0] += 3
    _, _, s = decode(flat, more)
    assert s[0].item() == ops.OCC_RANS_WORDS_LEFT and all(v != 0 for v in s.tolist())
    with pytest.raises(ValueError, match="group 0 is damaged \\(words left over\\)"):
        lp.check_status(s.cpu().numpy())
    huge = nwords.clone()
    huge[2] = 2 ** 31 - 1
    _, _, s = decode(flat, huge)
    assert s[:2].tolist() == [0, 0] and s[2].item() & ops.OCC_RANS_PAST_END
    good()

    # no words at all, and damaged states
    _, _, s = decode(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros_like(nwords))
    assert all(v & ops.OCC_RANS_PAST_END for v in s.tolist())
    bad_states = states.clone()
    bad_states[1, 17] ^= 1 << 40
    _, _, s = ops.occ_rans_decode(pd, fd, bad_states, flat, nwords, group)
    assert s[0].item() == 0 and s[1].item() != 0
    good()


def test_occupancy_round_trip_through_the_pack(dev):
    """encode_occupancy / decode_occupancy on a real decoder: batches that do not divide the cloud, a group size that
    does not divide the batch, coder launches of one group and of all of them, bytes in, words and points out; and a flipped byte of the stream raises."""
    from nvfpcc_amd import lossless_pack as lp, network
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False).to(dev)
    g = torch.Generator().manual_seed(5)
    lat = torch.round(2.0 * torch.randn(5, 3, 2, 2, 2, generator=g)).to(dev)
    gts = make_blocks(5)[0]
    gt = torch.from_numpy(gts).float().to(dev)
    want_words = R.occupancy_words(gts.reshape(5, -1))
    packs = {}
    for batch, group in ((2, 2), (3, 1), (5, 64)):
        data, info = lp.encode_occupancy(net, lat, gt, batch=batch, group=group, span_groups=1)
        side = lp.read(data, 5)
        assert side["group"] == group and len(data) == lp.size(5, group, int(side["nwords"].sum()))
        assert np.array_equal(u64(info["gt_words"]), want_words)
        # the same table whatever the batch; the device's sums are the reference's on the device's own p
        with torch.no_grad():
            p = net.reconstruct(lat, 2).reshape(5, -1).cpu().numpy()
        cnt, occ = R.histogram(p, gts.reshape(5, -1))
        assert side["f1"].tolist() == R.table(cnt, occ).tolist()
        ref = R.encode(p, gts.reshape(5, -1), side["f1"], group)
        assert np.array_equal(side["states"], np.stack([s for s, _ in ref]))
        assert np.array_equal(side["words"], np.concatenate([w for _, w in ref]))
        packs[group] = data
        for dec_batch in (1, 4):
            words, counts = lp.decode_occupancy(net, lat, data, batch=dec_batch, span_groups=1 if dec_batch == 1 else 8)
            assert np.array_equal(u64(words), want_words)
            assert counts.tolist() == gts.reshape(5, -1).astype(bool).sum(1).tolist()
    pts = lp.points_from_words(words, counts, np.arange(15).reshape(5, 3) * 32, batch=2)
    nz = np.argwhere(gts.reshape(5, 32, 32, 32))
    assert np.array_equal(pts, nz[:, 1:] + (np.arange(15).reshape(5, 3) * 32)[nz[:, 0]])
    data = bytearray(packs[2])
    data[-3] ^= 0x10
    with pytest.raises(ValueError, match="group 2 is damaged"):
        lp.decode_occupancy(net, lat, bytes(data), batch=2)
    with pytest.raises(ValueError, match="codes 5 blocks"):
        lp.decode_occupancy(net, lat[:4], packs[2], batch=2)
    words, _ = lp.decode_occupancy(net, lat, packs[2], batch=2)
    assert np.array_equal(u64(words), want_words)
    bad = gt.clone()
    with pytest.raises(ValueError, match="5 latents and 4 blocks"):
        lp.encode_occupancy(net, lat, bad[:4], batch=2, group=2)
