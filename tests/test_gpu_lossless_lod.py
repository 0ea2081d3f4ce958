"""The scalable lossless occupancy coder on the device (csrc/occ_hier.hip through nvfpcc_amd.ops) against the numpy
reference (tests/occ_hier_ref.py): pyramid, cell lists, histogram, encoder and decoder must agree exactly.  Blocks are
32^3; 1, 3 and 5 of them -- a lone block, a short last group, all-empty and all-full neighbours -- so the suite spends
seconds here."""
import numpy as np
import pytest
import torch

from tests import occ_hier_ref as H
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
    """Five blocks of adversarial probabilities (exactly 0, 1 and 0.5, denormals, -0.0, the whole exponent range) over
    a sparse ground truth -- most parents empty, as in a real cloud --, an all-empty and an all-full block among them;
    the reference's table and streams at every group size; left unchanged by every test."""
    rng = np.random.default_rng(11)
    p = adversarial_p(rng, 5)
    gt = np.zeros(p.shape, bool)
    for b, n in ((0, 700), (2, 1500), (4, 300)):
        seeds = rng.integers(0, 32, (n, 3))
        gt[b, (seeds[:, 0] * 32 + seeds[:, 1]) * 32 + seeds[:, 2]] = True
    gt[3] = True
    cnt, occ = H.histogram(p, gt)
    f1 = H.table(cnt, occ)
    ref = {(blocks, group): H.encode(p[:blocks], gt[:blocks], f1, group) for blocks in (1, 3, 5) for group in (1, 2, 64)}
    return p, gt, f1, ref


def to_dev(p, gt, f1, dev):
    shape = (p.shape[0], 1, 32, 32, 32)
    return (torch.from_numpy(p).reshape(shape).to(dev), torch.from_numpy(gt.astype(np.float32)).reshape(shape).to(dev),
            torch.from_numpy(np.asarray(f1, np.int32)).to(dev))


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_pyramid_and_cell_lists_equal_numpy(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, _, _ = cloud
    p = p.copy()
    p[0, :7] = [np.nan, -1e-9, 1.0000001, 2.0, -np.inf, np.inf, -0.0]       # six input errors; -0.0 is none
    p[4, 100] = np.nan
    pd, gd, _ = to_dev(p, gt, np.zeros(3072), dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    want = H.pyramid(p)
    for name, w in zip(("p1", "k1", "p2", "k2"), want):
        got = pyr[name].cpu().numpy()
        assert got.dtype == w.dtype and np.array_equal(got.view(np.uint8), w.view(np.uint8)), name     # bits, NaN included
    assert int(pyr["bad"].item()) == 7
    assert int(ops.occ_hier_pyramid(pd[1:2].contiguous(), None, pyr["bad"])["bad"].item()) == 7     # accumulates; no gt
    pools = H.maxpool(gt)
    for level in range(3):
        assert np.array_equal(u64(pyr["gt_words"][level]), H.words_of(pools[level])), level
    cells2, counts2, cells1, counts1 = pyr["lists"]
    for level, cells, counts in ((2, cells2, counts2), (1, cells1, counts1)):
        blk, cell = np.nonzero(pools[level])
        assert counts.tolist() == pools[level].sum(1).tolist()
        assert cells.numel() == 5 * pools[level].shape[1]
        assert np.array_equal(cells[:blk.size].cpu().numpy(), blk * pools[level].shape[1] + cell), level
    counts0, none = ops.occ_hier_cells(pyr["gt_words"][0], fill=False)
    assert none is None and counts0.tolist() == gt.sum(1).tolist() == [int(gt[0].sum()), 0, int(gt[2].sum()), VOX, int(gt[4].sum())]
    # one block alone, and the all-full one: every cell listed
    counts, cells = ops.occ_hier_cells(pyr["gt_words"][1][3:4].contiguous())
    assert counts.tolist() == [4096] and cells.tolist() == list(range(4096))


def test_histogram_equals_bincount_and_accumulates(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, _, _ = cloud
    want_cnt, want_occ = H.histogram(p, gt)
    pd, gd, _ = to_dev(p, gt, np.zeros(3072), dev)
    cnt, occ = ops.occ_hier_hist(ops.occ_hier_pyramid(pd, gd))
    assert np.array_equal(u64(cnt), want_cnt.astype(np.uint64)) and np.array_equal(u64(occ), want_occ.astype(np.uint64))
    assert int(cnt.sum()) == H.symbols_coded(p, gt) < 5 * VOX
    # streamed: two calls into the same sums
    acc = ops.occ_hier_hist(ops.occ_hier_pyramid(pd[:2].contiguous(), gd[:2].contiguous()))
    acc = ops.occ_hier_hist(ops.occ_hier_pyramid(pd[2:].contiguous(), gd[2:].contiguous()), *acc)
    assert torch.equal(acc[0], cnt) and torch.equal(acc[1], occ)


def check_against_reference(dev, p, gt, f1, group, ref=None):
    from nvfpcc_amd import ops
    pd, gd, fd = to_dev(p, gt, f1, dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    states, words = ops.occ_hier_encode(pyr, fd, group)
    ref = ref or H.encode(p, gt, f1, group)
    assert states.shape == (len(ref), 64) and len(words) == len(ref)
    for g, (s, w) in enumerate(ref):
        assert words[g].numel() == w.size, (group, g)
        assert np.array_equal(u64(states[g]), s), (group, g)
        assert np.array_equal(u32(words[g]), w), (group, g)
    nwords = torch.tensor([w.numel() for w in words], dtype=torch.int32, device=dev)
    flat = torch.cat(words) if words else torch.zeros(0, dtype=torch.int32, device=dev)
    dec = ops.occ_hier_pyramid(pd)                               # the decoder's side: no ground truth
    pools = H.maxpool(gt)
    used = {}
    for level in (0, 1, 2):
        occ_words, counts, status, pos = ops.occ_hier_decode(dec, fd, states, flat, nwords, group, level)
        assert status.tolist() == [0] * len(ref), level
        assert occ_words.shape == (p.shape[0], 512 >> 3 * level)
        assert np.array_equal(u64(occ_words), H.words_of(pools[level])), level
        assert torch.equal(occ_words, pyr["gt_words"][level])
        assert counts.tolist() == pools[level].sum(1).tolist()
        used[level] = pos.tolist()
    assert used[0] == nwords.tolist()
    for g in range(len(ref)):                                    # the coarse levels read what the reference reads: a prefix
        sl = slice(g * group, (g + 1) * group)
        for level in (1, 2):
            assert used[level][g] == H.decode_group(p[sl], f1, ref[g][0], ref[g][1], stop=level)[2] <= used[0][g]
    return states, flat, nwords, dec


@pytest.mark.parametrize("blocks", [1, 3, 5])
@pytest.mark.parametrize("group", [1, 2, 64])
def test_encoder_is_byte_identical_and_decoder_inverts_it_at_every_level(dev, cloud, blocks, group):
    p, gt, f1, ref = cloud
    check_against_reference(dev, p[:blocks], gt[:blocks], f1, group, ref[blocks, group])


def test_table_with_the_extreme_frequencies(dev, cloud):
    """Entries 1 and 65535: the rarest symbol costs 16 bits, the likeliest almost nothing; and symbols that contradict
    such an entry still round-trip."""
    p, gt, _, _ = cloud
    f1 = np.where(np.arange(3072) % 2 == 0, 1, 65535)
    f1[6:10] = [65535, 1, 40000, 3]
    f1[2048 + 254:2048 + 258] = [65535, 1, 1, 65535]
    check_against_reference(dev, p[:3], gt[:3], f1, 2)


def test_damaged_streams_raise_and_the_next_good_stream_decodes(dev, cloud):
    """The decoder's bounds logic, with well-formed launches: truncated words, a changed state, extra words and a word
    count pointing outside the buffer each end in a non-zero status (ValueError through check_status), whatever
    occupancy they decode on the way, and the process goes on to decode the good stream."""
    from nvfpcc_amd import lossless_lod_pack as lp, ops
    p, gt, f1, ref = cloud
    group = 2
    states, flat, nwords, dec = check_against_reference(dev, p, gt, f1, group, ref[5, group])
    fd = torch.from_numpy(np.asarray(f1, np.int32)).to(dev)
    want = torch.from_numpy(H.words_of(H.maxpool(gt)[0]).view(np.int64)).to(dev)
    assert flat.numel() > 64

    def decode(st, words, nw, level=0):
        out = ops.occ_hier_decode(dec, fd, st, words, nw, group, level)
        torch.cuda.synchronize()
        return out

    def good():
        w, c, s, _ = decode(states, flat, nwords)
        lp.check_status(s.cpu().numpy())
        assert torch.equal(w, want) and c.tolist() == gt.sum(1).tolist()

    # the word list cut short: the last group wants words beyond the buffer and gets zeros
    cut = flat[:flat.numel() - 9].contiguous()
    _, _, s, _ = decode(states, cut, nwords)
    assert s[:2].tolist() == [0, 0] and s[2].item() & ops.OCC_RANS_PAST_END
    with pytest.raises(ValueError, match="lossless_lod_pack: the stream of group 2 is damaged.*past the end"):
        lp.check_status(s.cpu().numpy())
    prefix = H.decode_group(p[4:], f1, *ref[5, group][2], stop=2)[2]       # what the 8^3 section of the last group reads
    _, _, s, _ = decode(states, cut, nwords, level=2)
    assert s.tolist() == [0, 0, 0 if prefix <= int(nwords[2]) - 9 else ops.OCC_RANS_PAST_END]
    good()

    # a changed state: the group decodes another occupancy, of any size, and says so
    bad_states = states.clone()
    bad_states[1, 17] ^= 1 << 40
    _, _, s, _ = decode(bad_states, flat, nwords)
    assert s[0].item() == 0 and s[1].item() != 0 and s[2].item() == 0
    with pytest.raises(ValueError, match="group 1 is damaged"):
        lp.check_status(s.cpu().numpy())
    flipped = flat.clone()
    flipped[5] ^= 0x00010000
    _, _, s, _ = decode(states, flipped, nwords)
    assert s[0].item() != 0 and s[1:].tolist() == [0, 0]
    good()

    # extra words: group 0 ends with words left over, and the groups behind it start in the wrong place
    more = nwords.clone()
    more[0] += 3
    _, _, s, _ = decode(states, flat, more)
    assert s[0].item() == ops.OCC_RANS_WORDS_LEFT and all(v != 0 for v in s.tolist())
    with pytest.raises(ValueError, match="group 0 is damaged \\(words left over\\)"):
        lp.check_status(s.cpu().numpy())
    _, _, s, _ = decode(states, flat, more, level=1)             # a stop cannot know: only "past the end" can show there
    assert s[0].item() == 0 and all(v in (0, ops.OCC_RANS_PAST_END) for v in s.tolist())
    good()

    # a word count pointing outside the buffer
    huge = nwords.clone()
    huge[2] = 2 ** 31 - 1
    _, _, s, _ = decode(states, flat, huge)
    assert s[:2].tolist() == [0, 0] and s[2].item() & ops.OCC_RANS_PAST_END
    huge[0] = -1                                                  # 2^32 - 1 words: every later group starts past the end
    _, _, s, _ = decode(states, flat, huge)
    assert all(v & ops.OCC_RANS_PAST_END for v in s.tolist())
    # no words at all
    _, _, s, _ = decode(states, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros_like(nwords))
    assert all(v & ops.OCC_RANS_PAST_END for v in s.tolist())
    good()


def test_occupancy_round_trip_through_the_pack(dev):
    """encode_occupancy / decode_occupancy on a real decoder at batch 1 and 7: batches that do not divide the cloud,
    coder launches of one group and of all of them, bytes in, words and points out at the three levels; the device's
    pack is the reference's on the device's own p; a flipped byte of the stream raises."""
    from nvfpcc_amd import lossless_lod_pack as lp, network
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False).to(dev)
    g = torch.Generator().manual_seed(5)
    lat = torch.round(2.0 * torch.randn(5, 3, 2, 2, 2, generator=g)).to(dev)
    gts = make_blocks(5)[0].reshape(5, -1)
    gt = torch.from_numpy(gts.reshape(5, 1, 32, 32, 32)).float().to(dev)
    pools = H.maxpool(gts)
    with torch.no_grad():
        p = net.reconstruct(lat, 2).reshape(5, -1).cpu().numpy()
    cnt, occ = H.histogram(p, gts)
    packs = {}
    for batch, group in ((1, 2), (7, 64)):
        data, info = lp.encode_occupancy(net, lat, gt, batch=batch, group=group, span_groups=1)
        side = lp.read(data, 5)
        assert side["group"] == group and len(data) == lp.size(5, group, int(side["nwords"].sum()), info["contexts"])
        assert info["symbols"] == int(cnt.sum()) and info["contexts"] == int((cnt > 0).sum()) == int(side["used"].sum())
        for level in range(3):
            assert np.array_equal(u64(info["gt_words"][level]), H.words_of(pools[level]))
        assert side["f1"].tolist() == H.table(cnt, occ).tolist()
        ref = H.encode(p, gts, side["f1"], group)
        assert np.array_equal(side["states"], np.stack([s for s, _ in ref]))
        assert np.array_equal(side["words"], np.concatenate([w for _, w in ref]))
        packs[group] = data
        for dec_batch in (1, 7):
            for level in (0, 1, 2):
                words, counts = lp.decode_occupancy(net, lat, data, level=level, batch=dec_batch,
                                                    span_groups=1 if dec_batch == 1 else 8)
                assert np.array_equal(u64(words), H.words_of(pools[level])), (batch, dec_batch, level)
                assert counts.tolist() == pools[level].sum(1).tolist()
    origins = np.arange(15).reshape(5, 3) * 32
    for level in (0, 1, 2):
        words, counts = lp.decode_occupancy(net, lat, packs[2], level=level, batch=2)
        pts = lp.points_from_words(words, counts, origins, level, batch=2)
        d = 32 >> level
        nz = np.argwhere(pools[level].reshape(5, d, d, d))
        assert np.array_equal(pts, nz[:, 1:] + (origins >> level)[nz[:, 0]]), level
    data = bytearray(packs[2])
    data[-3] ^= 0x10
    with pytest.raises(ValueError, match="lossless_lod_pack: the stream of group 2 is damaged"):
        lp.decode_occupancy(net, lat, bytes(data), batch=2)
    with pytest.raises(ValueError, match="codes 5 blocks"):
        lp.decode_occupancy(net, lat[:4], packs[2], batch=2)
    with pytest.raises(ValueError, match="level 3"):
        lp.decode_occupancy(net, lat, packs[2], level=3)
    words, _ = lp.decode_occupancy(net, lat, packs[2], batch=2)
    assert np.array_equal(u64(words), H.words_of(pools[0]))
    with pytest.raises(ValueError, match="5 latents and 4 blocks"):
        lp.encode_occupancy(net, lat, gt[:4], batch=2, group=2)
    bad = net.reconstruct
    try:                                                         # an input error in p raises before anything is coded
        net.reconstruct = lambda x, q: bad(x, q) * float("nan")
        with pytest.raises(ValueError, match="probabilities are NaN or outside"):
            lp.encode_occupancy(net, lat, gt, batch=7, group=2)
    finally:
        del net.reconstruct
