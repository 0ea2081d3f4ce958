"""The scalable lossless coder under the neighbour contexts on the device (csrc/occ_hier.hip through nvfpcc_amd.ops)
against the numpy reference (tests/occ_nbr_ref.py): histogram, encoder and decoder must agree exactly.  p is handed to
the kernels directly.  Five 32^3 blocks -- a surface, an empty block, a sparse random one with voxels on every face and
corner, a full block, another surface -- in groups of 1, 2 and 64: a lone block, a short last group, a batch that is no
multiple of the group, empty and full neighbours whose 16^3 cells must not be seen from the block next to them."""
import numpy as np
import pytest
import torch

from tests import occ_hier_ref as H
from tests import occ_nbr_ref as N
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
    """p, gt, the reference's counts, table and streams at every group size; left unchanged by every test."""
    from nvfpcc_amd.synth import make_blocks
    rng = np.random.default_rng(23)
    p = adversarial_p(rng, 5)
    gt = np.zeros(p.shape, bool)
    surf = make_blocks(2)[0].reshape(2, -1).astype(bool)
    gt[0], gt[4] = surf[0], surf[1]
    seeds = rng.integers(0, 32, (1500, 3))
    gt[2, (seeds[:, 0] * 32 + seeds[:, 1]) * 32 + seeds[:, 2]] = True
    for z in (0, 31):                                             # the eight corners, and a voxel inside each face
        for y in (0, 31):
            for x in (0, 31):
                gt[2, (z * 32 + y) * 32 + x] = True
    for axis in range(3):
        for side in (0, 31):
            v = [13, 18, 7]
            v[axis] = side
            gt[2, (v[0] * 32 + v[1]) * 32 + v[2]] = True
    gt[3] = True
    cnt, occ = N.histogram(p, gt)
    f1 = N.table(cnt, occ)
    ref = {group: N.encode(p, gt, f1, group) for group in (1, 2, 64)}
    return p, gt, cnt, occ, f1, ref


def to_dev(p, gt, f1, dev):
    shape = (p.shape[0], 1, 32, 32, 32)
    return (torch.from_numpy(p).reshape(shape).to(dev), torch.from_numpy(gt.astype(np.float32)).reshape(shape).to(dev),
            torch.from_numpy(np.asarray(f1, np.int32)).to(dev))


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_the_cloud_covers_what_it_is_built_for(cloud):
    p, gt, cnt, _, _, _ = cloud
    g1 = H.maxpool(gt)[1]
    per_block = 8 * g1.sum(1)
    assert per_block.tolist()[1] == 0 and per_block.tolist()[3] == VOX
    # section 0 is no multiple of 64 symbols for a lone block, a pair and the whole cloud: the last step has idle lanes
    assert per_block[0] % 64 and per_block[4] % 64 and (per_block[0] + per_block[1]) % 64 and per_block.sum() % 64
    classes = np.flatnonzero(cnt[3072:].reshape(32, 1024).sum(1))
    assert classes[0] == 0 and classes[-1] == 31 and classes.size >= 24


def test_histogram_equals_the_references_integers_and_accumulates(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, want_cnt, want_occ, _, _ = cloud
    pd, gd, _ = to_dev(p, gt, np.zeros(1), dev)
    cnt, occ = ops.occ_nbr_hist(ops.occ_hier_pyramid(pd, gd))
    assert cnt.shape == (35840,) == want_cnt.shape
    assert np.array_equal(u64(cnt), want_cnt.astype(np.uint64)) and np.array_equal(u64(occ), want_occ.astype(np.uint64))
    # levels 1 and 2 are the field coder's counts, level 0 is its counts spread over the classes
    hc, ho = ops.occ_hier_hist(ops.occ_hier_pyramid(pd, gd))
    assert torch.equal(cnt[1024:3072], hc[1024:]) and torch.equal(occ[1024:3072], ho[1024:]) and not cnt[:1024].any()
    assert torch.equal(cnt[3072:].reshape(32, 1024).sum(0), hc[:1024]) and torch.equal(occ[3072:].reshape(32, 1024).sum(0), ho[:1024])
    acc = ops.occ_nbr_hist(ops.occ_hier_pyramid(pd[:2].contiguous(), gd[:2].contiguous()))
    acc = ops.occ_nbr_hist(ops.occ_hier_pyramid(pd[2:].contiguous(), gd[2:].contiguous()), *acc)
    assert torch.equal(acc[0], cnt) and torch.equal(acc[1], occ)


def test_histogram_of_a_block_that_fills_one_context(dev):
    """A full block under a constant p: all 30^3 inner voxels fall into ONE context (n = 31, k = 3), symbols and
    occupied ones alike, which is as far as a block can push a counter (at most 32768); twice, to see the sums go on."""
    from nvfpcc_amd import ops
    p = np.full((2, VOX), 0.9, np.float32)
    gt = np.ones((2, VOX), bool)
    want_cnt, want_occ = N.histogram(p, gt)
    top = 3072 + (31 * 4 + 3) * 256 + int(N.R.contexts(np.asarray([0.9], np.float32))[0])
    assert want_cnt[top] == want_occ[top] == 2 * 30 ** 3 and np.count_nonzero(want_cnt[3072:]) == 4    # inside, faces, edges, corners
    pd, gd, _ = to_dev(p, gt, np.zeros(1), dev)
    cnt, occ = ops.occ_nbr_hist(ops.occ_hier_pyramid(pd, gd))
    assert np.array_equal(u64(cnt), want_cnt.astype(np.uint64)) and np.array_equal(u64(occ), want_occ.astype(np.uint64))


def check_against_reference(dev, p, gt, f1, group, ref):
    from nvfpcc_amd import ops
    pd, gd, fd = to_dev(p, gt, f1, dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    states, words = ops.occ_nbr_encode(pyr, fd, group)
    assert states.shape == (len(ref), 64) and len(words) == len(ref)
    for g, (s, w) in enumerate(ref):
        assert words[g].numel() == w.size <= min(group, p.shape[0] - g * group) * N.BLOCK_WORDS, (group, g)
        assert np.array_equal(u64(states[g]), s), (group, g)
        assert np.array_equal(u32(words[g]), w), (group, g)
    nwords = torch.tensor([w.numel() for w in words], dtype=torch.int32, device=dev)
    flat = torch.cat(words)
    dec = ops.occ_hier_pyramid(pd)                               # the decoder's side: no ground truth
    pools = H.maxpool(gt)
    used = {}
    for level in (0, 1, 2):
        occ_words, counts, status, pos = ops.occ_nbr_decode(dec, fd, states, flat, nwords, group, level)
        assert status.tolist() == [0] * len(ref), level
        assert occ_words.shape == (p.shape[0], 512 >> 3 * level)
        assert np.array_equal(u64(occ_words), H.words_of(pools[level])), level
        assert counts.tolist() == pools[level].sum(1).tolist()
        used[level] = pos.tolist()
    assert used[0] == nwords.tolist()
    for g in range(len(ref)):                                    # the coarse levels read what the reference reads: a prefix
        sl = slice(g * group, (g + 1) * group)
        for level in (1, 2):
            assert used[level][g] == N.decode_group(p[sl], f1, ref[g][0], ref[g][1], stop=level)[2] <= used[0][g]
    return states, flat, nwords, dec


@pytest.mark.parametrize("group", [1, 2, 64])
def test_encoder_is_byte_identical_and_decoder_inverts_it_at_every_level(dev, cloud, group):
    p, gt, _, _, f1, ref = cloud
    check_against_reference(dev, p, gt, f1, group, ref[group])


def test_the_full_block_under_the_costliest_table_stays_inside_its_region(dev, cloud):
    """Every symbol of the all-full block is a 1; under f1 = 1 each costs 16 bits, a word for every second symbol, the
    most a table can ask of a block: 37376 symbols, the per-block bound in words, of which the stream takes half (the
    64 states hold the rest).  The sparse blocks beside it run under the same table."""
    p, gt, _, _, _, _ = cloud
    f1 = np.ones(35840, np.int64)
    ref = N.encode(p[2:5], gt[2:5], f1, 1)
    assert 37376 // 2 - 64 <= ref[1][1].size <= 37376 // 2
    check_against_reference(dev, p[2:5], gt[2:5], f1, 1, ref)


def test_damaged_streams_end_in_a_status_and_raise(dev, cloud):
    from nvfpcc_amd import lossless_nbr_pack as lp, ops
    p, gt, _, _, f1, ref = cloud
    group = 2
    states, flat, nwords, dec = check_against_reference(dev, p, gt, f1, group, ref[group])
    fd = torch.from_numpy(np.asarray(f1, np.int32)).to(dev)
    want = torch.from_numpy(H.words_of(H.maxpool(gt)[0]).view(np.int64)).to(dev)

    def decode(st, words, nw, level=0):
        out = ops.occ_nbr_decode(dec, fd, st, words, nw, group, level)
        torch.cuda.synchronize()
        return out

    def good():
        w, c, s, _ = decode(states, flat, nwords)
        lp.check_status(s.cpu().numpy())
        assert torch.equal(w, want) and c.tolist() == gt.sum(1).tolist()

    # where the sections of groups 0 and 1 end, from the reference: the flips below aim at a section each
    coarse = [N.decode_group(p[2 * g:2 * g + 2], f1, *ref[group][g], stop=1)[2] for g in (0, 1)]
    assert N.decode_group(p[:2], f1, *ref[group][0], stop=2)[2] > 4 and coarse[1] < int(nwords[1]) - 40 and int(nwords[2]) > 9
    cut = flat[:flat.numel() - 9].contiguous()                   # truncated: the last group wants words beyond the buffer
    _, _, s, _ = decode(states, cut, nwords)
    assert s[:2].tolist() == [0, 0] and s[2].item() & ops.OCC_RANS_PAST_END
    with pytest.raises(ValueError, match="lossless_lod_pack: the stream of group 2 is damaged.*past the end"):
        lp.check_status(s.cpu().numpy())
    good()
    flipped = flat.clone()                                       # a flipped bit in the level-0 part of group 1
    at = int(nwords[0]) + int(nwords[1]) - 40
    flipped[at] ^= 0x00010000
    _, _, s, _ = decode(states, flipped, nwords)
    assert s[0].item() == 0 and s[1].item() != 0 and s[2].item() == 0
    with pytest.raises(ValueError, match="group 1 is damaged"):
        lp.check_status(s.cpu().numpy())
    _, _, s, _ = decode(states, flipped, nwords, level=1)        # the coarse sections lie before it
    assert s.tolist() == [0, 0, 0]
    flipped = flat.clone()                                       # and one in the 8^3 section of group 0: any 16^3 cells follow
    flipped[3] ^= 0x00010000
    _, _, s, _ = decode(states, flipped, nwords)
    assert s[0].item() != 0 and s[1:].tolist() == [0, 0]
    bad_states = states.clone()
    bad_states[2, 63] ^= 1 << 40
    _, _, s, _ = decode(bad_states, flat, nwords)
    assert s[:2].tolist() == [0, 0] and s[2].item() != 0
    _, _, s, _ = decode(states, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros_like(nwords))
    assert all(v & ops.OCC_RANS_PAST_END for v in s.tolist())
    good()


def test_refusals_of_the_wrappers(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, _, _, f1, _ = cloud
    pd, gd, fd = to_dev(p[:1], gt[:1], f1, dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    with pytest.raises(RuntimeError, match="f1 must be int32 \\[35840\\]"):
        ops.occ_nbr_encode(pyr, fd[:3072].contiguous(), 1)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.occ_nbr_encode(pyr, torch.cat([fd[:1], fd])[1:], 1)
    with pytest.raises(RuntimeError, match="cnt and occ are int64 \\[35840\\]"):
        ops.occ_nbr_hist(pyr, *(torch.zeros(3072, dtype=torch.int64, device=dev) for _ in range(2)))


def test_occupancy_round_trip_through_the_pack(dev):
    """encode_occupancy / decode_occupancy on a real decoder: the device's pack is the reference's on the device's own
    p, decodes at the three levels at other batches, and is told from the field contexts' pack by its first byte."""
    from nvfpcc_amd import lossless_lod_pack as llp, lossless_nbr_pack as lp, network
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
    cnt, occ = N.histogram(p, gts)
    packs = {}
    for batch, group in ((1, 2), (7, 64)):
        data, info = lp.encode_occupancy(net, lat, gt, batch=batch, group=group, span_groups=1)
        assert data[0] == 3 and lp.module_of(data) is lp
        side = lp.read(data, 5)
        assert side["group"] == group
        assert len(data) == lp.size(5, group, int(side["nwords"].sum()), info["contexts"], info["slots0"])
        assert info["symbols"] == int(cnt.sum()) and info["contexts"] == int((cnt > 0).sum()) == int(side["used"].sum())
        assert side["f1"].tolist() == N.table(cnt, occ).tolist()
        ref = N.encode(p, gts, side["f1"], group)
        assert np.array_equal(side["states"], np.stack([s for s, _ in ref]))
        assert np.array_equal(side["words"], np.concatenate([w for _, w in ref]))
        packs[group] = data
        for level in (0, 1, 2):
            assert np.array_equal(u64(info["gt_words"][level]), H.words_of(pools[level]))
            words, counts = lp.decode_occupancy(net, lat, data, level=level, batch=8 - batch, span_groups=1)
            assert np.array_equal(u64(words), H.words_of(pools[level])), (batch, level)
            assert counts.tolist() == pools[level].sum(1).tolist()
    field, _ = llp.encode_occupancy(net, lat, gt, batch=7, group=2)
    assert field[0] == 1 and lp.module_of(field) is llp
    with pytest.raises(ValueError, match="version 3, this reader knows 1"):
        llp.decode_occupancy(net, lat, packs[2], batch=2)
    data = bytearray(packs[2])
    data[-3] ^= 0x10
    with pytest.raises(ValueError, match="lossless_lod_pack: the stream of group 2 is damaged"):
        lp.decode_occupancy(net, lat, bytes(data), batch=2)
    with pytest.raises(ValueError, match="codes 5 blocks"):
        lp.decode_occupancy(net, lat[:4], packs[2], batch=2)
    with pytest.raises(ValueError, match="level 3"):
        lp.decode_occupancy(net, lat, packs[2], level=3)
