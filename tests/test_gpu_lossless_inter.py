"""The scalable lossless coder under the inter contexts on the device (csrc/occ_hier.hip through nvfpcc_amd.ops) against
the numpy reference (tests/occ_inter_ref.py): reference words, histogram, encoder and decoder must agree exactly.  p is
handed to the kernels directly.  The five 32^3 blocks of tests/test_gpu_lossless_nbr.py -- a surface, an empty block, a
sparse random one with voxels on every face and corner, a full block, another surface -- in groups of 1, 2 and 64, each
under a reference of its own: the block moved by a voxel, a full reference over the empty block, an empty one, the
sparse block's voxels under the full block (every corner and face voxel has neighbours outside), the block itself."""
import numpy as np
import pytest
import torch

from tests import occ_hier_ref as H
from tests import occ_inter_ref as I
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
    """p, gt, ref, the reference's counts, table and streams at every group size; left unchanged by every test."""
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
    ref = np.zeros(p.shape, bool)
    ref[0] = I.shifted(gt[:1], 1, 0, 0)[0]
    ref[1] = True
    ref[3] = gt[2]
    ref[4] = gt[4]
    cnt, occ = I.histogram(p, gt, ref)
    f1 = I.table(cnt, occ)
    streams = {group: I.encode(p, gt, ref, f1, group) for group in (1, 2, 64)}
    return p, gt, ref, cnt, occ, f1, streams


def to_dev(p, gt, ref, f1, dev):
    shape = (p.shape[0], 1, 32, 32, 32)
    return (torch.from_numpy(p).reshape(shape).to(dev), torch.from_numpy(gt.astype(np.float32)).reshape(shape).to(dev),
            torch.from_numpy(H.words_of(ref).view(np.int64)).to(dev), torch.from_numpy(np.asarray(f1, np.int32)).to(dev))


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_the_cloud_covers_what_it_is_built_for(cloud):
    p, gt, ref, cnt, _, _, _ = cloud
    per_block = 8 * H.maxpool(gt)[1].sum(1)
    assert per_block.tolist()[1] == 0 and per_block.tolist()[3] == VOX
    assert per_block[0] % 64 and per_block[4] % 64 and (per_block[0] + per_block[1]) % 64 and per_block.sum() % 64
    by_t = cnt[3072:].reshape(48, 1024).sum(1)
    assert all(by_t[r * 16:(r + 1) * 16].sum() > 0 for r in range(3))          # all three temporal classes
    assert np.count_nonzero(by_t) > 24
    # per block: the moved surface has all three, the sparse reference under the full block too, the static block only
    # r = 2 on its points
    blk, cell, ctx = I.group_sections(p, gt, ref)[2][1:4]
    r = (ctx - 3072) // 16384
    assert set(r[blk == 0].tolist()) == {0, 1, 2} and set(r[blk == 3].tolist()) == {0, 1, 2}
    assert set(r[blk == 2].tolist()) == {0} and np.all(r[(blk == 4) & gt[blk, cell]] == 2)


def test_reference_words_equal_the_numpy_words_bit_for_bit(dev):
    from nvfpcc_amd import lossless_inter_pack as lp, ops
    rng = np.random.default_rng(11)
    origins = np.asarray([[4064, 4064, 4064], [0, 0, 0], [32, 4064, 0], [2048, 96, 4032], [0, 0, 32], [64, 0, 0]])   # unsorted
    inside = origins[rng.integers(0, 6, 5000)] + rng.integers(0, 32, (5000, 3))
    outside = np.asarray([[96, 0, 0], [0, 32, 0], [4095, 4095, 4031], [-1, 0, 0], [0, 0, -32], [4096, 4064, 4064],
                          [31, 31, 64], [1 << 26, 0, 0], [0, (1 << 31) - 1, 0], [-(1 << 31), 0, 0]])
    corners = np.asarray([[4095, 4095, 4095], [0, 0, 0], [31, 31, 31], [0, 0, 63], [63, 4095, 31]])
    points = np.concatenate([inside, outside, corners, inside[:700], outside[:3]])
    points = points[rng.permutation(len(points))]
    want, want_dropped = I.reference_words(points, origins)
    assert want_dropped == 13
    pts = torch.from_numpy(points.astype(np.int32)).to(dev)
    org = torch.from_numpy(origins.astype(np.int32)).to(dev)
    words, dropped = ops.occ_ref_words(pts, org)
    assert words.shape == (6, 512) and words.dtype == torch.int64
    assert np.array_equal(u64(words), H.words_of(want)) and dropped.tolist() == [13]
    again, n = lp.reference_words(points, origins, dev)
    assert torch.equal(again, words) and n == 13
    # a lone block, no points, every point dropped
    one, d = ops.occ_ref_words(pts, org[3:4].contiguous())
    assert np.array_equal(u64(one), H.words_of(want[3:4])) and int(d) == len(points) - int(((points - origins[3] >= 0) & (points - origins[3] < 32)).all(1).sum())
    none, d = ops.occ_ref_words(pts[:0], org)
    assert not none.any() and int(d) == 0
    with pytest.raises(RuntimeError, match="points must be int32"):
        ops.occ_ref_words(pts.long(), org)
    with pytest.raises(RuntimeError, match="multiples of 32"):
        ops.occ_ref_words(pts, org + 1)
    with pytest.raises(RuntimeError, match="two blocks share an origin"):
        ops.occ_ref_words(pts, torch.cat([org, org[:1]]))
    with pytest.raises(RuntimeError, match="origins must be int32"):
        ops.occ_ref_words(pts, org[:0])


def test_histogram_equals_the_references_integers_and_accumulates(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, ref, want_cnt, want_occ, _, _ = cloud
    pd, gd, rd, _ = to_dev(p, gt, ref, np.zeros(1), dev)
    cnt, occ = ops.occ_inter_hist(ops.occ_hier_pyramid(pd, gd), rd)
    assert cnt.shape == (52224,) == want_cnt.shape
    assert np.array_equal(u64(cnt), want_cnt.astype(np.uint64)) and np.array_equal(u64(occ), want_occ.astype(np.uint64))
    # levels 1 and 2 are the field coder's counts, level 0 is its counts spread over the classes
    hc, ho = ops.occ_hier_hist(ops.occ_hier_pyramid(pd, gd))
    assert torch.equal(cnt[1024:3072], hc[1024:]) and torch.equal(occ[1024:3072], ho[1024:]) and not cnt[:1024].any()
    assert torch.equal(cnt[3072:].reshape(48, 1024).sum(0), hc[:1024]) and torch.equal(occ[3072:].reshape(48, 1024).sum(0), ho[:1024])
    acc = ops.occ_inter_hist(ops.occ_hier_pyramid(pd[:2].contiguous(), gd[:2].contiguous()), rd[:2].contiguous())
    acc = ops.occ_inter_hist(ops.occ_hier_pyramid(pd[2:].contiguous(), gd[2:].contiguous()), rd[2:].contiguous(), *acc)
    assert torch.equal(acc[0], cnt) and torch.equal(acc[1], occ)


def test_histogram_of_a_block_that_fills_one_context(dev):
    """A full block under a constant p with a full reference: all 30^3 inner voxels fall into ONE context (r = 2,
    s = 15, k = 3), symbols and occupied ones alike: 27000 in each half of the workgroup's counter, no carry; two
    blocks, to see the sums go on."""
    from nvfpcc_amd import ops
    p = np.full((2, VOX), 0.9, np.float32)
    gt = np.ones((2, VOX), bool)
    want_cnt, want_occ = I.histogram(p, gt, gt)
    top = 3072 + ((2 * 16 + 15) * 4 + 3) * 256 + int(I.R.contexts(np.asarray([0.9], np.float32))[0])
    assert want_cnt[top] == want_occ[top] == 2 * 30 ** 3 and np.count_nonzero(want_cnt[3072:]) == 4    # inside, faces, edges, corners
    pd, gd, rd, _ = to_dev(p, gt, gt, np.zeros(1), dev)
    cnt, occ = ops.occ_inter_hist(ops.occ_hier_pyramid(pd[:1].contiguous(), gd[:1].contiguous()), rd[:1].contiguous())
    assert int(cnt[top]) == int(occ[top]) == 27000
    cnt, occ = ops.occ_inter_hist(ops.occ_hier_pyramid(pd, gd), rd)
    assert np.array_equal(u64(cnt), want_cnt.astype(np.uint64)) and np.array_equal(u64(occ), want_occ.astype(np.uint64))


def check_against_reference(dev, p, gt, ref, f1, group, streams):
    from nvfpcc_amd import ops
    pd, gd, rd, fd = to_dev(p, gt, ref, f1, dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    states, words = ops.occ_inter_encode(pyr, rd, fd, group)
    assert states.shape == (len(streams), 64) and len(words) == len(streams)
    for g, (s, w) in enumerate(streams):
        assert words[g].numel() == w.size <= min(group, p.shape[0] - g * group) * I.BLOCK_WORDS, (group, g)
        assert np.array_equal(u64(states[g]), s), (group, g)
        assert np.array_equal(u32(words[g]), w), (group, g)
    nwords = torch.tensor([w.numel() for w in words], dtype=torch.int32, device=dev)
    flat = torch.cat(words)
    dec = ops.occ_hier_pyramid(pd)                               # the decoder's side: no ground truth
    pools = H.maxpool(gt)
    used = {}
    for level in (0, 1, 2):
        occ_words, counts, status, pos = ops.occ_inter_decode(dec, rd, fd, states, flat, nwords, group, level)
        assert status.tolist() == [0] * len(streams), level
        assert occ_words.shape == (p.shape[0], 512 >> 3 * level)
        assert np.array_equal(u64(occ_words), H.words_of(pools[level])), level
        assert counts.tolist() == pools[level].sum(1).tolist()
        used[level] = pos.tolist()
    assert used[0] == nwords.tolist()
    for g in range(len(streams)):                                # the coarse levels read what the reference reads: a prefix
        sl = slice(g * group, (g + 1) * group)
        for level in (1, 2):
            assert used[level][g] == I.decode_group(p[sl], ref[sl], f1, *streams[g], stop=level)[2] <= used[0][g]
    return states, flat, nwords, dec, rd


@pytest.mark.parametrize("group", [1, 2, 64])
def test_encoder_is_byte_identical_and_decoder_inverts_it_at_every_level(dev, cloud, group):
    p, gt, ref, _, _, f1, streams = cloud
    check_against_reference(dev, p, gt, ref, f1, group, streams[group])


def test_the_full_block_under_the_costliest_table_stays_inside_its_region(dev, cloud):
    """Every symbol of the all-full block is a 1; under f1 = 1 each costs 16 bits, a word for every second symbol, the
    most a table can ask of a block: 37376 symbols, of which the stream takes half in words (the 64 states hold the
    rest).  The sparse blocks beside it run under the same table."""
    p, gt, ref, _, _, _, _ = cloud
    f1 = np.ones(52224, np.int64)
    streams = I.encode(p[2:5], gt[2:5], ref[2:5], f1, 1)
    assert 37376 // 2 - 64 <= streams[1][1].size <= 37376 // 2
    check_against_reference(dev, p[2:5], gt[2:5], ref[2:5], f1, 1, streams)


def test_damaged_streams_end_in_a_status_and_raise(dev, cloud):
    from nvfpcc_amd import lossless_inter_pack as lp, ops
    p, gt, ref, _, _, f1, streams = cloud
    group = 2
    states, flat, nwords, dec, rd = check_against_reference(dev, p, gt, ref, f1, group, streams[group])
    fd = torch.from_numpy(np.asarray(f1, np.int32)).to(dev)
    want = torch.from_numpy(H.words_of(H.maxpool(gt)[0]).view(np.int64)).to(dev)

    def decode(st, words, nw, level=0, r=rd):
        out = ops.occ_inter_decode(dec, r, fd, st, words, nw, group, level)
        torch.cuda.synchronize()
        return out

    def good():
        w, c, s, _ = decode(states, flat, nwords)
        lp.check_status(s.cpu().numpy())
        assert torch.equal(w, want) and c.tolist() == gt.sum(1).tolist()

    coarse = [I.decode_group(p[2 * g:2 * g + 2], ref[2 * g:2 * g + 2], f1, *streams[group][g], stop=1)[2] for g in (0, 1)]
    assert I.decode_group(p[:2], ref[:2], f1, *streams[group][0], stop=2)[2] > 4 and coarse[1] < int(nwords[1]) - 40
    assert int(nwords[2]) > 9
    cut = flat[:flat.numel() - 9].contiguous()                   # truncated: the last group wants words beyond the buffer
    _, _, s, _ = decode(states, cut, nwords)
    assert s[:2].tolist() == [0, 0] and s[2].item() & ops.OCC_RANS_PAST_END
    with pytest.raises(ValueError, match="lossless_lod_pack: the stream of group 2 is damaged.*past the end"):
        lp.check_status(s.cpu().numpy())
    good()
    flipped = flat.clone()                                       # a flipped bit in the level-0 part of group 1
    flipped[int(nwords[0]) + int(nwords[1]) - 40] ^= 0x00010000
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
    # another reference is another model: the stream of the groups it touches is damaged (the digest is what tells)
    other = rd.clone()
    other[4] = 0
    w, _, s, _ = decode(states, flat, nwords, r=other)
    assert s[:2].tolist() == [0, 0] and (s[2].item() != 0 or not torch.equal(w[4], want[4]))
    good()


def test_refusals_of_the_wrappers(dev, cloud):
    from nvfpcc_amd import ops
    p, gt, ref, _, _, f1, _ = cloud
    pd, gd, rd, fd = to_dev(p[:1], gt[:1], ref[:1], f1, dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    with pytest.raises(RuntimeError, match="f1 must be int32 \\[52224\\]"):
        ops.occ_inter_encode(pyr, rd, fd[:35840].contiguous(), 1)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.occ_inter_encode(pyr, rd, torch.cat([fd[:1], fd])[1:], 1)
    with pytest.raises(RuntimeError, match="cnt and occ are int64 \\[52224\\]"):
        ops.occ_inter_hist(pyr, rd, *(torch.zeros(35840, dtype=torch.int64, device=dev) for _ in range(2)))
    for wrong in (torch.cat([rd, rd]), rd[:, :64].contiguous(), rd.int()):
        with pytest.raises(RuntimeError, match="ref_words must be int64 \\[1, 512\\]"):
            ops.occ_inter_hist(pyr, wrong)
        with pytest.raises(RuntimeError, match="ref_words must be int64 \\[1, 512\\]"):
            ops.occ_inter_encode(pyr, wrong, fd, 1)
    states, words = ops.occ_inter_encode(pyr, rd, fd, 1)
    nwords = torch.tensor([words[0].numel()], dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="ref_words must be int64 \\[1, 512\\]"):
        ops.occ_inter_decode(pyr, torch.cat([rd, rd]), fd, states, words[0], nwords, 1)
    with pytest.raises(RuntimeError, match="level must be 0, 1 or 2"):
        ops.occ_inter_decode(pyr, rd, fd, states, words[0], nwords, 1, level=3)


def test_c_entry_points_return_einval_before_any_launch(dev):
    from nvfpcc_amd import ops
    lib = ops.lib()
    t = torch.zeros(64, dtype=torch.int64, device=dev)
    a = t.data_ptr()
    EINVAL = ops._K["NVF_EINVAL"]
    assert lib.nvf_occ_ref_words(a, 1, a, a, 0, a, a, None) == EINVAL
    assert lib.nvf_occ_ref_words(a, -1, a, a, 1, a, a, None) == EINVAL
    assert lib.nvf_occ_ref_words(None, 1, a, a, 1, a, a, None) == EINVAL
    assert lib.nvf_occ_ref_words(a, 1, a, a, 1, None, a, None) == EINVAL
    assert lib.nvf_occ_inter_hist(a, a, a, a, None, a, a, 1, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_hist(a, a, a, a, a, a, a, 0, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_encode(a, a, a, a, a, a, a, a, None, a, a, a, a, a, 1, 1, a, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_encode(a, a, a, a, a, a, a, a, a, a, a, a, a, a + 4, 1, 1, a, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_encode(a, a, a, a, a, a, a, a, a, a, a, a, a, a, 1, 0, a, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_decode(a, a, a, a, a, None, a, a, a, a, a, a, 0, 1, 1, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_decode(a, a, a, a, a, a, a + 8, a, a, a, a, a, 0, 1, 1, a, a, None) == EINVAL
    assert lib.nvf_occ_inter_decode(a, a, a, a, a, a, a, a, a, a, a, a, -1, 1, 1, a, a, None) == EINVAL
    torch.cuda.synchronize()


def test_occupancy_round_trip_through_the_pack(dev):
    """encode_occupancy / decode_occupancy on a real decoder: the device's pack is the reference's on the device's own
    p, decodes at the three levels at other batches, is told from the other packs by its first byte, and a reference
    that differs in one voxel raises on the digest."""
    from nvfpcc_amd import lossless_inter_pack as lp, lossless_nbr_pack as nbr, network
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False).to(dev)
    g = torch.Generator().manual_seed(5)
    lat = torch.round(2.0 * torch.randn(5, 3, 2, 2, 2, generator=g)).to(dev)
    gts = make_blocks(5)[0].reshape(5, -1)
    gt = torch.from_numpy(gts.reshape(5, 1, 32, 32, 32)).float().to(dev)
    ref = I.shifted(gts, 0, 0, 1)
    ref[1] = gts[1].astype(bool)
    rd = torch.from_numpy(H.words_of(ref).view(np.int64)).to(dev)
    pools = H.maxpool(gts)
    with torch.no_grad():
        p = net.reconstruct(lat, 2).reshape(5, -1).cpu().numpy()
    cnt, occ = I.histogram(p, gts, ref)
    packs = {}
    for batch, group in ((1, 2), (7, 64)):
        data, info = lp.encode_occupancy(net, lat, gt, rd, batch=batch, group=group, span_groups=1)
        assert data[0] == 4 and lp.module_of(data) is lp
        side = lp.read(data, 5)
        assert side["group"] == group and side["digest"] == info["digest"] == lp.digest(H.words_of(ref))
        assert len(data) == lp.size(5, group, int(side["nwords"].sum()), info["contexts"], info["slots0"])
        assert info["symbols"] == int(cnt.sum()) and info["contexts"] == int((cnt > 0).sum()) == int(side["used"].sum())
        assert side["f1"].tolist() == I.table(cnt, occ).tolist()
        streams = I.encode(p, gts, ref, side["f1"], group)
        assert np.array_equal(side["states"], np.stack([s for s, _ in streams]))
        assert np.array_equal(side["words"], np.concatenate([w for _, w in streams]))
        packs[group] = data
        for level in (0, 1, 2):
            assert np.array_equal(u64(info["gt_words"][level]), H.words_of(pools[level]))
            words, counts = lp.decode_occupancy(net, lat, data, rd, level=level, batch=8 - batch, span_groups=1)
            assert np.array_equal(u64(words), H.words_of(pools[level])), (batch, level)
            assert counts.tolist() == pools[level].sum(1).tolist()
    with pytest.raises(ValueError, match="version 4, this reader knows 3"):
        nbr.decode_occupancy(net, lat, packs[2], batch=2)
    one = rd.clone()
    one[3, 100] ^= 1 << 9                                        # a reference that differs in one voxel
    n_ref = int(ref.sum()) + (1 if not ref[3, 100 * 64 + 9] else -1)
    with pytest.raises(ValueError, match="the reference is not the one the pack was coded under: its words' digest is %s, "
                       "the pack's %s; the reference sets %d voxels" % (lp.digest(one).hex(), lp.digest(rd).hex(), n_ref)):
        lp.decode_occupancy(net, lat, packs[2], one, batch=2)
    with pytest.raises(ValueError, match=r"reference words are int64 \[5, 512\]"):
        lp.decode_occupancy(net, lat, packs[2], rd[:4], batch=2)
    data = bytearray(packs[2])
    data[-3] ^= 0x10
    with pytest.raises(ValueError, match="lossless_lod_pack: the stream of group 2 is damaged"):
        lp.decode_occupancy(net, lat, bytes(data), rd, batch=2)
    with pytest.raises(ValueError, match="codes 5 blocks"):
        lp.decode_occupancy(net, lat[:4], packs[2], rd[:4].contiguous(), batch=2)
    with pytest.raises(ValueError, match="level 3"):
        lp.decode_occupancy(net, lat, packs[2], rd, level=3)
