"""Block motion compensation on the device (csrc/occ_motion.hip through nvfpcc_amd.ops and lossless_mv_pack) against the
numpy reference (tests/occ_motion_ref.py), byte for byte: the compensated words under vectors at 0, +-1 and +-8 on every
axis with reference blocks present and absent on every side, at origin 0 and at the top of the 2^26 range, the guard rows
around a block whose vector is out of range, the exhaustive search at radius 1, 2 and 8 with its tie order, and the
version-4 pack of the trained fixtures coded under the words the device fetched."""
import itertools

import numpy as np
import pytest
import torch

from tests import occ_hier_ref as H
from tests import occ_inter_ref as I
from tests import occ_motion_ref as M
from tests.test_lossless_mv_cpu import MOVES, fixture_origins, moved_blocks, trained

pytestmark = pytest.mark.gpu
VOX = 32768
TOP = (1 << 26) - 32
GUARD = 0x5555555555555555


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).astype(np.int32).reshape(-1, 3)).to(dev)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def words(occupancy):
    return H.words_of(np.asarray(occupancy).reshape(-1, VOX))


def own(points, dev):
    from nvfpcc_amd import ops
    return ops.occ_ref_blocks(i32(points, dev))


ORIGINS = np.asarray([[0, 0, 0], [TOP, TOP, TOP], [64, 96, 128], [64, 96, 160]])


@pytest.fixture(scope="module")
def scene():
    """A reference around the four origins: of the 27 blocks around each, about two thirds are present, so that every
    origin has present and absent reference blocks on every side; points outside [0, 2^26) among them."""
    rng = np.random.default_rng(31)
    pts = []
    for o in ORIGINS:
        for step in itertools.product((-32, 0, 32), repeat=3):
            if rng.random() < 0.67:
                pts.append(o + np.asarray(step) + rng.integers(0, 32, (400, 3)))
    pts.append(np.asarray([[-1, 0, 0], [0, -1, 5], [1 << 26, 3, 3], [TOP, 1 << 26, TOP], [(1 << 31) - 1, 0, 0], [-(1 << 31), 5, 5]]))
    pts = np.concatenate(pts)
    return pts[rng.permutation(len(pts))]


VECTORS = [(0, 0, 0)] + [tuple(s if a == axis else 0 for a in range(3)) for axis in range(3) for s in (-8, -1, 1, 8)] + \
    [(8, -8, 8), (-8, -8, -8), (3, -5, 7), (-1, 8, -7)]


def test_the_scene_covers_what_it_is_built_for(scene):
    have = set(map(tuple, (M.in_range(scene) & ~31).tolist()))
    for o in ORIGINS[2:]:
        around = [tuple((o + np.asarray(s)).tolist()) in have for s in itertools.product((-32, 0, 32), repeat=3)]
        assert 8 < sum(around) < 27
    assert (scene < 0).any() and (scene >= 1 << 26).any() and len(VECTORS) == 17


def test_reference_blocks_are_the_distinct_blocks_sorted_with_their_words(dev, scene):
    from nvfpcc_amd import lossless_mv_pack as mp
    ref_own, ref_keys = own(scene, dev)
    inside = M.in_range(scene)
    blocks = np.unique(inside & ~31, axis=0)
    keys = ((blocks[:, 0] >> 5) << 42) | ((blocks[:, 1] >> 5) << 21) | (blocks[:, 2] >> 5)
    order = np.argsort(keys)
    assert ref_keys.tolist() == keys[order].tolist() and ref_own.shape == (len(blocks), 512) and ref_own.dtype == torch.int64
    assert np.array_equal(u64(ref_own), words(I.reference_words(inside, blocks[order])[0]))
    again = mp.reference_blocks(scene, dev)
    assert torch.equal(again[0], ref_own) and torch.equal(again[1], ref_keys)
    none = own(np.zeros((0, 3), np.int64), dev)
    assert none[0].shape == (0, 512) and none[1].shape == (0,)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_words_equal_the_numpy_words_bit_for_bit(dev, scene, n):
    from nvfpcc_amd import ops
    ref_own, ref_keys = own(scene, dev)
    origins = ORIGINS[4 - n:] if n < 3 else ORIGINS[:n]
    for k, d in enumerate(VECTORS):
        mv = np.asarray([VECTORS[(k + 5 * b) % len(VECTORS)] for b in range(n)]) if n == 4 else np.tile(d, (n, 1))
        got, status = ops.occ_mv_words(ref_own, ref_keys, i32(origins, dev), i32(mv, dev))
        assert got.shape == (n, 512) and got.dtype == torch.int64 and status.tolist() == [0]
        want = M.compensated(scene, origins, mv)
        assert want.any(1).all()
        assert np.array_equal(u64(got), words(want)), (n, d)


def test_origins_of_any_content_stay_inside_the_arrays(dev, scene):
    """Unaligned, negative and extreme origins: the words are still Ref(o + v - d), zero wherever no point can be."""
    from nvfpcc_amd import ops
    ref_own, ref_keys = own(scene, dev)
    origins = np.asarray([[69, 90, 131], [-5, -31, 3], [(1 << 31) - 1, -(1 << 31), 0], [TOP - 3, TOP + 1, TOP - 30],
                          [-(1 << 31), 0, 0], [TOP + 27, TOP + 1, TOP + 31]])
    mv = np.asarray([[2, -3, 8], [-8, -8, 1], [-8, 8, 0], [8, 0, -8], [8, 8, 8], [-8, 8, 8]])
    got, status = ops.occ_mv_words(ref_own, ref_keys, i32(origins, dev), i32(mv, dev))
    want = M.compensated(scene, origins, mv)
    assert want[[0, 1, 3]].any(1).all() and not want[[2, 4]].any()
    assert np.array_equal(u64(got), words(want)) and status.tolist() == [0]


def test_no_reference_gives_zero_words_and_zero_vectors(dev):
    from nvfpcc_amd import lossless_mv_pack as mp, ops
    ref_own, ref_keys = own(np.zeros((0, 3), np.int64), dev)
    got, status = ops.occ_mv_words(ref_own, ref_keys, i32(ORIGINS, dev), i32(np.tile([1, -8, 3], (4, 1)), dev), guard=1)
    assert not got[1:5].any() and status.tolist() == [0] and bool((got[0] == GUARD).all()) and bool((got[5] == GUARD).all())
    gt = np.random.default_rng(1).random((4, VOX)) < 0.01
    gw = torch.from_numpy(words(gt).view(np.int64)).to(dev)
    mv, cost = ops.occ_mv_search(gw, ref_own, ref_keys, i32(ORIGINS, dev), 3)
    assert not mv.any() and cost.tolist() == [[int(g.sum())] * 2 for g in gt]
    only_outside = np.asarray([[-1, -1, -1], [1 << 26, 0, 0]])
    assert not mp.compensated_words(only_outside, ORIGINS, np.zeros((4, 3), np.int64), dev).any()


def test_a_vector_out_of_range_zeroes_its_block_and_nothing_else(dev, scene):
    from nvfpcc_amd import lossless_mv_pack as mp, ops
    ref_own, ref_keys = own(scene, dev)
    origins = ORIGINS[1:]
    for wrong in ((0, 9, 0), (-9, 0, 0), (0, 0, (1 << 31) - 1), (-(1 << 31), 8, 8)):
        mv = np.asarray([(8, -8, 1), wrong, (-1, 0, 8)])
        mvd = i32(np.zeros((3, 3)), dev)
        mvd.copy_(torch.tensor(mv.tolist(), dtype=torch.int32))     # straight into the device tensor
        buf, status = ops.occ_mv_words(ref_own, ref_keys, i32(origins, dev), mvd, guard=2)
        assert buf.shape == (7, 512) and status.tolist() == [1]
        assert bool((buf[:2] == GUARD).all()) and bool((buf[5:] == GUARD).all())
        want = M.compensated(scene, origins[[0, 2]], mv[[0, 2]])
        assert np.array_equal(u64(buf[[2, 4]]), words(want)) and not buf[3].any()
    every = i32(np.tile([9, 9, 9], (3, 1)), dev)
    buf, status = ops.occ_mv_words(ref_own, ref_keys, i32(origins, dev), every, guard=1)
    assert status.tolist() == [3] and not buf[1:4].any() and bool((buf[0] == GUARD).all()) and bool((buf[4] == GUARD).all())
    with pytest.raises(ValueError, match=r"lossless_mv_pack: 1 vectors have a component beyond \+-8"):
        mp.compensated_words(scene, origins, [[0, 0, 0], [0, 0, 9], [0, 0, 0]], dev)


def test_zero_vectors_give_occ_ref_words_when_the_reference_lies_under_the_blocks(dev):
    from nvfpcc_amd import lossless_mv_pack as mp, ops
    rng = np.random.default_rng(8)
    origins = np.asarray([[4064, 4064, 4064], [0, 0, 0], [32, 4064, 0], [2048, 96, 4032], [0, 0, 32], [64, 0, 0]])   # unsorted
    points = origins[rng.integers(0, 6, 6000)] + rng.integers(0, 32, (6000, 3))
    want, dropped = ops.occ_ref_words(i32(points, dev), i32(origins, dev))
    assert dropped.tolist() == [0]
    got, status = ops.occ_mv_words(*own(points, dev), i32(origins, dev), i32(np.zeros((6, 3)), dev))
    assert torch.equal(got, want) and status.tolist() == [0]
    assert torch.equal(mp.compensated_words(points, origins, np.zeros((6, 3), np.int64), dev), want)


@pytest.fixture(scope="module")
def moving():
    """Three sparse blocks (two adjacent) and a reference in which each has moved by a vector of its own, with voxels
    lost and voxels added, so that no vector costs 0."""
    rng = np.random.default_rng(17)
    origins = ORIGINS[[0, 2, 3]]
    gt = rng.random((3, VOX)) < 0.03
    moves = np.asarray([(1, 0, -1), (-8, 7, 8), (0, -1, 0)])
    keep = [rng.random(int(g.sum())) < 0.9 for g in gt]
    pts = [M.cloud_of(gt[b:b + 1], origins[b:b + 1])[keep[b]] + moves[b] for b in range(3)]
    pts.append(origins[rng.integers(0, 3, 300)] + rng.integers(-8, 40, (300, 3)))
    return gt, origins, np.concatenate(pts), moves


@pytest.mark.parametrize("radius", [1, 2, 8])
def test_search_equals_the_numpy_search(dev, moving, radius):
    from nvfpcc_amd import lossless_mv_pack as mp, ops
    gt, origins, pts, moves = moving
    sl = slice(1, 3) if radius == 8 else slice(0, 3)                # radius 8 on two blocks only
    want_mv, want_cost = M.search(gt[sl], pts, origins[sl], radius)
    if radius == 8:
        assert want_mv.tolist() == (-moves[sl]).tolist()
    assert want_cost[:, 0].all() and (want_cost[:, 0] < want_cost[:, 1]).any()
    gw = torch.from_numpy(words(gt[sl]).view(np.int64)).to(dev)
    ref_own, ref_keys = own(pts, dev)
    mv, cost = ops.occ_mv_search(gw, ref_own, ref_keys, i32(origins[sl], dev), radius)
    assert mv.dtype == torch.int32 and mv.tolist() == want_mv.tolist() and cost.tolist() == want_cost.tolist()
    mv2, cost2 = mp.search(gw, pts, origins[sl], radius)
    assert torch.equal(mv2, mv) and torch.equal(cost2, cost)         # two calls, the same bits
    one = ops.occ_mv_search(gw[:1].contiguous(), ref_own, ref_keys, i32(origins[sl][:1], dev), radius)
    assert one[0].tolist() == want_mv[:1].tolist() and one[1].tolist() == want_cost[:1].tolist()


def test_search_tie_order_and_an_empty_window(dev):
    from nvfpcc_amd import ops
    o = np.asarray([[64, 64, 64], [4096, 0, 0], [128, 64, 64]])
    stripes = np.zeros((32, 32, 32), bool)
    stripes[:, 1::2, :] = True                                       # period 2 along axis 1: (0, -1, 0) and (0, 1, 0) tie at 0
    ref = np.zeros((48, 48, 48), bool)
    ref[:, 0::2, :] = True
    pts = np.concatenate([np.argwhere(ref) + 56, np.argwhere(np.ones((48, 48, 48), bool)) + np.asarray([120, 56, 56])])
    gt = np.stack([stripes.reshape(-1), stripes.reshape(-1), np.ones(VOX, bool)])
    gw = torch.from_numpy(words(gt).view(np.int64)).to(dev)
    ref_own, ref_keys = own(pts, dev)
    for radius in (1, 2, 8):
        want_mv, want_cost = M.search(gt, pts, o, radius) if radius < 8 else (None, None)
        mv, cost = ops.occ_mv_search(gw, ref_own, ref_keys, i32(o, dev), radius)
        # the shortest of the equal vectors, the lexicographically smaller of those; 0 for the empty window and for the
        # full block in a full window, where every vector ties
        assert mv.tolist() == [[0, -1, 0], [0, 0, 0], [0, 0, 0]]
        assert cost.tolist() == [[0, VOX], [VOX // 2, VOX // 2], [0, 0]]
        if want_mv is not None:
            assert mv.tolist() == want_mv.tolist() and cost.tolist() == want_cost.tolist()


@pytest.mark.parametrize("tag", ["S", "W"])
def test_fixtures_moved_block_by_block_vectors_costs_and_the_whole_pack(dev, golden_dir, tag):
    """The per-block case of tests/test_lossless_mv_cpu.py on the device: the vectors are -MOVES[b], both costs and the
    compensated words are the numpy reference's, and the version-4 pack coded under the device's words is
    tests/occ_inter_ref.py's under the reference's words, byte for byte."""
    from nvfpcc_amd import lossless_inter_pack as lp, lossless_mv_pack as mp, ops
    p, gt, _ = trained(golden_dir, tag)
    origins = fixture_origins()
    ref = moved_blocks(gt, origins)
    want_mv, want_cost = M.search(gt, ref, origins, 2)
    comp = M.compensated(ref, origins, want_mv)
    shape = (12, 1, 32, 32, 32)
    pd, gd = torch.from_numpy(p).reshape(shape).to(dev), torch.from_numpy(gt.astype(np.float32)).reshape(shape).to(dev)
    pyr = ops.occ_hier_pyramid(pd, gd)
    assert np.array_equal(u64(pyr["gt_words"][0]), words(gt))
    rb = mp.reference_blocks(ref, dev)
    mv, cost = mp.search(pyr["gt_words"][0], rb, origins, 2)
    assert mv.tolist() == want_mv.tolist() == (-np.asarray(MOVES)).tolist() and cost.tolist() == want_cost.tolist()
    assert int(cost[:, 0].sum()) == 409
    rd = mp.compensated_words(rb, origins, mv)
    assert np.array_equal(u64(rd), words(comp))
    assert mp.write(2, mv) == mp.write(2, want_mv) and len(mp.write(2, mv)) == 41
    # the pack: the device's table and stream under its own R' against the numpy coder under the reference's R'
    cnt, occ = (t.cpu().numpy().view(np.uint64) for t in ops.occ_inter_hist(pyr, rd))
    f1, used = lp.table_from_counts(cnt, occ)
    states, stream = ops.occ_inter_encode(pyr, rd, torch.from_numpy(f1.astype(np.int32)).to(dev), 12)
    data = lp.write(12, 12, lp.digest(rd), f1, used, states.cpu().numpy(), [w.cpu().numpy().view(np.uint32) for w in stream])
    want_cnt, want_occ = I.histogram(p, gt, comp)
    want_f1 = I.table(want_cnt, want_occ)
    (s, w), = I.encode(p, gt, comp, want_f1, 12)
    assert data == lp.write(12, 12, lp.digest(words(comp)), want_f1, want_cnt > 0, s[None], [w])
    assert lp.read(data, 12)["digest"] == lp.digest(words(comp)) != lp.digest(words(I.reference_words(ref, origins)[0]))


def test_refusals_of_the_wrappers_and_einval_of_the_entry_points(dev, scene):
    from nvfpcc_amd import ops
    ref_own, ref_keys = own(scene, dev)
    org, mv = i32(ORIGINS, dev), i32(np.zeros((4, 3)), dev)
    gw = torch.zeros((4, 512), dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="origins must be int32"):
        ops.occ_mv_words(ref_own, ref_keys, org.long(), mv)
    with pytest.raises(RuntimeError, match="origins must be int32"):
        ops.occ_mv_words(ref_own, ref_keys, org[:0], mv[:0])
    with pytest.raises(RuntimeError, match=r"mv must be int32 \[4, 3\]"):
        ops.occ_mv_words(ref_own, ref_keys, org, mv[:3])
    with pytest.raises(RuntimeError, match=r"ref_own int64 \[Nref, 512\]"):
        ops.occ_mv_words(ref_own[:-1], ref_keys, org, mv)
    with pytest.raises(RuntimeError, match="distinct and sorted ascending"):
        ops.occ_mv_words(ref_own, ref_keys.flip(0).contiguous(), org, mv)
    with pytest.raises(RuntimeError, match=r"gt_words0 must be int64 \[4, 512\]"):
        ops.occ_mv_search(gw[:3], ref_own, ref_keys, org, 2)
    for radius in (0, 9, -1):
        with pytest.raises(RuntimeError, match="radius %d outside 1..8" % radius):
            ops.occ_mv_search(gw, ref_own, ref_keys, org, radius)
    with pytest.raises(RuntimeError, match="points must be int32"):
        ops.occ_ref_blocks(i32(scene, dev).long())
    lib = ops.lib()
    EINVAL = ops._K["NVF_EINVAL"]
    a = torch.zeros(4096, dtype=torch.int64, device=dev).data_ptr()
    big = ops.OCC_HIER_MAX_BATCH + 1
    for args in ((None, a, 1, a, a, 1, a, a), (a, None, 1, a, a, 1, a, a), (a, a, 1, None, a, 1, a, a), (a, a, 1, a, None, 1, a, a),
                 (a, a, 1, a, a, 1, None, a), (a, a, 1, a, a, 1, a, None), (a, a, 1, a, a, 0, a, a), (a, a, 1, a, a, -1, a, a),
                 (a, a, 1, a, a, big, a, a), (a, a, -1, a, a, 1, a, a)):
        assert lib.nvf_occ_mv_words(*args, None) == EINVAL, args
    for args in ((None, a, a, 1, a, 1, 2, a, a), (a, None, a, 1, a, 1, 2, a, a), (a, a, None, 1, a, 1, 2, a, a),
                 (a, a, a, 1, None, 1, 2, a, a), (a, a, a, 1, a, 1, 2, None, a), (a, a, a, 1, a, 1, 2, a, None),
                 (a, a, a, 1, a, 0, 2, a, a), (a, a, a, 1, a, big, 2, a, a), (a, a, a, -1, a, 1, 2, a, a),
                 (a, a, a, 1, a, 1, 0, a, a), (a, a, a, 1, a, 1, 9, a, a), (a, a, a, 1, a, 1, -3, a, a)):
        assert lib.nvf_occ_mv_search(*args, None) == EINVAL, args
    torch.cuda.synchronize()
