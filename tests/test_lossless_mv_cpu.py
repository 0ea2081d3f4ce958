"""Block motion compensation in front of the inter contexts, the host half: the numpy reference (tests/occ_motion_ref.py)
on hand-made blocks, the byte layout of lossless_mv_pack and every malformed case, the command line's flag and its
refusals, and the held-out rates on the trained fixtures under a reference that moves as a whole, block by block and
beyond the search radius.  tests/test_gpu_lossless_mv.py holds the device to this reference byte for byte."""
import functools
import struct

import numpy as np
import pytest

from nvfpcc_amd import lossless_mv_pack as mp
from tests import occ_inter_ref as I
from tests import occ_motion_ref as M
from tests import occ_nbr_ref as N

VOX = 32768
MOVES = [(0, 0, 0), (1, 0, 0), (0, -2, 1), (2, 1, -1), (-1, 2, 1), (0, 0, -2), (1, 2, 1), (-2, -2, 2), (0, 1, 0), (2, 0, 0),
         (-1, -1, -1), (1, -2, 0)]


def vox(v0, v1, v2):
    return (v0 * 32 + v1) * 32 + v2


def test_a_single_point_under_each_sign_of_each_axis():
    """R'(v) = Ref(o + v - d): a reference point q shows at v = q - o + d."""
    o, q = np.asarray([[64, 96, 128]]), np.asarray([[64 + 10, 96 + 11, 128 + 12]])
    assert np.flatnonzero(M.compensated(q, o, [[0, 0, 0]])).tolist() == [vox(10, 11, 12)]
    for axis in range(3):
        for step in (-8, -1, 1, 8):
            d = [0, 0, 0]
            d[axis] = step
            v = [10, 11, 12]
            v[axis] += step
            assert np.flatnonzero(M.compensated(q, o, [d])).tolist() == [vox(*v)], (axis, step)
    assert np.flatnonzero(M.compensated(q, o, [[3, -4, 5]])).tolist() == [vox(13, 7, 17)]
    # a point outside the block comes inside under the right vector, and one inside leaves
    edge = np.asarray([[63, 96, 128], [64, 96, 160]])
    assert not M.compensated(edge, o, [[0, 0, 0]])[0, 1:].any() and not M.compensated(edge, o, [[0, 0, 0]])[0, 0]
    assert np.flatnonzero(M.compensated(edge, o, [[1, 0, 0]])).tolist() == [vox(0, 0, 0)]
    assert np.flatnonzero(M.compensated(edge, o, [[0, 0, -1]])).tolist() == [vox(0, 0, 31)]
    assert not M.compensated(np.asarray([[64, 96, 128 + 25]]), o, [[0, 0, 8]]).any()      # v2 = 33: out of the block


def test_a_window_over_eight_reference_blocks_of_which_some_are_absent():
    rng = np.random.default_rng(4)
    o, d = np.asarray([[64, 64, 64]]), np.asarray([[5, -7, 3]])          # the window starts at (59, 71, 61)
    corners = [(32, 64, 32), (32, 64, 64), (32, 96, 32), (32, 96, 64), (64, 64, 32), (64, 64, 64), (64, 96, 32), (64, 96, 64)]
    present = [c for i, c in enumerate(corners) if i not in (1, 6)]
    pts = np.concatenate([np.asarray(c) + rng.integers(0, 32, (4000, 3)) for c in present])
    got = M.compensated(pts, o, d)[0].reshape(32, 32, 32)
    have = set(map(tuple, pts.tolist()))
    for v in rng.integers(0, 32, (500, 3)).tolist() + [[0, 0, 0], [31, 31, 31], [4, 24, 2], [5, 25, 3]]:
        q = (64 + v[0] - 5, 64 + v[1] + 7, 64 + v[2] - 3)
        assert got[tuple(v)] == (q in have)
    # the two absent reference blocks read 0: (32, 64, 64) and (64, 96, 32)
    assert not got[:5, :25, 3:].any() and not got[5:, 25:, :3].any()
    assert got[:5, :25, :3].any() and got[5:, 25:, 3:].any() and got[5:, :25, 3:].any()


def test_negative_and_too_large_coordinates_read_zero():
    pts = np.asarray([[0, 0, 0], [1, 2, 3], [-1, 0, 0], [0, -3, 0], [(1 << 26) - 1] * 3, [1 << 26, 0, 0]])
    zero = M.compensated(pts, [[0, 0, 0]], [[2, 1, 8]])                  # the window starts at (-2, -1, -8)
    assert np.flatnonzero(zero).tolist() == [vox(2, 1, 8), vox(3, 3, 11)]
    top = (1 << 26) - 32
    assert np.flatnonzero(M.compensated(pts, [[top] * 3], [[0, 0, 0]])).tolist() == [vox(31, 31, 31)]
    assert np.flatnonzero(M.compensated(pts, [[top] * 3], [[-8, -8, -8]])).tolist() == [vox(23, 23, 23)]
    assert not M.compensated(pts, [[top, 0, 0]], [[-8, 0, 0]]).any()    # (2^26, 0, 0) is no point of Ref


def test_search_finds_a_move_and_keeps_the_tie_order():
    rng = np.random.default_rng(9)
    g = rng.random((1, VOX)) < 0.05
    o = np.asarray([[64, 64, 64]])
    pts = M.cloud_of(g, o) + np.asarray([1, -2, 2])
    mv, cost = M.search(g, pts, o, 2)
    assert mv.tolist() == [[-1, 2, -2]]
    lost = int(g.sum()) - int(M.compensated(pts, o, mv)[0].sum())        # what the move pushed out of the window's reach
    assert cost[0, 0] == lost == 0 and cost[0, 1] > 0
    # a pattern of period 2 along axis 1: (0, -1, 0) and (0, 1, 0) cost the same, and so do (0, +-1, +-2 ...); the winner
    # is the shortest vector, and among the shortest the lexicographically smaller
    stripes = np.zeros((32, 32, 32), bool)
    stripes[:, 1::2, :] = True
    ref = np.zeros((36, 36, 36), bool)
    ref[:, 0::2, :] = True                                               # the window, two voxels wider on every side
    pts = np.argwhere(ref) + 62
    c = M.costs(stripes.reshape(-1), M.in_range(pts), o[0], 2)
    vs = M.vectors(2)
    assert c[vs.index((0, -1, 0))] == c[vs.index((0, 1, 0))] == c[vs.index((2, 1, -2))] == 0 and c[vs.index((0, 0, 0))] == VOX
    mv, cost = M.search(stripes.reshape(1, -1), pts, o, 2)
    assert mv.tolist() == [[0, -1, 0]] and cost.tolist() == [[0, VOX]]
    # the zero vector wins every tie it takes part in; an empty window gives 0
    full = np.argwhere(np.ones((36, 36, 36), bool)) + 62
    assert M.search(np.ones((1, VOX), bool), full, o, 2)[0].tolist() == [[0, 0, 0]]
    mv, cost = M.search(g, np.zeros((0, 3), np.int64), o, 2)
    assert mv.tolist() == [[0, 0, 0]] and cost.tolist() == [[int(g.sum())] * 2]


def test_pack_layout_size_and_every_malformed_case():
    mv = np.zeros((11, 3), np.int64)
    mv[1], mv[8], mv[10] = (1, -2, 3), (0, 0, -3), (-3, 0, 0)
    data = mp.write(3, mv)
    assert len(data) == mp.size(11, 3) == 6 + 2 + 9
    assert data[0] == mp.VERSION == 1 and data[1] == 3 and struct.unpack_from("<I", data, 2) == (11,)
    assert data[6:8] == bytes([0b00000010, 0b00000101])
    assert struct.unpack_from("<9b", data, 8) == (1, -2, 3, 0, 0, -3, -3, 0, 0)
    side = mp.read(data, 11)
    assert side["radius"] == 3 and side["n_blocks"] == 11 and np.array_equal(side["mv"], mv) and side["mv"].dtype == np.int32
    assert np.array_equal(mp.read(data)["mv"], mv)
    import torch
    assert mp.write(3, torch.from_numpy(mv).int()) == data
    still = mp.write(8, np.zeros((8, 3), np.int32))
    assert still == bytes([1, 8, 8, 0, 0, 0, 0]) and len(still) == mp.size(8, 0) and not mp.read(still, 8)["mv"].any()
    assert mp.size(12, 11) == 41 and mp.size(1, 0) == 7 and mp.size(9, 9) == 6 + 2 + 27
    far = mp.write(8, [[8, -8, 0]])
    assert mp.read(far)["mv"].tolist() == [[8, -8, 0]]

    def bad(blob, match, **kw):
        with pytest.raises(ValueError, match="lossless_mv_pack: .*" + match):
            mp.read(blob, **kw)
    patch = lambda at, *b: data[:at] + bytes(x & 255 for x in b) + data[at + len(b):]
    bad(b"", "empty")
    bad(patch(0, 2), "version 2, this reader knows 1")
    bad(patch(0, 0), "version 0")
    bad(data[:4], "truncated header")
    bad(patch(1, 0), "radius 0 outside 1..8")
    bad(patch(1, 9), "radius 9 outside 1..8")
    bad(data, "codes 11 blocks, the pack holds 12", n_blocks=12)
    bad(patch(2, 0, 0, 0, 0), "no blocks")
    bad(data[:7], "truncated bitmap")
    bad(data[:-1], "truncated vectors: the bitmap names 3, 2 follow whole")
    bad(data[:8], "truncated vectors: the bitmap names 3, 0 follow whole")
    bad(data + b"\0", "1 trailing bytes")
    bad(patch(7, 0b00001101), "the bitmap sets bit 11, at or above the 11 blocks")
    bad(patch(7, 0b10000101) + b"\1\1\1", "the bitmap sets bit 15")
    bad(patch(11, 0, 0, 0), "block 8 is listed with the vector 0")
    bad(patch(8, 4), r"block 1's vector \(4, -2, 3\) has a component beyond \+-3")
    bad(patch(15, -4),r"block 10's vector \(-3, -4, 0\) has a component beyond \+-3")
    for args, match in (((0, mv), "radius 0 outside"), ((9, mv), "radius 9 outside"), ((2, mv), r"block 1's vector \(1, -2, 3\)"),
                        ((3, mv[:, :2]), r"integers \[N, 3\]"), ((3, mv.astype(np.float32)), r"integers \[N, 3\]"),
                        ((3, mv[:0]), r"integers \[N, 3\], N >= 1")):
        with pytest.raises(ValueError, match=match):
            mp.write(*args)


def test_parser_grows_only_by_the_new_flag_and_the_refusals_need_no_device():
    import NVFPCC
    parse = NVFPCC.build_parser().parse_args
    inter = ["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "inter", "--lossless_ref", "prev.ply"]
    for argv in (["decode", "pack.pk"], ["encode", "x.ply", "--lossless"], ["encode", "x.ply", "--lossless_lod"], inter,
                 ["decode", "pack.pk", "--lossless_lod", "1", "--lossless_ref", "prev.ply"]):
        ns = parse(argv)
        assert not hasattr(ns, "lossless_mv")
        assert vars(parse(argv + ["--lossless_mv", "4"])) == dict(vars(ns), lossless_mv=4)
    with pytest.raises(SystemExit):
        parse(inter + ["--lossless_mv", "far"])
    for r in (1, 2, 8):
        NVFPCC.lossless_ctx_refusals(parse(inter + ["--lossless_mv", str(r)]))
    NVFPCC.lossless_ctx_refusals(parse(inter))
    for argv, match in ((["encode", "x.ply", "--lossless_lod", "--lossless_mv", "2"],
                         "--lossless_mv 2 moves the reference of --lossless_ctx inter"),
                        (["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "nbr", "--lossless_mv", "2"],
                         "--lossless_mv 2 moves the reference of --lossless_ctx inter"),
                        (["encode", "x.ply", "--lossless_mv", "2"], "--lossless_mv 2 moves the reference of --lossless_ctx inter"),
                        (inter[:-2] + ["--lossless_mv", "2"], "name it with --lossless_ref"),
                        (inter + ["--lossless_mv", "0"], "--lossless_mv 0: the search radius is 1..8"),
                        (inter + ["--lossless_mv", "9"], "--lossless_mv 9: the search radius is 1..8"),
                        (inter + ["--lossless_mv", "-1"], "--lossless_mv -1: the search radius is 1..8")):
        with pytest.raises(SystemExit, match=match):
            NVFPCC.lossless_ctx_refusals(parse(argv))
        with pytest.raises(SystemExit, match=match):
            NVFPCC.encode(parse(argv))                                 # before the device, the data or the weights are touched
    with pytest.raises(SystemExit, match="--lossless_mv 2 is the search radius of encode"):
        NVFPCC.decode(parse(["decode", "no_such.pk", "--lossless_lod", "0", "--lossless_ref", "prev.ply", "--lossless_mv", "2"]))


def fixture_origins():
    from nvfpcc_amd.synth import make_origins
    return make_origins(12).astype(np.int64) + 64


def moved_blocks(gt, origins):
    """The reference of the per-block case: block b's points + MOVES[b], blocks running into one another."""
    return np.concatenate([M.cloud_of(gt[b:b + 1], origins[b:b + 1]) + np.asarray(MOVES[b]) for b in range(12)])


@functools.lru_cache(maxsize=None)
def trained(golden_dir, tag):
    """The fixture's field and cloud, and the neighbour contexts' held-out bits: once for every case of the tag."""
    from tests.test_lossless_lod_cpu import _trained
    p, gt = _trained(golden_dir, tag)
    return p, gt, N.held_out_bits(N.group_sections, N.CONTEXTS, p, gt)


@pytest.mark.parametrize("tag", ["S", "W"])
def test_rates_on_the_trained_fixtures_under_moving_references(golden_dir, tag):
    """Held out as I.held_out_bits, origins make_origins(12) + 64, search radius 2.  The whole cloud moved by (1, 2, 1):
    the search finds (-1, -2, -1) everywhere, the compensated words ARE the frame and the rate is the static one (x 0.263
    on S, x 0.254 on W; uncompensated x 1.029 and 1.041).  Block b moved by MOVES[b]: the search finds -MOVES[b], 409
    voxels differ, and bits + 8 x the 41-byte mv pack stay within 0.35 of the neighbour contexts' bits, the bound the
    static case is held to (measured 0.277 with the pack, 0.267 / 0.258 without; uncompensated 1.068 / 1.061, above 1).
    Moved by (3, 0, 0), beyond the radius: printed, nothing asserted (measured x 0.979 / 0.992)."""
    p, gt, held_nbr = trained(golden_dir, tag)
    origins = fixture_origins()
    n_points = int(gt.sum())
    cloud = M.cloud_of(gt, origins)
    assert n_points == len(cloud) == 11685
    say = lambda name, bits: print(f"{tag} {name}: {bits / n_points:.4f} bpp (x {bits / held_nbr:.3f} of nbr's {held_nbr / n_points:.4f})")

    ref = cloud + np.asarray([1, 2, 1])                                 # the global move
    mv, cost = M.search(gt, ref, origins, 2)
    assert np.array_equal(mv, np.tile([-1, -2, -1], (12, 1))) and not cost[:, 0].any() and cost[:, 1].all()
    comp = M.compensated(ref, origins, mv)
    assert np.array_equal(comp, gt)
    held = I.held_out_bits(p, gt, comp)
    assert held == I.held_out_bits(p, gt, gt)
    say("moved by (1, 2, 1), compensated", held)
    say("moved by (1, 2, 1), plain", I.held_out_bits(p, gt, I.reference_words(ref, origins)[0]))
    assert held <= 0.35 * held_nbr

    ref = moved_blocks(gt, origins)                                     # every block its own move
    mv, cost = M.search(gt, ref, origins, 2)
    assert np.array_equal(mv, -np.asarray(MOVES))
    comp = M.compensated(ref, origins, mv)
    pack = mp.write(2, mv)
    assert len(pack) == mp.size(12, 11) == 41 and np.array_equal(mp.read(pack, 12)["mv"], mv)
    assert int((comp != gt).sum()) == int(cost[:, 0].sum()) == 409
    held = I.held_out_bits(p, gt, comp)
    plain = I.held_out_bits(p, gt, I.reference_words(ref, origins)[0])
    say("moved block by block, compensated", held)
    say("moved block by block, compensated, with the 41-byte mv pack", held + 8 * len(pack))
    say("moved block by block, plain", plain)
    assert held + 8 * len(pack) <= 0.35 * held_nbr
    assert plain > 1.0 * held_nbr

    ref = cloud + np.asarray([3, 0, 0])                                 # beyond the radius: no operating point
    mv, cost = M.search(gt, ref, origins, 2)
    say("moved by (3, 0, 0), radius 2, compensated", I.held_out_bits(p, gt, M.compensated(ref, origins, mv)))
    say("moved by (3, 0, 0), radius 2, plain", I.held_out_bits(p, gt, I.reference_words(ref, origins)[0]))
    print(f"{tag} vectors found: {mv.tolist()}")
