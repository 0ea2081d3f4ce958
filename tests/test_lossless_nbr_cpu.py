"""Scalable lossless geometry under the neighbour contexts, the host half: the numpy reference (tests/occ_nbr_ref.py)
round-trips, stops exactly at the coarse levels on a strict prefix, shares its first two sections with the field
contexts' coder, computes the neighbour class as defined, beats the field contexts held out on the trained fixtures and
stays inside the code-length bound; the byte layout of lossless_nbr_pack, the dispatcher on byte 0, the command line's
flag.  tests/test_gpu_lossless_nbr.py holds the device to this reference byte for byte."""
import math
import struct

import numpy as np
import pytest

from nvfpcc_amd import lossless_lod_pack as llp
from nvfpcc_amd import lossless_nbr_pack as lp
from tests import occ_hier_ref as H
from tests import occ_nbr_ref as N
from tests import occ_rans_ref as R
from tests.test_lossless_cpu import cases
from tests.test_lossless_lod_cpu import _trained

VOX = 32768


def vox(z, y, x):
    return (z * 32 + y) * 32 + x


def cell1(z, y, x):
    return (z * 16 + y) * 16 + x


def test_neighbour_class_on_a_hand_made_block():
    full, empty = np.ones((1, 4096), bool), np.zeros((1, 4096), bool)
    n = lambda v, occ1, blk=0: int(N.neighbour_class(np.asarray([blk]), np.asarray([v]), occ1)[0])
    assert n(vox(0, 0, 0), full) == 0                              # a corner voxel: every neighbour is outside the block
    assert n(vox(31, 31, 31), full) == 0
    assert n(vox(3, 3, 3), full) == n(vox(2, 2, 2), full) == 31    # parent (1, 1, 1), towards +1 and towards -1
    assert n(vox(3, 3, 3), empty) == 0
    only = lambda *cells: np.isin(np.arange(4096), [cell1(*c) for c in cells])[None]
    # v = (3, 3, 3): P = (1, 1, 1), s = (+1, +1, +1)
    assert n(vox(3, 3, 3), only((2, 1, 1))) == n(vox(3, 3, 3), only((1, 2, 1))) == n(vox(3, 3, 3), only((1, 1, 2))) == 8
    assert n(vox(3, 3, 3), only((2, 2, 1))) == n(vox(3, 3, 3), only((2, 1, 2))) == n(vox(3, 3, 3), only((1, 2, 2))) == 2
    assert n(vox(3, 3, 3), only((2, 2, 2))) == 1
    assert n(vox(3, 3, 3), only((2, 1, 1), (1, 2, 1), (1, 2, 2))) == (2 * 4 + 1) * 2
    # the parent itself and the cells on the other side do not count
    assert n(vox(3, 3, 3), only((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0))) == 0
    # v = (2, 3, 2): P = (1, 1, 1), s = (-1, +1, -1)
    assert n(vox(2, 3, 2), only((0, 1, 1))) == 8 and n(vox(2, 3, 2), only((0, 2, 1))) == 2
    assert n(vox(2, 3, 2), only((0, 2, 0))) == 1 and n(vox(2, 3, 2), only((2, 1, 1), (1, 0, 1), (1, 1, 2))) == 0
    # a face of the block: the neighbours along x are outside, the others count
    assert n(vox(3, 3, 31), full) == (2 * 4 + 1) * 2 and n(vox(3, 31, 31), full) == (1 * 4 + 0) * 2
    # blocks do not see each other: the last voxel of an empty block next to a full one, and the first of the full one
    two = np.concatenate([empty, full])
    assert n(vox(31, 31, 31), two, 0) == 0 and n(vox(0, 0, 0), two, 1) == 0 and n(vox(1, 1, 1), two, 1) == 31
    assert n(vox(1, 1, 1), two[::-1], 1) == 0


def test_contexts_of_the_three_sections():
    _, p, gt = next(cases())
    sections = N.group_sections(p[:3], gt[:3])
    old = H.group_sections(p[:3], gt[:3])
    assert [s[0] for s in sections] == [2, 1, 0]
    for new, was in zip(sections[:2], old[:2]):                    # sections 2 and 1: the field contexts' own
        assert all(np.array_equal(a, b) for a, b in zip(new[1:], was[1:]))
    blk, cell, ctx = sections[2][1:4]
    assert np.array_equal(blk, old[2][1]) and np.array_equal(cell, old[2][2])
    assert ctx.min() >= 3072 and ctx.max() < N.CONTEXTS == 35840 == lp.CONTEXTS
    assert np.array_equal((ctx - 3072) % 1024, old[2][3])
    assert np.array_equal((ctx - 3072) // 1024, N.neighbour_class(blk, cell, H.maxpool(gt[:3])[1]))
    assert len(np.unique((ctx - 3072) // 1024)) > 8


@pytest.mark.parametrize("group", [1, 2, 64])
def test_reference_round_trips_and_stops_at_every_level(group):
    for name, p, gt in cases():
        cnt, occ = N.histogram(p, gt)
        assert int(cnt.sum()) == N.symbols_coded(p, gt) and np.all(occ <= cnt) and not cnt[:1024].any()
        hc, ho = H.histogram(p, gt)
        assert np.array_equal(cnt[1024:3072], hc[1024:]) and np.array_equal(occ[1024:3072], ho[1024:])
        assert np.array_equal(cnt[3072:].reshape(32, 1024).sum(0), hc[:1024])
        f1 = N.table(cnt, occ)
        streams = N.encode(p, gt, f1, group)
        assert len(streams) == -(-p.shape[0] // group)
        pools = H.maxpool(gt)
        for g, (states, words) in enumerate(streams):
            sl = slice(g * group, (g + 1) * group)
            assert states.min() >= 1 << 31 and states.max() < 1 << 63
            assert words.size <= p[sl].shape[0] * N.BLOCK_WORDS
            occ0, final, used = N.decode_group(p[sl], f1, states, words)
            assert np.array_equal(occ0, pools[0][sl]), (name, g)
            assert np.all(final == np.uint64(1 << 31)) and used == words.size, (name, g)
            for stop in (2, 1):
                got, x_l, used_l = N.decode_group(p[sl], f1, states, words, stop=stop)
                assert np.array_equal(got, pools[stop][sl]), (name, g, stop)
                mixed = any(0 < int(b.sum()) < VOX for b in gt[sl])     # as tests/test_lossless_lod_cpu.py
                assert (used_l < words.size if mixed else used_l <= words.size), (name, g, stop)
                again, _, k = N.decode_group(p[sl], f1, states, words[:used_l], stop=stop)
                assert k == used_l and np.array_equal(again, got)
                # the first two sections are the field coder's, given the same table entries: word for word
                was, x_h, used_h = H.decode_group(p[sl], f1[:3072], states, words, stop=stop)
                assert used_h == used_l and np.array_equal(was, got) and np.array_equal(x_h, x_l)


@pytest.mark.parametrize("tag", ["S", "W"])
def test_rate_and_code_length_bound_on_the_trained_fixtures(golden_dir, tag):
    """Held out (a table from the even blocks codes the odd ones and back) the neighbour contexts spend at most 0.95 of
    the field contexts' bits: measured 2.6665 / 3.0900 = 0.863 on S and 2.3372 / 2.5706 = 0.909 on W.  In sample, on 12
    blocks and 11685 points (printed, no assertion on the bytes: the larger table may outweigh the gain on so few):
    S 3.0256 -> 2.5289 ideal bpp, W 2.4980 -> 2.1681.  Stream bits <= ideal + 4096 per group + log2(1 + 2^-15) per coded
    symbol, as for the field contexts."""
    p, gt = _trained(golden_dir, tag)
    n_points = int(gt.sum())
    assert n_points == 11685
    held_old = N.held_out_bits(H.group_sections, H.CONTEXTS, p, gt)
    held_new = N.held_out_bits(N.group_sections, N.CONTEXTS, p, gt)
    print(f"{tag}: held out {held_old / n_points:.4f} -> {held_new / n_points:.4f} bpp (x {held_new / held_old:.3f})")
    hc, ho = H.histogram(p, gt)
    hf = H.table(hc, ho)
    ideal_old = H.ideal_bits(hf[hc > 0], hc[hc > 0], ho[hc > 0])
    cnt, occ = N.histogram(p, gt)
    f1 = N.table(cnt, occ)
    live = cnt > 0
    ideal = N.ideal_bits(f1[live], cnt[live], occ[live])
    symbols = int(cnt.sum())
    assert symbols == int(hc.sum()) == 51072
    slots0 = int(live[3072:].reshape(32, 1024).any(0).sum())
    states, words = N.encode(p, gt, f1, 12)[0]
    data = lp.write(12, 12, f1, live, states[None], [words])
    h_states, h_words = H.encode(p, gt, hf, 12)[0]
    was = llp.write(12, 12, hf, hc > 0, h_states[None], [h_words])
    print(f"{tag}: in sample {ideal_old / n_points:.4f} -> {ideal / n_points:.4f} ideal bpp, contexts {int((hc > 0).sum())} "
          f"-> {int(live.sum())}, pack {len(was)} -> {len(data)} bytes with the table, {8 * len(was) / n_points:.4f} -> "
          f"{8 * len(data) / n_points:.4f} bpp")
    assert held_new <= 0.95 * held_old
    assert len(data) == lp.size(12, 12, words.size, int(live.sum()), slots0) == \
        9 + 384 + 4 * slots0 + 2 * int(live.sum()) + 516 + 4 * words.size
    side = lp.read(data, 12)
    assert np.array_equal(side["f1"], f1) and np.array_equal(side["used"], live)
    assert np.array_equal(side["states"], states[None]) and np.array_equal(side["words"], words)
    for group in (1, 4, 12):
        streams = N.encode(p, gt, f1, group)
        bits = sum(64 * 64 + 32 * w.size for _, w in streams)
        bound = ideal + 4096 * len(streams) + symbols * math.log2(1 + 2.0 ** -15)
        print(f"  group {group}: {bits} bits, bound {bound:.1f}, {bits / n_points:.4f} bpp")
        assert bits <= bound
        for g, (s, w) in enumerate(streams):
            sl = slice(g * group, (g + 1) * group)
            occ0, final, used = N.decode_group(p[sl], f1, s, w)
            assert np.array_equal(occ0, gt[sl]) and np.all(final == np.uint64(1 << 31)) and used == w.size


def test_table_rule_is_v1s_over_the_coded_symbols():
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 1 << 40, lp.CONTEXTS)
    occ = (cnt * rng.random(lp.CONTEXTS)).astype(np.int64)
    cnt[:4], occ[:4] = [0, 5, 5, 1 << 40], [0, 0, 5, 1]
    f1, used = lp.table_from_counts(cnt, occ)
    assert np.array_equal(f1, R.table(cnt, occ)) and f1[:4].tolist() == [32768, 1, 65535, 1]
    assert used[:4].tolist() == [False, True, True, True] and np.array_equal(used, cnt > 0)
    for c, o in (([1] * 3072, [1] * 3072), ([1] * lp.CONTEXTS, [2] * lp.CONTEXTS), ([0] * lp.CONTEXTS, [0] * 9 + [1] * (lp.CONTEXTS - 9))):
        with pytest.raises(ValueError, match="35840 pairs with 0 <= occupied <= symbols"):
            lp.table_from_counts(c, o)


def small_pack():
    rng = np.random.default_rng(1)
    used = rng.random(lp.CONTEXTS) < 0.01
    used[:1024] = False
    used[[1024, 3071, 3072, 3072 + 31 * 1024 + 1023]] = True      # slots 0 (n = 0) and 1023 (n = 31) among them
    used[3072 + 5::1024] = False
    used[[3072 + 5 + 3 * 1024, 3072 + 5 + 17 * 1024]] = True      # slot 5: n = 3 and 17
    f1 = np.where(used, rng.integers(1, 65536, lp.CONTEXTS), 32768)
    states = rng.integers(1 << 31, 1 << 62, (3, 64)).astype(np.uint64)
    words = [rng.integers(0, 1 << 32, n).astype(np.uint32) for n in (5, 0, 17)]
    return f1, used, states, words, lp.write(2, 5, f1, used, states, words)


def test_pack_layout_and_every_malformed_case():
    f1, used, states, words, data = small_pack()
    k = int(used.sum())
    by_n = used[3072:].reshape(32, 1024)
    slots0 = np.flatnonzero(by_n.any(0))
    m = slots0.size
    assert len(data) == lp.size(5, 2, 22, k, m) == 9 + 384 + 4 * m + 2 * k + 3 * 4 + 3 * 512 + 4 * 22
    assert data[0] == lp.VERSION == 3 and struct.unpack_from("<HIH", data, 1) == (2, 5, 35840)
    bitmap = np.unpackbits(np.frombuffer(data, np.uint8, 384, 9), bitorder="little").astype(bool)
    assert np.array_equal(np.flatnonzero(bitmap[:1024]), slots0) and np.array_equal(bitmap[1024:], used[1024:3072])
    assert bitmap[0] and bitmap[5] and bitmap[1023] and bitmap[1024] and bitmap[3071]
    masks = struct.unpack_from("<%dI" % m, data, 9 + 384)
    assert all(masks[i] == sum(int(by_n[n, s]) << n for n in range(32)) for i, s in enumerate(slots0))
    assert masks[0] & 1 and masks[list(slots0).index(5)] == (1 << 3) | (1 << 17) and masks[-1] >> 31
    assert struct.unpack_from("<%dH" % k, data, 9 + 384 + 4 * m) == tuple(f1[used].tolist())      # ascending contexts
    table_end = 9 + 384 + 4 * m + 2 * k
    assert struct.unpack_from("<3I", data, table_end) == (5, 0, 17)
    side = lp.read(data)
    assert np.array_equal(side["f1"], f1) and np.array_equal(side["used"], used) and np.array_equal(side["states"], states)
    assert np.array_equal(side["words"], np.concatenate(words)) and side["states"].dtype == np.uint64
    assert side["nwords"].tolist() == [5, 0, 17] and side["group"] == 2 and side["n_blocks"] == 5
    assert lp.write(2, 5, f1[used], used, states.view(np.int64), [w.view(np.int32) for w in words]) == data

    def bad(blob, match, **kw):
        with pytest.raises(ValueError, match=match):
            lp.read(blob, **kw)
    patch = lambda at, fmt, *v: data[:at] + struct.pack(fmt, *v) + data[at + struct.calcsize(fmt):]
    bad(b"", "empty")
    bad(patch(0, "<B", 2), "version 2")
    bad(patch(0, "<B", 1), "version 1, this reader knows 3")
    bad(data[:5], "truncated header")
    bad(patch(1, "<H", 0), "group size 0")
    bad(patch(1, "<H", 2000), "group size 2000")
    bad(patch(3, "<I", 0), "no blocks")
    bad(data, "codes 5 blocks, the pack holds 6", n_blocks=6)
    bad(patch(7, "<H", 3072), "3072 contexts, this reader knows 35840")
    bad(data[:300], "truncated bitmap")
    bad(data[:9 + 384 + 4 * m - 2], "the bitmap names %d level-0 slots, %d masks follow" % (m, m - 1))
    bad(patch(9 + 384 + 4 * list(slots0).index(5), "<I", 0), "a neighbour mask of 0 for slot 5")
    bad(data[:9 + 384 + 4 * m + 10], "the bitmap and the masks name %d contexts" % k)
    bad(patch(9, "<384B", *[255] * 384)[:9 + 384 + 4 * m], "the bitmap names 1024 level-0 slots")
    # a bitmap or a mask that disagrees with what follows: everything behind it shifts, and some check says so
    bad(patch(9, "<B", data[9] ^ 2), "lossless_lod_pack: ")
    bad(patch(9 + 384, "<I", masks[0] ^ 4), "lossless_lod_pack: ")
    bad(patch(9 + 384 + 4 * m + 2 * 3, "<H", 0), "frequency of 0")
    bad(patch(table_end, "<I", 2 * 37376 + 1), "group 0 claims 74753 words")
    bad(patch(table_end + 8, "<I", 37376 + 1), "group 2 claims 37377 words")
    bad(patch(table_end, "<I", 6), "bytes, .* expected")
    bad(data[:-4], "bytes, .* expected")
    bad(data + b"\0", "bytes, .* expected")
    lp.read(patch(table_end + 8, "<I", 17))
    low = used.copy()
    low[7] = True                                                  # contexts 0..1023: no level of this table has them
    for args, match in (((0, 5, f1, used, states, words), "group 0 outside"), ((2, 0, f1, used, states, words), "block count"),
                        ((2, 5, f1, used[:3072], states, words), "35840 contexts"),
                        ((2, 5, f1, low, states, words), "contexts 0..1023 belong to no level"),
                        ((2, 5, f1[used][:-1], used, states, words), "the table names %d contexts, %d frequencies" % (k, k - 1)),
                        ((2, 5, np.where(np.arange(lp.CONTEXTS) == 3072, 0, f1), used, states, words), r"\[1, 65535\]"),
                        ((2, 5, np.where(np.arange(lp.CONTEXTS) == 3072, 65536, f1), used, states, words), r"\[1, 65535\]"),
                        ((2, 5, f1, used, states[:2], words), "3 groups"), ((2, 5, f1, used, states, words[:2]), "3 groups"),
                        ((2, 5, f1, used, states, [words[0], words[1], np.zeros(37377, np.uint32)]), "group 2 holds more words")):
        with pytest.raises(ValueError, match=match):
            lp.write(*args)


def test_the_reader_is_chosen_by_byte_0():
    from tests.test_lossless_lod_cpu import small_pack as small_field_pack
    data = small_pack()[-1]
    field = small_field_pack()[-1]
    assert lp.module_of(data) is lp and lp.module_of(field) is llp
    assert lp.module_of(data).read(data)["f1"].size == 35840 and lp.module_of(field).read(field)["f1"].size == 3072
    with pytest.raises(ValueError, match="lossless_lod_pack: version 3, this reader knows 1"):
        llp.read(data)                                             # the field reader keeps refusing what it does not know
    for v in (0, 2, 4, 255):
        with pytest.raises(ValueError, match="lossless_lod_pack: version %d, the readers know 1 .* and 3" % v):
            lp.module_of(bytes([v]) + data[1:])
    with pytest.raises(ValueError, match="empty"):
        lp.module_of(b"")


def test_parser_grows_only_by_the_new_flag_and_the_refusal_needs_no_device():
    import NVFPCC
    parse = NVFPCC.build_parser().parse_args
    for argv in (["decode", "pack.pk"], ["encode", "x.ply", "--lossless"], ["encode", "x.ply", "--lossless_lod"],
                 ["decode", "pack.pk", "--lossless_lod", "1"]):
        ns = parse(argv)
        assert not hasattr(ns, "lossless_ctx")
        for ctx in ("field", "nbr"):
            assert vars(parse(argv + ["--lossless_ctx", ctx])) == dict(vars(ns), lossless_ctx=ctx)
    with pytest.raises(SystemExit):
        parse(["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "faces"])
    NVFPCC.lossless_ctx_refusals(parse(["encode", "x.ply"]))
    NVFPCC.lossless_ctx_refusals(parse(["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "nbr"]))
    for argv in (["encode", "x.ply", "--lossless_ctx", "nbr"], ["encode", "x.ply", "--lossless", "--lossless_ctx", "field"]):
        with pytest.raises(SystemExit, match="--lossless_ctx .* chooses the contexts of --lossless_lod"):
            NVFPCC.lossless_ctx_refusals(parse(argv))
        with pytest.raises(SystemExit, match="--lossless_ctx .* chooses the contexts of --lossless_lod"):
            NVFPCC.encode(parse(argv))                             # before the device, the data or the weights are touched
