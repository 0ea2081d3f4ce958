"""Scalable lossless geometry under the inter contexts, the host half: the numpy reference (tests/occ_inter_ref.py)
computes the temporal and the spatial class as defined, shares its first two sections with the field contexts' coder,
round-trips and stops exactly at the coarse levels on a strict prefix, holds its held-out rate against the neighbour
contexts' on the trained fixtures under four reference clouds and stays inside the code-length bound; the byte layout
of lossless_inter_pack, the dispatcher on byte 0, the command line's flags; reference_words against a dense scatter.
tests/test_gpu_lossless_inter.py holds the device to this reference byte for byte."""
import hashlib
import math
import struct

import numpy as np
import pytest

from nvfpcc_amd import lossless_inter_pack as lp
from nvfpcc_amd import lossless_lod_pack as llp
from nvfpcc_amd import lossless_nbr_pack as nbr
from tests import occ_hier_ref as H
from tests import occ_inter_ref as I
from tests import occ_nbr_ref as N
from tests import occ_rans_ref as R
from tests.test_lossless_cpu import cases
from tests.test_lossless_lod_cpu import _trained

VOX = 32768


def vox(z, y, x):
    return (z * 32 + y) * 32 + x


def cell1(z, y, x):
    return (z * 16 + y) * 16 + x


def only(*voxels, n=VOX, index=vox):
    return np.isin(np.arange(n), [index(*v) for v in voxels])[None]


def references(gt):
    """The reference clouds of the rate test for a cloud gt [nb, 32768]: the frame itself, moved by (1, 0, 0) and by
    (1, 2, 1) inside each block with zero fill, and another frame's blocks (permuted)."""
    return {"static": gt, "shift 1 0 0": I.shifted(gt, 1, 0, 0), "shift 1 2 1": I.shifted(gt, 1, 2, 1),
            "permuted": gt[np.random.default_rng(0).permutation(gt.shape[0])]}


def test_temporal_class_on_a_hand_made_block():
    r = lambda v, ref, blk=0: int(I.temporal_class(np.asarray([blk]), np.asarray([v]), ref)[0])
    empty, full = np.zeros((1, VOX), bool), np.ones((1, VOX), bool)
    v = (5, 6, 7)
    assert r(vox(*v), empty) == 0 and r(vox(*v), full) == 2
    assert r(vox(*v), only(v)) == 2                                 # the voxel in the reference alone
    for axis in range(3):
        for step in (-1, 1):
            q = list(v)
            q[axis] += step
            assert r(vox(*v), only(q)) == 1                        # a face neighbour alone
            assert r(vox(*v), only(q, v)) == 2
    for q in ((4, 5, 7), (6, 6, 8), (5, 7, 6), (4, 5, 6), (6, 7, 8), (5, 6, 9), (7, 6, 7)):
        assert r(vox(*v), only(q)) == 0                            # edge and corner neighbours, and two steps away
    # a voxel on a block face does not see the next block's reference: rows wrap neither along x nor along y, z
    assert r(vox(3, 3, 31), only((3, 4, 0))) == 0 and r(vox(3, 3, 0), only((3, 2, 31))) == 0
    assert r(vox(3, 31, 5), only((4, 0, 5))) == 0 and r(vox(3, 0, 5), only((2, 31, 5))) == 0
    assert r(vox(0, 0, 0), only((0, 0, 1))) == r(vox(31, 31, 31), only((31, 31, 30))) == 1
    two = np.concatenate([empty, full])
    assert r(vox(31, 31, 31), two, 0) == 0 and r(vox(0, 0, 0), two, 1) == 2
    assert r(vox(0, 0, 0), two[::-1], 1) == 0 and r(vox(31, 31, 31), two[::-1], 0) == 2


def test_spatial_class_on_version_3s_hand_made_cases():
    """s = (F * 2 + (E > 0)) * 2 + C on the cases of tests/test_lossless_nbr_cpu.py."""
    full, empty = np.ones((1, 4096), bool), np.zeros((1, 4096), bool)
    s = lambda v, occ1, blk=0: int(I.spatial_class(np.asarray([blk]), np.asarray([v]), occ1)[0])
    cells = lambda *c: only(*c, n=4096, index=cell1)
    fold = lambda F, E, C: (F * 2 + (E > 0)) * 2 + C
    assert s(vox(0, 0, 0), full) == 0 and s(vox(31, 31, 31), full) == 0
    assert s(vox(3, 3, 3), full) == s(vox(2, 2, 2), full) == fold(3, 3, 1) == 15 and s(vox(3, 3, 3), empty) == 0
    assert s(vox(3, 3, 3), cells((2, 1, 1))) == s(vox(3, 3, 3), cells((1, 2, 1))) == s(vox(3, 3, 3), cells((1, 1, 2))) == fold(1, 0, 0) == 4
    assert s(vox(3, 3, 3), cells((2, 2, 1))) == s(vox(3, 3, 3), cells((2, 1, 2))) == s(vox(3, 3, 3), cells((1, 2, 2))) == fold(0, 1, 0) == 2
    assert s(vox(3, 3, 3), cells((2, 2, 1), (2, 1, 2), (1, 2, 2))) == fold(0, 3, 0) == 2       # the edge count is a bit
    assert s(vox(3, 3, 3), cells((2, 2, 2))) == 1
    assert s(vox(3, 3, 3), cells((2, 1, 1), (1, 2, 1), (1, 2, 2))) == fold(2, 1, 0) == 10
    assert s(vox(3, 3, 3), cells((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0))) == 0
    assert s(vox(2, 3, 2), cells((0, 1, 1))) == 4 and s(vox(2, 3, 2), cells((0, 2, 1))) == 2
    assert s(vox(2, 3, 2), cells((0, 2, 0))) == 1 and s(vox(2, 3, 2), cells((2, 1, 1), (1, 0, 1), (1, 1, 2))) == 0
    assert s(vox(3, 3, 31), full) == fold(2, 1, 0) and s(vox(3, 31, 31), full) == fold(1, 0, 0)
    # every class of version 3 folds as defined
    rng = np.random.default_rng(5)
    occ1 = rng.random((2, 4096)) < 0.5
    blk, cell = rng.integers(0, 2, 4000), rng.integers(0, VOX, 4000)
    n = N.neighbour_class(blk, cell, occ1)
    assert np.array_equal(I.spatial_class(blk, cell, occ1), ((n >> 3) * 2 + (((n >> 1) & 3) > 0)) * 2 + (n & 1))
    assert set(I.spatial_class(blk, cell, occ1).tolist()) == set(range(16))


def test_contexts_of_the_three_sections():
    _, p, gt = next(cases())
    ref = I.shifted(gt[:3], 0, 1, 0)
    sections = I.group_sections(p[:3], gt[:3], ref)
    old = H.group_sections(p[:3], gt[:3])
    assert [s[0] for s in sections] == [2, 1, 0]
    for new, was in zip(sections[:2], old[:2]):                    # sections 2 and 1: the field contexts' own
        assert all(np.array_equal(a, b) for a, b in zip(new[1:], was[1:]))
    blk, cell, ctx = sections[2][1:4]
    assert np.array_equal(blk, old[2][1]) and np.array_equal(cell, old[2][2])
    assert ctx.min() >= 3072 and ctx.max() < I.CONTEXTS == 52224 == lp.CONTEXTS
    assert np.array_equal((ctx - 3072) % 1024, old[2][3])
    t = (ctx - 3072) // 1024
    assert np.array_equal(t // 16, I.temporal_class(blk, cell, ref))
    assert np.array_equal(t % 16, I.spatial_class(blk, cell, H.maxpool(gt[:3])[1]))
    assert set((t // 16).tolist()) == {0, 1, 2} and len(np.unique(t)) > 24


@pytest.mark.parametrize("group", [1, 2, 64])
def test_reference_round_trips_and_stops_at_every_level(group):
    for name, p, gt in cases():
        ref = I.shifted(gt, 1, 0, 0)
        ref[0] = gt[0]                                             # a block that stands still, an empty and a full one
        ref[1], ref[-1] = True, False
        cnt, occ = I.histogram(p, gt, ref)
        assert int(cnt.sum()) == I.symbols_coded(p, gt) and np.all(occ <= cnt) and not cnt[:1024].any()
        hc, ho = H.histogram(p, gt)
        assert np.array_equal(cnt[1024:3072], hc[1024:]) and np.array_equal(occ[1024:3072], ho[1024:])
        assert np.array_equal(cnt[3072:].reshape(48, 1024).sum(0), hc[:1024])
        assert np.array_equal(occ[3072:].reshape(48, 1024).sum(0), ho[:1024])
        f1 = I.table(cnt, occ)
        streams = I.encode(p, gt, ref, f1, group)
        assert len(streams) == -(-p.shape[0] // group)
        pools = H.maxpool(gt)
        for g, (states, words) in enumerate(streams):
            sl = slice(g * group, (g + 1) * group)
            assert states.min() >= 1 << 31 and states.max() < 1 << 63
            assert words.size <= p[sl].shape[0] * I.BLOCK_WORDS
            occ0, final, used = I.decode_group(p[sl], ref[sl], f1, states, words)
            assert np.array_equal(occ0, pools[0][sl]), (name, g)
            assert np.all(final == np.uint64(1 << 31)) and used == words.size, (name, g)
            for stop in (2, 1):
                got, x_l, used_l = I.decode_group(p[sl], ref[sl], f1, states, words, stop=stop)
                assert np.array_equal(got, pools[stop][sl]), (name, g, stop)
                mixed = any(0 < int(b.sum()) < VOX for b in gt[sl])     # as tests/test_lossless_lod_cpu.py
                assert (used_l < words.size if mixed else used_l <= words.size), (name, g, stop)
                again, _, k = I.decode_group(p[sl], ref[sl], f1, states, words[:used_l], stop=stop)
                assert k == used_l and np.array_equal(again, got)
                # the first two sections are the field coder's, given the same table entries: word for word
                was, x_h, used_h = H.decode_group(p[sl], f1[:3072], states, words, stop=stop)
                assert used_h == used_l and np.array_equal(was, got) and np.array_equal(x_h, x_l)


@pytest.mark.parametrize("tag", ["S", "W"])
def test_rate_and_code_length_bound_on_the_trained_fixtures(golden_dir, tag):
    """Held out (a table from the even blocks codes the odd ones and back; the reference's blocks go with the cloud's)
    against the neighbour contexts on the same blocks, the inter contexts spend at most 0.35 of the bits under the frame
    itself (measured 0.263 on S, 0.254 on W: 2.6665 -> 0.7010 and 2.3372 -> 0.5938 bpp), at most 0.95 under the frame
    moved by (1, 0, 0) (0.905, 0.913: 2.4133 and 2.1336 bpp) and at most 1.04 under another frame's blocks (1.022, 1.020:
    2.7253 and 2.3837 bpp) -- the price of folding 32 neighbour classes into 16.  Under (1, 2, 1): 2.7419 and 2.4306 bpp,
    printed.  Stream bits <= ideal + 4096 per group + log2(1 + 2^-15) per coded symbol, as for the other contexts."""
    p, gt = _trained(golden_dir, tag)
    n_points = int(gt.sum())
    assert n_points == 11685
    held_nbr = N.held_out_bits(N.group_sections, N.CONTEXTS, p, gt)
    symbols = I.symbols_coded(p, gt)
    assert symbols == 51072
    bounds = {"static": 0.35, "shift 1 0 0": 0.95, "shift 1 2 1": None, "permuted": 1.04}
    held = {}
    for name, ref in references(gt).items():
        held[name] = I.held_out_bits(p, gt, ref)
        cnt, occ = I.histogram(p, gt, ref)
        f1 = I.table(cnt, occ)
        live = cnt > 0
        ideal = I.ideal_bits(f1[live], cnt[live], occ[live])
        print(f"{tag} {name}: held out {held_nbr / n_points:.4f} -> {held[name] / n_points:.4f} bpp (x "
              f"{held[name] / held_nbr:.3f}), in sample {ideal / n_points:.4f} ideal bpp, {int(live.sum())} contexts")
        assert int(cnt.sum()) == symbols
        for group in (4, 12):
            streams = I.encode(p, gt, ref, f1, group)
            bits = sum(64 * 64 + 32 * w.size for _, w in streams)
            bound = ideal + 4096 * len(streams) + symbols * math.log2(1 + 2.0 ** -15)
            print(f"  group {group}: {bits} bits, bound {bound:.1f}, {bits / n_points:.4f} bpp")
            assert bits <= bound
            for g, (s, w) in enumerate(streams):
                sl = slice(g * group, (g + 1) * group)
                occ0, final, used = I.decode_group(p[sl], ref[sl], f1, s, w)
                assert np.array_equal(occ0, gt[sl]) and np.all(final == np.uint64(1 << 31)) and used == w.size
        if name == "static":                                       # the pack of it: size, and what read gives back
            slots0 = int(live[3072:].reshape(48, 1024).any(0).sum())
            states, words = streams[0]
            dg = lp.digest(H.words_of(ref))
            data = lp.write(12, 12, dg, f1, live, states[None], [words])
            assert len(data) == lp.size(12, 12, words.size, int(live.sum()), slots0) == \
                9 + 32 + 384 + 8 * slots0 + 2 * int(live.sum()) + 516 + 4 * words.size
            side = lp.read(data, 12)
            assert side["digest"] == dg and np.array_equal(side["f1"], f1) and np.array_equal(side["used"], live)
            assert np.array_equal(side["states"], states[None]) and np.array_equal(side["words"], words)
    for name, bound in bounds.items():
        if bound is not None:
            assert held[name] <= bound * held_nbr, (name, held[name] / held_nbr)


def test_table_rule_is_v1s_over_the_coded_symbols():
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 1 << 40, lp.CONTEXTS)
    occ = (cnt * rng.random(lp.CONTEXTS)).astype(np.int64)
    cnt[:4], occ[:4] = [0, 5, 5, 1 << 40], [0, 0, 5, 1]
    f1, used = lp.table_from_counts(cnt, occ)
    assert np.array_equal(f1, R.table(cnt, occ)) and f1[:4].tolist() == [32768, 1, 65535, 1]
    assert used[:4].tolist() == [False, True, True, True] and np.array_equal(used, cnt > 0)
    for c, o in (([1] * 35840, [1] * 35840), ([1] * lp.CONTEXTS, [2] * lp.CONTEXTS), ([0] * lp.CONTEXTS, [0] * 9 + [1] * (lp.CONTEXTS - 9))):
        with pytest.raises(ValueError, match="52224 pairs with 0 <= occupied <= symbols"):
            lp.table_from_counts(c, o)


DIGEST = hashlib.sha256(b"a reference").digest()


def small_pack():
    rng = np.random.default_rng(1)
    used = rng.random(lp.CONTEXTS) < 0.01
    used[:1024] = False
    used[[1024, 3071, 3072, 3072 + 47 * 1024 + 1023]] = True      # slots 0 (t = 0) and 1023 (t = 47) among them
    used[3072 + 5::1024] = False
    used[[3072 + 5 + 3 * 1024, 3072 + 5 + 33 * 1024]] = True      # slot 5: t = 3 and 33, the second past a uint32
    f1 = np.where(used, rng.integers(1, 65536, lp.CONTEXTS), 32768)
    states = rng.integers(1 << 31, 1 << 62, (3, 64)).astype(np.uint64)
    words = [rng.integers(0, 1 << 32, n).astype(np.uint32) for n in (5, 0, 17)]
    return f1, used, states, words, lp.write(2, 5, DIGEST, f1, used, states, words)


def test_pack_layout_and_every_malformed_case():
    f1, used, states, words, data = small_pack()
    k = int(used.sum())
    by_t = used[3072:].reshape(48, 1024)
    slots0 = np.flatnonzero(by_t.any(0))
    m = slots0.size
    assert len(data) == lp.size(5, 2, 22, k, m) == 9 + 32 + 384 + 8 * m + 2 * k + 3 * 4 + 3 * 512 + 4 * 22
    assert data[0] == lp.VERSION == 4 and struct.unpack_from("<HIH", data, 1) == (2, 5, 52224)
    assert data[9:41] == DIGEST                                    # the digest's place: right behind the header
    bitmap = np.unpackbits(np.frombuffer(data, np.uint8, 384, 41), bitorder="little").astype(bool)
    assert np.array_equal(np.flatnonzero(bitmap[:1024]), slots0) and np.array_equal(bitmap[1024:], used[1024:3072])
    assert bitmap[0] and bitmap[5] and bitmap[1023] and bitmap[1024] and bitmap[3071]
    masks = struct.unpack_from("<%dQ" % m, data, 41 + 384)
    assert all(masks[i] == sum(int(by_t[t, s]) << t for t in range(48)) for i, s in enumerate(slots0))
    assert masks[0] & 1 and masks[list(slots0).index(5)] == (1 << 3) | (1 << 33) and masks[-1] >> 47 == 1
    assert struct.unpack_from("<%dH" % k, data, 41 + 384 + 8 * m) == tuple(f1[used].tolist())     # ascending contexts
    table_end = 41 + 384 + 8 * m + 2 * k
    assert struct.unpack_from("<3I", data, table_end) == (5, 0, 17)
    side = lp.read(data)
    assert side["digest"] == DIGEST
    assert np.array_equal(side["f1"], f1) and np.array_equal(side["used"], used) and np.array_equal(side["states"], states)
    assert np.array_equal(side["words"], np.concatenate(words)) and side["states"].dtype == np.uint64
    assert side["nwords"].tolist() == [5, 0, 17] and side["group"] == 2 and side["n_blocks"] == 5
    assert lp.write(2, 5, DIGEST, f1[used], used, states.view(np.int64), [w.view(np.int32) for w in words]) == data

    def bad(blob, match, **kw):
        with pytest.raises(ValueError, match=match):
            lp.read(blob, **kw)
    patch = lambda at, fmt, *v: data[:at] + struct.pack(fmt, *v) + data[at + struct.calcsize(fmt):]
    at5 = 41 + 384 + 8 * list(slots0).index(5)
    bad(b"", "empty")
    bad(patch(0, "<B", 2), "version 2")
    bad(patch(0, "<B", 3), "version 3, this reader knows 4")
    bad(data[:5], "truncated header")
    bad(patch(1, "<H", 0), "group size 0")
    bad(patch(1, "<H", 2000), "group size 2000")
    bad(patch(3, "<I", 0), "no blocks")
    bad(data, "codes 5 blocks, the pack holds 6", n_blocks=6)
    bad(patch(7, "<H", 35840), "35840 contexts, this reader knows 52224")
    bad(data[:30], "truncated digest")
    bad(data[:300], "truncated bitmap")
    bad(data[:41 + 384 + 8 * m - 2], "the bitmap names %d level-0 slots, %d masks follow" % (m, m - 1))
    bad(patch(at5, "<Q", 0), "a class mask of 0 for slot 5")
    bad(patch(at5, "<Q", (1 << 3) | (1 << 48)), "a class mask with a bit at or above 48 for slot 5")
    bad(patch(at5, "<Q", (1 << 3) | (1 << 63)), "a class mask with a bit at or above 48 for slot 5")
    bad(data[:41 + 384 + 8 * m + 10], "the bitmap and the masks name %d contexts" % k)
    bad(patch(41, "<384B", *[255] * 384)[:41 + 384 + 8 * m], "the bitmap names 1024 level-0 slots")
    # a bitmap or a mask that disagrees with what follows: everything behind it shifts, and some check says so
    bad(patch(41, "<B", data[41] ^ 2), "lossless_lod_pack: ")
    bad(patch(41 + 384, "<Q", masks[0] ^ 4), "lossless_lod_pack: ")
    bad(patch(41 + 384 + 8 * m + 2 * 3, "<H", 0), "frequency of 0")
    bad(patch(table_end, "<I", 2 * 37376 + 1), "group 0 claims 74753 words")
    bad(patch(table_end + 8, "<I", 37376 + 1), "group 2 claims 37377 words")
    bad(patch(table_end, "<I", 6), "bytes, .* expected")
    bad(data[:-4], "bytes, .* expected")
    bad(data + b"\0", "bytes, .* expected")
    lp.read(patch(table_end + 8, "<I", 17))
    assert lp.read(patch(9, "<B", data[9] ^ 1))["digest"] != DIGEST    # the digest is carried, the device half judges it
    low = used.copy()
    low[7] = True                                                  # contexts 0..1023: no level of this table has them
    for args, match in (((0, 5, DIGEST, f1, used, states, words), "group 0 outside"),
                        ((2, 0, DIGEST, f1, used, states, words), "block count"),
                        ((2, 5, DIGEST[:31], f1, used, states, words), "digest is 32 bytes"),
                        ((2, 5, DIGEST, f1, used[:35840], states, words), "52224 contexts"),
                        ((2, 5, DIGEST, f1, low, states, words), "contexts 0..1023 belong to no level"),
                        ((2, 5, DIGEST, f1[used][:-1], used, states, words), "the table names %d contexts, %d frequencies" % (k, k - 1)),
                        ((2, 5, DIGEST, np.where(np.arange(lp.CONTEXTS) == 3072, 0, f1), used, states, words), r"\[1, 65535\]"),
                        ((2, 5, DIGEST, np.where(np.arange(lp.CONTEXTS) == 3072, 65536, f1), used, states, words), r"\[1, 65535\]"),
                        ((2, 5, DIGEST, f1, used, states[:2], words), "3 groups"),
                        ((2, 5, DIGEST, f1, used, states, words[:2]), "3 groups"),
                        ((2, 5, DIGEST, f1, used, states, [words[0], words[1], np.zeros(37377, np.uint32)]), "group 2 holds more words")):
        with pytest.raises(ValueError, match=match):
            lp.write(*args)


def test_digest_is_sha256_over_the_little_endian_words():
    import torch
    rng = np.random.default_rng(2)
    words = rng.integers(0, 1 << 63, (3, 512)).astype(np.uint64)
    words[0, 0] = np.uint64((1 << 64) - 1)
    want = hashlib.sha256(words.astype("<u8").tobytes()).digest()
    assert lp.digest(words) == lp.digest(words.view(np.int64)) == lp.digest(torch.from_numpy(words.view(np.int64))) == want
    assert lp.digest(words[:, ::-1]) != want
    one = words.copy()
    one[2, 511] ^= np.uint64(1 << 17)
    assert lp.digest(one) != want
    for wrong in (words[:, :511], words.astype(np.int32), words.reshape(-1)):
        with pytest.raises(ValueError, match=r"64-bit \[N, 512\]"):
            lp.digest(wrong)


def test_the_reader_is_chosen_by_byte_0():
    from tests.test_lossless_lod_cpu import small_pack as small_field_pack
    from tests.test_lossless_nbr_cpu import small_pack as small_nbr_pack
    data = small_pack()[-1]
    field, three = small_field_pack()[-1], small_nbr_pack()[-1]
    assert lp.module_of(data) is lp and lp.module_of(field) is llp and lp.module_of(three) is nbr
    assert lp.module_of(data).read(data)["f1"].size == 52224 and lp.module_of(three).read(three)["f1"].size == 35840
    assert lp.module_of(field).read(field)["f1"].size == 3072
    with pytest.raises(ValueError, match="lossless_lod_pack: version 4, this reader knows 3"):
        nbr.read(data)                                             # the other readers keep refusing what they do not know
    with pytest.raises(ValueError, match="lossless_lod_pack: version 4, this reader knows 1"):
        llp.read(data)
    for v in (0, 2, 5, 255):
        with pytest.raises(ValueError, match="lossless_lod_pack: version %d, the readers know" % v):
            lp.module_of(bytes([v]) + data[1:])
    with pytest.raises(ValueError, match="empty"):
        lp.module_of(b"")


def test_parser_grows_only_by_the_new_choice_and_flag_and_the_refusals_need_no_device():
    import NVFPCC
    parse = NVFPCC.build_parser().parse_args
    for argv in (["decode", "pack.pk"], ["encode", "x.ply", "--lossless"], ["encode", "x.ply", "--lossless_lod"],
                 ["decode", "pack.pk", "--lossless_lod", "1"], ["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "nbr"]):
        ns = parse(argv)
        assert not hasattr(ns, "lossless_ref")
        assert vars(parse(argv + ["--lossless_ref", "prev.ply"])) == dict(vars(ns), lossless_ref="prev.ply")
    ns = parse(["encode", "x.ply", "--lossless_lod"])
    assert vars(parse(["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "inter"])) == dict(vars(ns), lossless_ctx="inter")
    with pytest.raises(SystemExit):
        parse(["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "temporal"])
    inter = ["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "inter"]
    NVFPCC.lossless_ctx_refusals(parse(inter + ["--lossless_ref", "prev.ply"]))
    NVFPCC.lossless_ctx_refusals(parse(["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "nbr"]))
    NVFPCC.lossless_ctx_refusals(parse(["decode", "pack.pk", "--lossless_lod", "0"]))
    for argv, match in ((inter, "--lossless_ctx inter codes the voxels under a reference cloud; name it with --lossless_ref"),
                        (["encode", "x.ply", "--lossless_lod", "--lossless_ref", "prev.ply"],
                         "--lossless_ref prev.ply is the reference of --lossless_ctx inter"),
                        (["encode", "x.ply", "--lossless_lod", "--lossless_ctx", "nbr", "--lossless_ref", "prev.ply"],
                         "--lossless_ref prev.ply is the reference of --lossless_ctx inter"),
                        (["encode", "x_%d.ply", "--gof", "2"] + inter[2:] + ["--lossless_ref", "prev.ply"],
                         "--gof and --lossless_ctx inter exclude each other"),
                        (["encode", "x.ply", "--lossless_ctx", "inter", "--lossless_ref", "prev.ply"],
                         "--lossless_ctx inter chooses the contexts of --lossless_lod")):
        with pytest.raises(SystemExit, match=match):
            NVFPCC.lossless_ctx_refusals(parse(argv))
        with pytest.raises(SystemExit, match=match):
            NVFPCC.encode(parse(argv))                             # before the device, the data or the weights are touched


def test_reference_words_against_a_dense_scatter():
    """The numpy reference_words against a dense volume: dropped points, duplicates, origins at 12 bits."""
    rng = np.random.default_rng(11)
    origins = np.asarray([[4064, 4064, 4064], [0, 0, 0], [32, 4064, 0], [2048, 96, 4032], [0, 0, 32]])
    inside = origins[rng.integers(0, 5, 3000)] + rng.integers(0, 32, (3000, 3))
    outside = np.asarray([[64, 0, 0], [0, 32, 0], [4095, 4095, 4031], [-1, 0, 0], [0, 0, -32], [4096, 4064, 4064], [31, 31, 64]])
    corners = np.asarray([[4095, 4095, 4095], [0, 0, 0], [31, 31, 31], [0, 0, 63], [63, 4095, 31]])
    points = np.concatenate([inside, outside, corners, inside[:500], outside[:3]])      # duplicates of both kinds
    points = points[rng.permutation(len(points))]
    ref, dropped = I.reference_words(points, origins)
    assert dropped == 10 and ref.shape == (5, VOX)
    want = np.zeros((5, 32, 32, 32), bool)
    for b, o in enumerate(origins):                                # a dense scatter per block, by comparison not by key
        rel = points - o
        keep = ((rel >= 0) & (rel < 32)).all(1)
        want[b][tuple(rel[keep].T)] = True
    assert np.array_equal(ref, want.reshape(5, VOX))
    assert ref[0, VOX - 1] and ref[1, 0] and ref[1, VOX - 1] and ref[4, 31] and ref[2, vox(31, 31, 31)]
    assert int(ref.sum()) == len(np.unique(np.concatenate([inside, corners]), axis=0))
    words = H.words_of(ref)
    assert words.shape == (5, 512) and int(words[1, 0]) & 1 and int(words[0, 511]) >> 63 == 1
    none, dropped = I.reference_words(np.zeros((0, 3), np.int64), origins)
    assert dropped == 0 and not none.any()
