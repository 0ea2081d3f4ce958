"""Scalable lossless geometry, the host half: the numpy reference of the coarse-to-fine coder (tests/occ_hier_ref.py)
round-trips, stops exactly at the coarse levels on a prefix of the words, and stays inside its code-length bound on the
trained fixtures; the byte layout of lossless_lod_pack; the command line's flags.  tests/test_gpu_lossless_lod.py holds
the device to this reference byte for byte."""
import math
import struct

import numpy as np
import pytest

from nvfpcc_amd import lossless_lod_pack as lp
from tests import occ_hier_ref as H
from tests import occ_rans_ref as R
from tests.test_lossless_cpu import cases

VOX = 32768


def test_pyramid_children_and_fold():
    c = H.children(np.asarray([0, 7, 511]), 8)
    assert c[0].tolist() == [0, 1, 16, 17, 256, 257, 272, 273]
    assert c[1].tolist() == [14, 15, 30, 31, 270, 271, 286, 287] and c[2, 7] == 4095
    assert sorted(H.children(np.arange(4096), 16).reshape(-1).tolist()) == list(range(VOX))
    p = np.zeros((1, VOX), np.float32)
    kids = H.children(np.asarray([5]), 16)[0]
    p[0, kids] = [-0.0, 0.0, 0.6, 0.6, 0.7, 0.5, 0.9, 0.51]
    p[0, H.children(np.asarray([6]), 16)[0][3]] = np.float32(-0.0)
    p1, k1, p2, k2 = H.pyramid(p)
    assert p1[0, 5] == np.float32(0.9) and k1[0, 5] == 3           # five children above 0.5, clipped
    assert p1[0, 6] == 0 and not np.signbit(p1[0, 6]) and k1[0, 6] == 0     # the first of +0.0 / -0.0 stays
    p[0, H.children(np.asarray([6]), 16)[0][0]] = np.float32(-0.0)
    assert np.signbit(H.pyramid(p)[0][0, 6])
    assert p2[0, 2] == np.float32(0.9) and k2[0, 2] == 1 and p2[0, 3] == 0 and k2[0, 3] == 0      # cells 5, 6: X = 2, 3


@pytest.mark.parametrize("group", [1, 2, 64])
def test_reference_round_trips_and_stops_at_every_level(group):
    for name, p, gt in cases():
        assert not R.bad(p).any()
        cnt, occ = H.histogram(p, gt)
        assert int(cnt.sum()) == H.symbols_coded(p, gt) and np.all(occ <= cnt)
        f1 = H.table(cnt, occ)
        assert f1.min() >= 1 and f1.max() <= 65535 and np.all(f1[cnt == 0] == 32768)
        streams = H.encode(p, gt, f1, group)
        assert len(streams) == -(-p.shape[0] // group)
        pools = H.maxpool(gt)
        for g, (states, words) in enumerate(streams):
            sl = slice(g * group, (g + 1) * group)
            assert states.min() >= 1 << 31 and states.max() < 1 << 63
            assert words.size <= p[sl].shape[0] * H.BLOCK_WORDS
            occ0, final, used = H.decode_group(p[sl], f1, states, words)
            assert np.array_equal(occ0, pools[0][sl]), (name, g)
            assert np.all(final == np.uint64(1 << 31)) and used == words.size, (name, g)
            used2 = None
            for stop in (2, 1):
                got, _, used_l = H.decode_group(p[sl], f1, states, words, stop=stop)
                assert np.array_equal(got, pools[stop][sl]), (name, g, stop)
                # strict wherever the finer sections have something to say: a group of all-empty blocks has no finer
                # symbols at all, and one of all-full blocks may spend no whole word on them
                mixed = any(0 < int(b.sum()) < VOX for b in gt[sl])
                assert (used_l < words.size if mixed else used_l <= words.size), (name, g, stop)
                assert used2 is None or used2 <= used_l, (name, g, stop)
                # a strict prefix is all it reads: the words behind it may be anything, or missing
                again, _, n = H.decode_group(p[sl], f1, states, words[:used_l], stop=stop)
                assert n == used_l and np.array_equal(again, got)
                used2 = used_l


def test_an_empty_parent_costs_no_symbol():
    _, p, gt = next(cases())
    sections = H.group_sections(p[:3], gt[:3])
    g0, g1, g2 = H.maxpool(gt[:3])
    assert [s[0] for s in sections] == [2, 1, 0]
    assert sections[0][3].size == 3 * 512 and sections[1][3].size == 8 * int(g2.sum())
    assert sections[2][3].size == 8 * int(g1.sum()) and int(g2[1].sum()) == 0          # block 1 is empty: 512 symbols
    assert all(0 <= s[3].min() and s[3].max() < 3072 for s in sections)
    assert np.all(sections[2][3] < 1024) and np.all(sections[0][3] >= 2048)


def _trained(golden_dir, tag):
    """p of the 12 blocks of a trained fixture through the oracle (as tests/test_lossless_cpu.py::trained), and gt."""
    import torch
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    from oracle import nvf_oracle as O
    from tests.test_trained_golden import CFG, load_pack, state_from_pack
    pack, G = load_pack(golden_dir, tag)
    ch, channels = CFG[tag]
    P, _ = O.build_state(ch, channels, synthetic_seed())
    P.update(state_from_pack(pack))
    lat = torch.from_numpy(G["latents"][:12].astype(np.float32))
    torch.set_num_threads(8)
    with torch.no_grad():
        p = np.concatenate([O.decoder(P, lat[i:i + 1], 2)[0].reshape(1, -1).numpy() for i in range(12)])
    return p.astype(np.float32), make_blocks(12)[0].reshape(12, -1).astype(bool)


@pytest.mark.parametrize("tag", ["S", "W"])
def test_rate_and_code_length_bound_on_the_trained_fixtures(golden_dir, tag):
    """The ideal code length is below v1's on both fixtures, and stream bits <= ideal + 4096 per group (the flushed
    states) + log2(1 + 2^-15) per CODED symbol: v1's bound with the coded symbol count."""
    p, gt = _trained(golden_dir, tag)
    n_points = int(gt.sum())
    assert n_points == 11685
    v1_cnt, v1_occ = R.histogram(p, gt)
    v1 = R.ideal_bits(R.table(v1_cnt, v1_occ), v1_cnt, v1_occ)
    cnt, occ = H.histogram(p, gt)
    f1 = H.table(cnt, occ)
    live = cnt > 0
    ideal = H.ideal_bits(f1[live], cnt[live], occ[live])
    symbols = int(cnt.sum())
    print(f"{tag}: v1 ideal {v1 / n_points:.4f} bpp, new {ideal / n_points:.4f} bpp, {symbols} symbols, "
          f"{symbols / 64 / 12:.1f} steps per block, {int(live.sum())} contexts")
    assert ideal < v1
    assert symbols == 51072
    for group in (1, 4, 12):
        streams = H.encode(p, gt, f1, group)
        bits = sum(64 * 64 + 32 * w.size for _, w in streams)
        bound = ideal + 4096 * len(streams) + symbols * math.log2(1 + 2.0 ** -15)
        print(f"  group {group}: {bits} bits, bound {bound:.1f}, {bits / n_points:.4f} bpp")
        assert bits <= bound
        for g, (states, words) in enumerate(streams):
            sl = slice(g * group, (g + 1) * group)
            occ0, final, used = H.decode_group(p[sl], f1, states, words)
            assert np.array_equal(occ0, gt[sl]) and np.all(final == np.uint64(1 << 31)) and used == words.size
    # a stop after the 8^3 section reads a small prefix of the one group's words
    states, words = streams[0]
    got, _, used = H.decode_group(p, f1, states, words, stop=2)
    assert np.array_equal(got, H.maxpool(gt)[2]) and used < words.size // 8
    # the pack of these streams: the size formula, and write / read identity
    data = lp.write(12, 12, f1, live, states[None], [words])
    assert len(data) == lp.size(12, 12, words.size, int(live.sum())) == 9 + 384 + 2 * int(live.sum()) + 516 + 4 * words.size
    side = lp.read(data, 12)
    assert np.array_equal(side["f1"], f1) and np.array_equal(side["used"], live)
    assert np.array_equal(side["states"], states[None]) and np.array_equal(side["words"], words)


def test_table_rule_is_v1s_over_the_coded_symbols():
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 1 << 40, 3072)
    occ = (cnt * rng.random(3072)).astype(np.int64)
    cnt[:4], occ[:4] = [0, 5, 5, 1 << 40], [0, 0, 5, 1]
    f1, used = lp.table_from_counts(cnt, occ)
    assert f1 == R.table(cnt, occ).tolist() and f1[:4] == [32768, 1, 65535, 1] and used[:4] == [False, True, True, True]
    with pytest.raises(ValueError):
        lp.table_from_counts([1] * 3072, [2] * 3072)
    with pytest.raises(ValueError):
        lp.table_from_counts([1] * 256, [1] * 256)


def small_pack():
    rng = np.random.default_rng(1)
    used = rng.random(3072) < 0.1
    used[[0, 9, 3071]] = True
    f1 = np.where(used, rng.integers(1, 65536, 3072), 32768)
    states = rng.integers(1 << 31, 1 << 62, (3, 64)).astype(np.uint64)
    words = [rng.integers(0, 1 << 32, n).astype(np.uint32) for n in (5, 0, 17)]
    return f1, used, states, words, lp.write(2, 5, f1, used, states, words)


def test_pack_layout_and_every_malformed_case():
    f1, used, states, words, data = small_pack()
    k = int(used.sum())
    assert len(data) == lp.size(5, 2, 22, k) == 9 + 384 + 2 * k + 3 * 4 + 3 * 512 + 4 * 22
    assert data[0] == lp.VERSION and struct.unpack_from("<HIH", data, 1) == (2, 5, 3072)
    assert data[9] & 1 and data[10] & 2 and data[9 + 383] & 0x80            # contexts 0, 9 and 3071
    assert struct.unpack_from("<%dH" % k, data, 9 + 384) == tuple(f1[used].tolist())
    table_end = 9 + 384 + 2 * k
    assert struct.unpack_from("<3I", data, table_end) == (5, 0, 17)
    side = lp.read(data)
    assert np.array_equal(side["f1"], f1) and np.array_equal(side["used"], used) and np.array_equal(side["states"], states)
    assert np.array_equal(side["words"], np.concatenate(words)) and side["states"].dtype == np.uint64
    assert side["nwords"].tolist() == [5, 0, 17] and side["group"] == 2 and side["n_blocks"] == 5
    # the present frequencies alone, and int64 / int32 views of the same bits, as the device hands them over
    assert lp.write(2, 5, f1[used], used, states.view(np.int64), [w.view(np.int32) for w in words]) == data

    def bad(blob, match, **kw):
        with pytest.raises(ValueError, match=match):
            lp.read(blob, **kw)
    patch = lambda at, fmt, *v: data[:at] + struct.pack(fmt, *v) + data[at + struct.calcsize(fmt):]
    bad(b"", "empty")
    bad(patch(0, "<B", 2), "version 2")
    bad(data[:5], "truncated header")
    bad(patch(1, "<H", 0), "group size 0")
    bad(patch(1, "<H", 2000), "group size 2000")
    bad(patch(3, "<I", 0), "no blocks")
    bad(data, "codes 5 blocks, the pack holds 6", n_blocks=6)
    bad(patch(7, "<H", 256), "256 contexts")
    bad(data[:300], "truncated bitmap")
    bad(data[:9 + 384 + 10], "the bitmap names %d contexts" % k)
    bad(patch(9, "<384B", *[255] * 384)[:9 + 384 + 2 * k + 12], "the bitmap names 3072 contexts")
    bad(patch(9, "<B", data[9] ^ 2), "claims|expected")                          # a bitmap that disagrees with the table: what follows no longer fits
    bad(patch(9 + 384 + 2 * 3, "<H", 0), "frequency of 0")
    bad(patch(table_end, "<I", 2 * 37376 + 1), "group 0 claims 74753 words")
    bad(patch(table_end + 8, "<I", 37376 + 1), "group 2 claims 37377 words")      # the short last group: one block
    bad(patch(table_end, "<I", 6), "bytes, .* expected")                           # a word count too large
    bad(data[:-4], "bytes, .* expected")                                           # a truncated word list
    bad(data + b"\0", "bytes, .* expected")
    lp.read(patch(table_end + 8, "<I", 17))
    for args, match in (((0, 5, f1, used, states, words), "group 0 outside"), ((2, 0, f1, used, states, words), "block count"),
                        ((2, 5, f1, used[:100], states, words), "3072 contexts"),
                        ((2, 5, f1[used][:-1], used, states, words), "the bitmap names %d contexts, %d frequencies" % (k, k - 1)),
                        ((2, 5, np.where(np.arange(3072) == 9, 0, f1), used, states, words), r"\[1, 65535\]"),
                        ((2, 5, np.where(np.arange(3072) == 9, 65536, f1), used, states, words), r"\[1, 65535\]"),
                        ((2, 5, f1, used, states[:2], words), "3 groups"), ((2, 5, f1, used, states, words[:2]), "3 groups"),
                        ((2, 5, f1, used, states, [words[0], words[1], np.zeros(37377, np.uint32)]), "group 2 holds more words")):
        with pytest.raises(ValueError, match=match):
            lp.write(*args)


def test_status_and_line():
    lp.check_status(np.zeros(4, np.int32))
    with pytest.raises(ValueError, match=r"lossless_lod_pack: the stream of group 1 is damaged \(a read past the end of its words\); 1 of 3"):
        lp.check_status(np.asarray([0, 1, 0], np.int32))
    assert lp.lossless_lod_line(1000, 4000, 7000.0, 300, 51072, 64) == \
        "[LosslessLoD] bytes: 1000 bpp: 2.0000 ideal bpp: 1.7500 contexts: 300 symbols: 51072 group: 64"


def test_parser_grows_only_by_the_new_flag_and_refusals_need_no_device():
    import NVFPCC
    parse = NVFPCC.build_parser().parse_args
    for argv in (["decode", "pack.pk"], ["encode", "x.ply", "--lossless"], ["decode", "pack.pk", "--lod", "1"]):
        ns = parse(argv)
        assert not hasattr(ns, "lossless_lod")
        assert vars(parse(argv + ["--lossless_lod"])) == dict(vars(ns), lossless_lod=0)
    assert parse(["encode", "x.ply", "--lossless_lod"]).lossless_lod == 0
    assert [parse(["decode", "pack.pk", "--lossless_lod", str(l)]).lossless_lod for l in (0, 1, 2)] == [0, 1, 2]
    with pytest.raises(SystemExit):
        parse(["decode", "pack.pk", "--lossless_lod", "3"])
    with pytest.raises(SystemExit, match="--lossless_lod and --lod exclude each other"):
        NVFPCC.lossless_lod_refusals(parse(["decode", "pack.pk", "--lossless_lod", "1", "--lod", "1"]), None)
    with pytest.raises(SystemExit, match="--lossless_lod and --lossless exclude each other"):
        NVFPCC.lossless_lod_refusals(parse(["decode", "pack.pk", "--lossless_lod", "0", "--lossless"]), None)
    ns = parse(["decode", "pack.pk", "--lossless_lod", "2"])
    NVFPCC.lossless_lod_refusals(ns, None)
    with pytest.raises(SystemExit, match="decode --lossless_lod 2: pack.pk carries no lossless_lod_pack"):
        NVFPCC.lossless_lod_refusals(ns, {"net_weight_pack": {}, "latent_pack": {}, "lossless_pack": b""})
    NVFPCC.lossless_lod_refusals(ns, {"lossless_lod_pack": b""})
    NVFPCC.lossless_lod_refusals(parse(["decode", "pack.pk", "--lossless"]), {})
    # the existing refusal stands
    with pytest.raises(SystemExit, match="--lossless and --lod"):
        NVFPCC.lossless_refusals(parse(["decode", "pack.pk", "--lossless", "--lod", "1"]), None)
