"""Lossless geometry, the host half: the numpy reference of the coder (tests/occ_rans_ref.py) round-trips and stays
inside its code-length bound on the trained fixture, the byte layout of lossless_pack, and the command line's flags.
tests/test_gpu_lossless.py holds the device to this reference byte for byte."""
import math
import struct

import numpy as np
import pytest
import torch

from nvfpcc_amd import lossless_pack as lp
from tests import occ_rans_ref as R

VOX = 32768


def adversarial_p(rng, n_blocks):
    """Probabilities that sit on every edge of the context function: exactly 0, 1 and 0.5, their neighbours, denormals,
    -0.0, and random values over the whole exponent range."""
    p = rng.random((n_blocks, VOX), dtype=np.float32)
    p = np.where(rng.random(p.shape) < 0.5, p ** 8, 1.0 - p ** 8).astype(np.float32)
    special = np.asarray([0.0, 1.0, 0.5, -0.0, 1e-45, 1e-40, 1.1754944e-38, np.nextafter(np.float32(0.5), np.float32(1)),
                          np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(1), np.float32(0)),
                          2.0 ** -127, 2.0 ** -126, 2.0 ** -64, 0.25, 0.75], np.float32)
    where = rng.random(p.shape) < 0.3
    p[where] = rng.choice(special, int(where.sum()))
    return p


def cases():
    rng = np.random.default_rng(7)
    p = adversarial_p(rng, 5)
    gt = rng.random(p.shape) < np.where(p > 0.5, 0.9, 0.1)
    gt[1] = False                       # an all-empty and an all-full block
    gt[3] = True
    yield "adversarial", p, gt
    p = rng.random((3, VOX), dtype=np.float32)
    yield "random", p, rng.random(p.shape) < p


@pytest.mark.parametrize("group", [1, 2, 64])
def test_reference_round_trips_at_every_group_size(group):
    for name, p, gt in cases():
        assert not R.bad(p).any()
        f1 = R.table(*R.histogram(p, gt))
        assert f1.min() >= 1 and f1.max() <= 65535
        streams = R.encode(p, gt, f1, group)
        assert len(streams) == -(-p.shape[0] // group)
        for g, (states, words) in enumerate(streams):
            pg = p[g * group:(g + 1) * group].reshape(-1)
            assert states.min() >= 1 << 31 and states.max() < 1 << 63
            sym, final, used = R.decode_group(pg, f1, states, words)
            assert np.array_equal(sym, gt[g * group:(g + 1) * group].reshape(-1)), (name, g)
            assert np.all(final == np.uint64(1 << 31)) and used == words.size, (name, g)


def test_context_function_edges():
    f = lambda v: int(R.contexts(np.asarray([v], np.float32))[0])
    assert f(0.5) == 0 and f(np.nextafter(np.float32(0.5), np.float32(1))) == 3      # side 1 has q < 0.5: context 1 is never used
    assert f(0.0) == 254 and f(1.0) == 255 and f(1e-45) == 254
    assert f(-0.0) == 0                 # no input error (it counts as +0.0 there), and its sign bit makes the key large
    assert f(0.25) == 8 and f(0.75) == 9 and f(0.3) == 8 and f(0.4) == 4
    assert R.bad(np.asarray([np.nan, -1e-9, 1.0000001, 2.0, -0.0, 0.0, 1.0], np.float32)).tolist() == [1, 1, 1, 1, 0, 0, 0]
    # every bit pattern has a context
    allbits = (np.arange(0, 1 << 32, 65537, dtype=np.uint64).astype(np.uint32)).view(np.float32)
    c = R.contexts(allbits)
    assert c.min() >= 0 and c.max() <= 255


def test_table_rule_is_the_modules():
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 1 << 40, 256)
    occ = (cnt * rng.random(256)).astype(np.int64)
    cnt[:4], occ[:4] = [0, 5, 5, 1 << 40], [0, 0, 5, 1]
    f1 = lp.table_from_counts(cnt, occ)
    assert f1 == R.table(cnt, occ).tolist() and f1[:4] == [32768, 1, 65535, 1]
    assert abs(lp.ideal_bits(f1, cnt, occ) - R.ideal_bits(f1, cnt, occ)) <= 1e-9 * R.ideal_bits(f1, cnt, occ)
    with pytest.raises(ValueError):
        lp.table_from_counts([1] * 256, [2] * 256)


@pytest.fixture(scope="module")
def trained(golden_dir):
    """p of the 12 blocks of the trained S fixture through the oracle (as tests/test_trained_golden.py), and their gt."""
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    from oracle import nvf_oracle as O
    from tests.test_trained_golden import CFG, load_pack, state_from_pack
    pack, G = load_pack(golden_dir, "S")
    ch, channels = CFG["S"]
    P, _ = O.build_state(ch, channels, synthetic_seed())
    P.update(state_from_pack(pack))
    lat = torch.from_numpy(G["latents"][:12].astype(np.float32))
    torch.set_num_threads(8)
    with torch.no_grad():
        p = np.concatenate([O.decoder(P, lat[i:i + 1], 2)[0].reshape(1, -1).numpy() for i in range(12)])
    gt = make_blocks(12)[0].reshape(12, -1).astype(bool)
    return p.astype(np.float32), gt


@pytest.mark.parametrize("group", [1, 4, 12])
def test_code_length_bound_on_the_trained_fixture(trained, group):
    """stream bits <= ideal + 4096 per group (the flushed states) + log2(1 + 2^-15) per symbol (the state is never
    below 2^31 and f <= 2^16, so x -> (x / f) * 65536 + x % f + start loses at most that much per step)."""
    p, gt = trained
    assert int(gt.sum()) == 11685
    cnt, occ = R.histogram(p, gt)
    f1 = R.table(cnt, occ)
    ideal = R.ideal_bits(f1, cnt, occ)
    streams = R.encode(p, gt, f1, group)
    bits = sum(64 * 64 + 32 * w.size for _, w in streams)
    bound = ideal + 4096 * len(streams) + p.size * math.log2(1 + 2.0 ** -15)
    print(f"group {group}: {bits} bits, ideal {ideal:.1f}, bound {bound:.1f}, {bits / gt.sum():.4f} bpp")
    assert bits <= bound
    for g, (states, words) in enumerate(streams):
        sym, final, used = R.decode_group(p[g * group:(g + 1) * group].reshape(-1), f1, states, words)
        assert np.array_equal(sym, gt[g * group:(g + 1) * group].reshape(-1))
        assert np.all(final == np.uint64(1 << 31)) and used == words.size
    # the pack of these streams: the size formula, and write / read identity
    data = lp.write(group, 12, f1, np.stack([s for s, _ in streams]), [w for _, w in streams])
    assert len(data) == lp.size(12, group, sum(w.size for _, w in streams)) == 9 + 512 + 516 * len(streams) + 4 * sum(w.size for _, w in streams)
    side = lp.read(data, 12)
    assert side["group"] == group and side["n_blocks"] == 12 and np.array_equal(side["f1"], f1)
    assert np.array_equal(side["states"], np.stack([s for s, _ in streams]))
    assert np.array_equal(side["words"], np.concatenate([w for _, w in streams]))
    assert side["nwords"].tolist() == [w.size for _, w in streams]


def small_pack():
    rng = np.random.default_rng(1)
    f1 = rng.integers(1, 65536, 256)
    states = rng.integers(1 << 31, 1 << 62, (3, 64)).astype(np.uint64)
    words = [rng.integers(0, 1 << 32, n).astype(np.uint32) for n in (5, 0, 17)]
    return f1, states, words, lp.write(2, 5, f1, states, words)


def test_pack_layout_and_every_malformed_case():
    f1, states, words, data = small_pack()
    assert len(data) == lp.size(5, 2, 22) == 9 + 512 + 3 * 4 + 3 * 512 + 4 * 22
    assert data[0] == lp.VERSION and struct.unpack_from("<HIH", data, 1) == (2, 5, 256)
    assert struct.unpack_from("<3I", data, 9 + 512) == (5, 0, 17)
    side = lp.read(data)
    assert np.array_equal(side["f1"], f1) and np.array_equal(side["states"], states)
    assert np.array_equal(side["words"], np.concatenate(words)) and side["states"].dtype == np.uint64
    # int64 / int32 views of the same bits, as the device hands them over
    assert lp.write(2, 5, f1, states.view(np.int64), [w.view(np.int32) for w in words]) == data

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
    bad(patch(7, "<H", 128), "128 contexts")
    bad(data[:300], "truncated table")
    bad(patch(9 + 2 * 77, "<H", 0), "frequency of 0")
    bad(patch(9 + 512, "<I", 2 * 32768 + 1), "group 0 claims 65537 words")
    bad(patch(9 + 512 + 8, "<I", 32768 + 1), "group 2 claims 32769 words")     # the short last group: one block
    bad(patch(9 + 512, "<I", 6), "bytes, .* expected")                           # a word count too large
    bad(data[:-4], "bytes, .* expected")                                         # a truncated word list
    bad(data + b"\0", "bytes, .* expected")
    for args, match in (((0, 5, f1, states, words), "group 0 outside"), ((2, 0, f1, states, words), "block count"),
                        ((2, 5, f1[:255], states, words), "256 frequencies"),
                        ((2, 5, np.where(np.arange(256) == 3, 0, f1), states, words), "256 frequencies"),
                        ((2, 5, np.where(np.arange(256) == 3, 65536, f1), states, words), "256 frequencies"),
                        ((2, 5, f1, states[:2], words), "3 groups"), ((2, 5, f1, states, words[:2]), "3 groups"),
                        ((2, 5, f1, states, [words[0], words[1], np.zeros(32769, np.uint32)]), "group 2 holds more words")):
        with pytest.raises(ValueError, match=match):
            lp.write(*args)


def test_status_names_the_fault():
    lp.check_status(np.zeros(4, np.int32))
    with pytest.raises(ValueError, match=r"group 1 is damaged \(a read past the end of its words, words left over\); 2 of 3"):
        lp.check_status(np.asarray([0, 5, 2], np.int32))
    with pytest.raises(ValueError, match="a final state that is not 2\\^31"):
        lp.check_status([2])


def test_lossless_line():
    assert lp.lossless_line(1000, 4000, 7000.0, 64) == "[Lossless] bytes: 1000 bpp: 2.0000 ideal bpp: 1.7500 contexts: 256 group: 64"


def test_parser_flags_default_to_absent_and_refusals_need_no_device(tmp_path):
    import pickle
    import NVFPCC
    ns = NVFPCC.build_parser().parse_args(["decode", "pack.pk"])
    assert not hasattr(ns, "lossless")
    assert NVFPCC.build_parser().parse_args(["encode", "x.ply", "--lossless"]).lossless is True
    ns = NVFPCC.build_parser().parse_args(["decode", "pack.pk", "--lossless", "--lod", "1"])
    with pytest.raises(SystemExit, match="--lossless and --lod"):
        NVFPCC.lossless_refusals(ns, None)
    ns = NVFPCC.build_parser().parse_args(["decode", "pack.pk", "--lossless"])
    with pytest.raises(SystemExit, match="carries no lossless_pack"):
        NVFPCC.lossless_refusals(ns, {"net_weight_pack": {}, "latent_pack": {}})
    NVFPCC.lossless_refusals(ns, {"lossless_pack": b""})
    NVFPCC.lossless_refusals(NVFPCC.build_parser().parse_args(["decode", "pack.pk", "--lod", "1"]), {})
