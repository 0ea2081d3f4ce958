"""The octree of clouds with 11 and 12 bits per axis on the host (nvfpcc_amd/preprocess.py: octree_partition,
octree_level_bytes, the octree_pack of depths 6 and 7) against the 10-bit restatement, which is pinned to the
reference's executable, under translation by whole octants.  Host code only; every comparison is exact."""
import numpy as np
import pytest

from nvfpcc_amd import preprocess as pp
from tests.golden_inputs import synthetic_cloud

OCTANTS = ((1, 0, 0), (0, 1, 0), (1, 1, 1))


@pytest.fixture(scope="module")
def cloud():
    pts = synthetic_cloud()
    return pts, pp.octree_level5(pts), pp.octree_level_bytes(pts)


def test_ten_bits_is_what_it_was(cloud):
    pts, (origins, subtree), levels = cloud
    assert pp.octree_level_bytes(pts, 10) == levels and len(levels) == 6
    o10, s10 = pp.octree_partition(pts, 10)
    assert o10.dtype == origins.dtype and np.array_equal(o10, origins) and s10 == subtree
    assert pp.octree_partition(pts)[1] == subtree
    single = np.array([[1023, 0, 517]])
    assert np.array_equal(pp.octree_partition(single, 10)[0], pp.octree_level5(single)[0])
    assert pp.octree_partition(single, 10)[1] == pp.octree_level5(single)[1]


@pytest.mark.parametrize("octant", OCTANTS)
@pytest.mark.parametrize("bits", (11, 12))
def test_translation_by_an_octant_prepends_one_level_per_bit(cloud, bits, octant):
    pts, (origins, subtree), levels = cloud
    o = np.array(octant)
    child = bytes([1 << (octant[0] + 2 * octant[1] + 4 * octant[2])])
    # 11 bits: octant o of the root.  12 bits: 3072 = 2048 + 1024 is octant o of the root, then octant o again
    shift, extra = ((1024 * o, [child]) if bits == 11 else (3072 * o, [child, child]))
    moved, sub = pp.octree_partition(pts + shift, bits)
    assert np.array_equal(moved, origins + shift)                        # the same leaves in the same order
    got = pp.octree_level_bytes(pts + shift, bits)
    assert len(got) == bits - 4 and got[:len(extra)] == extra and got[len(extra):] == levels
    assert sub == pp.subtree_from_level_bytes(extra + levels)
    assert sub.endswith(subtree) and len(sub) == len(subtree) + 8 * len(extra)


def deep_cloud(bits):
    """A few hundred points in every octant of the volume, its corners among them."""
    rng = np.random.default_rng(bits)
    top = (1 << bits) - 1
    return np.concatenate([rng.integers(0, top + 1, size=(300, 3)), [[0, 0, 0], [top, top, top], [1023, 1024, 1023]]])


@pytest.mark.parametrize("bits", (11, 12))
def test_pack_round_trip(bits):
    depth = bits - 5
    pts = deep_cloud(bits)
    origins, _ = pp.octree_partition(pts, bits)
    assert origins.max() == (1 << bits) - 32 and origins.min() == 0
    levels = pp.octree_level_bytes(pts, bits)
    assert [len(levels[0]), len(levels[depth])] == [1, len(origins)]
    pack = pp.write_octree_pack(levels)
    assert pack[0] == depth and len(pack) == 1 + sum(len(b) for b in levels[:depth])
    assert pack == pp.write_octree_pack(levels[:depth], depth)
    back = pp.read_octree_pack(pack)
    assert back.dtype == np.int64 and np.array_equal(back, origins)
    assert pp.octree_pack_from_origins(origins, bits) == pack
    # the leaves of a partition are a cloud of their own: the same pack from the origins alone, at any row order
    assert pp.octree_pack_from_origins(origins[::-1], bits) == pack


@pytest.mark.parametrize("bits", (11, 12))
def test_malformed_deep_pack_raises(bits):
    depth = bits - 5
    levels = pp.octree_level_bytes(deep_cloud(bits), bits)
    good = pp.write_octree_pack(levels)
    pp.read_octree_pack(good)
    starts = np.cumsum([1] + [len(b) for b in levels[:depth]])          # starts[L] = the first byte of level L
    bad = {"trailing byte": good + b"\x01", "header of another depth": bytes([depth - 1]) + good[1:],
           "header 8": bytes([8]) + good[1:], "header 4": bytes([4]) + good[1:]}
    for cut in list(range(1, 40)) + [int(s) for s in starts[1:depth]] + [len(good) - 1]:
        bad[f"cut at {cut}"] = good[:cut]
    for level in (5, 6)[:depth - 5]:                                    # a childless node in the new levels
        at = int(starts[level])
        bad[f"childless node at level {level}"] = good[:at] + b"\x00" + good[at + 1:]
    for name, data in bad.items():
        with pytest.raises(ValueError, match="octree_pack"):
            pp.read_octree_pack(data)
    with pytest.raises(ValueError):
        pp.write_octree_pack(levels[:depth - 1], depth)
    with pytest.raises(ValueError):
        pp.write_octree_pack(levels + [b"\x01", b"\x01"])


def test_bounds_and_bits_are_checked():
    for bits, bound in ((10, 1024), (11, 2048), (12, 4096)):
        for row in ([0, bound, 5], [-1, 0, 0]):
            for fn in (pp.octree_level_bytes, pp.octree_partition):
                with pytest.raises(ValueError, match=r"\[0, %d\)" % bound):
                    fn(np.array([[1, 2, 3], row]), bits)
        fn(np.array([[bound - 1, 0, bound - 1]]), bits)
    for bits in (9, 13, 10.5, None, True):
        with pytest.raises(ValueError, match="bits"):
            pp.octree_level_bytes(np.array([[1, 2, 3]]), bits)
        with pytest.raises(ValueError, match="bits"):
            pp.octree_pack_from_origins(np.array([[0, 0, 0]]), bits)
        with pytest.raises(ValueError, match="bits"):
            pp.preprocess_device(np.array([[1, 2, 3]]), "cuda", bits=bits)


def test_parser_and_the_checks_that_need_no_device():
    import NVFPCC as cli
    p = cli.build_parser()
    assert not hasattr(p.parse_args(["train", "cloud.ply"]), "bits")           # not given: today's namespace
    a = p.parse_args(["encode", "cloud.ply", "--from_ply", "--bits", "11"])
    assert a.bits == 11 and cli._bits(a) == 11
    assert cli._bits(p.parse_args(["encode", "cloud.ply"])) == 10
    assert cli._bits(p.parse_args(["encode", "cloud.ply", "--bits", "10", "--ref_ply", "ref.ply"])) == 10
    with pytest.raises(SystemExit):
        p.parse_args(["train", "cloud.ply", "--bits", "13"])
    for argv, word in ((["--bits", "11"], "10-bit only"), (["--bits", "12", "--from_ply", "--ref_ply", "r.ply"], "ref_ply"),
                       (["--bits", "11", "--from_ply", "--thh_mode", "d1"], "d1")):
        for command in ("train", "encode"):
            with pytest.raises(SystemExit, match=word):
                cli._bits(p.parse_args([command, "cloud.ply"] + argv))


def test_psnr1_peak_follows_the_bits():
    import NVFPCC as cli
    mse, ten = cli._psnr1(3.0, 1.0)
    assert ten == 20 * np.log10(1023) and cli._psnr1(3.0, 1.0, 1023) == (mse, ten)
    assert cli._psnr1(3.0, 1.0, 4095)[1] == 20 * np.log10(4095)
    sums = np.arange(1.0, 23.0)
    a = cli.test_fields_from_sums(sums, 100, 10.0, 10.0, 1.0, 200)
    b = cli.test_fields_from_sums(sums, 100, 10.0, 10.0, 1.0, 200, peak=2047)
    assert a[:-1] == b[:-1] and np.isclose(b[-1] - a[-1], 20 * np.log10(2047 / 1023), rtol=0, atol=1e-12)
