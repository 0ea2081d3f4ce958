"""A group of frames on the host (nvfpcc_amd/gof.py): frame names, the dataset of several clouds, the gof_pack framing,
the extraction of one frame as a plain pack and the arithmetic of the group's closing lines.  No device."""
import os

import numpy as np
import pytest

from nvfpcc_amd import gof
from nvfpcc_amd.dataloader import LoadedVoxelDataset
from nvfpcc_amd.synth import write_dataset

BLOCKS = (5, 8, 3)


def touch(path):
    with open(path, "wb"):
        pass


# ---------------------------------------------------------------- frame names
def test_frame_names_of_both_conversions(tmp_path):
    for n in (7, 8, 9):
        touch(tmp_path / ("toy_%04d.ply" % n))
        touch(tmp_path / ("raw%d.ply" % n))
    assert gof.frame_names(str(tmp_path / "toy_%04d.ply"), 7, 3) == [str(tmp_path / ("toy_%04d.ply" % n)) for n in (7, 8, 9)]
    assert gof.frame_names(str(tmp_path / "raw%d.ply"), 8, 2) == [str(tmp_path / "raw8.ply"), str(tmp_path / "raw9.ply")]
    assert gof.frame_names(str(tmp_path / "toy_%04d.ply"), 9, 1) == [str(tmp_path / "toy_0009.ply")]


@pytest.mark.parametrize("pattern", ["toy.ply", "toy_%04d_%d.ply", "toy_%04d%%.ply", "toy_%04d_%s.ply", "toy_%.ply", "100%_%d.ply",
                                     "toy_%5d.ply", "toy_%x.ply"])
def test_frame_names_refuses_a_bad_pattern(pattern, tmp_path):
    with pytest.raises(ValueError) as e:
        gof.frame_names(str(tmp_path / pattern), 0, 2)
    assert pattern in str(e.value)


def test_frame_names_refuses_no_frames_and_names_the_first_missing_file(tmp_path):
    pattern = str(tmp_path / "toy_%04d.ply")
    for n in (7, 9):
        touch(pattern % n)
    for count in (0, -1):
        with pytest.raises(ValueError) as e:
            gof.frame_names(pattern, 7, count)
        assert pattern in str(e.value)
    with pytest.raises(ValueError) as e:
        gof.frame_names(pattern, 7, 4)
    assert pattern % 8 in str(e.value) and pattern % 10 not in str(e.value)
    # the files a frame is read from may be others than its name: the first of them that is missing is named
    touch(str(tmp_path / "toy_0007_l5_origins.npy"))
    with pytest.raises(ValueError) as e:
        gof.frame_names(pattern, 7, 1, gof.npy_triple)
    assert str(tmp_path / "toy_0007_l5_gt_grid.npy") in str(e.value)


# ---------------------------------------------------------------- dataset
def load(prefix, shuffle=True):
    return LoadedVoxelDataset(*gof.npy_triple(prefix + ".ply"), shuffle=shuffle)


@pytest.fixture(scope="module")
def triples(tmp_path_factory):
    """Three frames of 5, 8 and 3 blocks, each from its own seed -> (prefixes, [(gt, dist)], [origins])."""
    d = tmp_path_factory.mktemp("gof_cpu")
    prefixes = [str(d / ("f%d" % k)) for k in range(3)]
    arrays = [write_dataset(p, n, base_seed=20221 + 1000 * k) for k, (p, n) in enumerate(zip(prefixes, BLOCKS))]
    return prefixes, arrays, [np.load(p + "_l5_origins.npy") for p in prefixes]


def test_dataset_is_the_frames_one_after_another(triples, capsys):
    prefixes, arrays, origins = triples
    frames = [gof.quiet(load, p) for p in prefixes]
    capsys.readouterr()
    data = gof.GofDataset(frames)
    points = [int(a[0].astype(bool).sum()) for a in arrays]
    assert capsys.readouterr().out == "[data] 16 leaf blocks, %d points\n" % sum(points)
    assert data.N_leaf == len(data) == 16 and int(data.N) == sum(points)
    assert data.frame_ranges.dtype == np.int64 and data.frame_ranges.tolist() == [0, 5, 13, 16]
    assert [int(n) for n in data.frame_points] == points
    assert not np.array_equal(arrays[0][0][:3], arrays[2][0])           # the frames differ
    for name, parts in (("gt_grid", [a[0] for a in arrays]), ("dist", [a[1] for a in arrays]), ("origins", origins)):
        whole = np.concatenate(parts, 0)
        got = getattr(data, name)
        assert got.dtype == whole.dtype and np.array_equal(got, whole), name
    gt, dist = data.to_device("cpu")
    assert gt.shape == (16, 1, 32, 32, 32) and np.array_equal(gt.numpy(), data.gt_grid.astype(np.float32))
    assert np.array_equal(dist.numpy(), data.dist.astype(np.float32))
    for k in range(3):
        v = data.frame(k)
        assert v.N_leaf == len(v) == BLOCKS[k] and int(v.N) == points[k] and v.pre is None
        for name, part in (("gt_grid", arrays[k][0]), ("dist", arrays[k][1]), ("origins", origins[k])):
            got = getattr(v, name)
            assert np.array_equal(got, part), (k, name)
            assert np.shares_memory(got, getattr(data, name)), "frame(k) is a view: no copy"
    for k in (-1, 3):
        with pytest.raises(ValueError):
            data.frame(k)


@pytest.mark.parametrize("shuffle", [False, True])
def test_epoch_order_is_a_permutation_of_all_blocks(triples, shuffle):
    data = gof.quiet(gof.GofDataset, [gof.quiet(load, p, shuffle) for p in triples[0]], shuffle)
    for loader_shuffle in (False, True):
        for epoch in (0, 3):
            order = data.epoch_order(epoch, loader_shuffle, seed=1)
            assert order.dtype == np.int64 and sorted(order.tolist()) == list(range(16))
    if not shuffle:
        assert data.epoch_order(0, False).tolist() == list(range(16))


def test_one_frame_is_the_plain_dataset(triples):
    prefix = triples[0][1]
    for shuffle in (False, True):
        plain = gof.quiet(load, prefix, shuffle)
        data = gof.quiet(gof.GofDataset, [gof.quiet(load, prefix, shuffle)], shuffle)
        assert set(vars(plain)) <= set(vars(data))
        for name, want in vars(plain).items():
            got = getattr(data, name)
            assert type(got) is type(want) and np.array_equal(got, want), name
        assert len(data) == len(plain) and data.MAGIC == plain.MAGIC
        assert [data.permute(i) for i in range(8)] == [plain.permute(i) for i in range(8)]
        for ep in (0, 1):
            assert np.array_equal(data.epoch_order(ep, True, seed=2), plain.epoch_order(ep, True, seed=2))
        for a, b in zip(data.to_device("cpu"), plain.to_device("cpu")):
            assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy())
        for a, b in zip(data[3], plain[3]):
            assert np.array_equal(a.numpy(), b.numpy())
        assert data.frame_ranges.tolist() == [0, 8] and np.array_equal(data.frame(0).gt_grid, plain.gt_grid)


# ---------------------------------------------------------------- framing
@pytest.mark.parametrize("F", [1, 3])
def test_gof_pack_round_trip(F):
    leaves, points = [917, 8, 4000000000][:F], [850123, 7411, 4294967295][:F]
    data = gof.write_gof_pack(1300, leaves, points)
    assert isinstance(data, bytes) and len(data) == 7 + 8 * F
    assert data[0] == 1 and data[1:3] == F.to_bytes(2, "little") and data[3:7] == (1300).to_bytes(4, "little")
    assert data[7:15] == leaves[0].to_bytes(4, "little") + points[0].to_bytes(4, "little")
    assert gof.read_gof_pack(data) == {"start": 1300, "n_leaf": leaves, "n_points": points}


def test_gof_pack_refusals():
    good = gof.write_gof_pack(7, [8, 8, 8], [100, 200, 300])
    for bad, word in ((bytes([2]) + good[1:], "version"), (good[:-1], "bytes"), (good + b"\0", "bytes"), (good[:5], "bytes"),
                      (b"", "bytes"), (bytes([1, 0, 0]) + good[3:7], "0 frames")):
        with pytest.raises(ValueError) as e:
            gof.read_gof_pack(bad)
        assert "gof_pack" in str(e.value) and word in str(e.value), (bad, str(e.value))
    with pytest.raises(ValueError):
        gof.write_gof_pack(0, [], [])
    with pytest.raises(ValueError):
        gof.write_gof_pack(0, [1, 2], [3])


# ---------------------------------------------------------------- extraction and accounting
def hand_made_pack():
    W = {"bit_stream": bytes(1000), "keys_quantize": ["k"]}
    frames = []
    for k, (n, lat, side) in enumerate(((8, 50, 11), (8, 61, 0), (3, 40, 7))):
        f = {"origins": np.zeros((n, 3), np.int16), "latent_pack": {"latent_byte_stream": bytes(lat)}}
        if side:
            f["thh_pack"] = bytes(5)
            f["lossless_pack"] = bytes(side - 5)
        frames.append(f)
    return {"net_weight_pack": W, "gof_pack": gof.write_gof_pack(7, [8, 8, 3], [1000, 2000, 500]), "frames": frames}


def test_extract_is_a_plain_pack_of_one_frame():
    pack = hand_made_pack()
    for k in range(3):
        one = gof.extract(pack, k)
        assert list(one) == ["net_weight_pack"] + list(pack["frames"][k])
        assert one["net_weight_pack"] is pack["net_weight_pack"]
        assert all(one[key] is pack["frames"][k][key] for key in pack["frames"][k])
    assert list(gof.extract(pack, 0)) == ["net_weight_pack", "origins", "latent_pack", "thh_pack", "lossless_pack"]
    for k in (-1, 3, 70000):
        with pytest.raises(ValueError) as e:
            gof.extract(pack, k)
        assert str(k) in str(e.value)
    pack["frames"][1]["origins"] = np.zeros((7, 3), np.int16)
    with pytest.raises(ValueError) as e:
        gof.extract(pack, 1)
    assert "7 leaf blocks" in str(e.value) and "8" in str(e.value)
    assert list(gof.extract(pack, 2)) == ["net_weight_pack", "origins", "latent_pack", "thh_pack", "lossless_pack"]    # the others still come out
    with pytest.raises(ValueError):
        gof.extract(dict(pack, frames=pack["frames"][:2]), 0)


def test_extract_counts_the_leaves_of_an_octree_pack():
    from nvfpcc_amd.preprocess import octree_pack_from_origins
    from nvfpcc_amd.synth import make_origins
    pack = hand_made_pack()
    f = pack["frames"][2]
    pack["frames"][2] = {"latent_pack": f["latent_pack"], "octree_pack": octree_pack_from_origins(make_origins(3).astype(np.int16))}
    assert list(gof.extract(pack, 2)) == ["net_weight_pack", "latent_pack", "octree_pack"]
    pack["frames"][2]["octree_pack"] = octree_pack_from_origins(make_origins(4).astype(np.int16))
    with pytest.raises(ValueError):
        gof.extract(pack, 2)


def test_group_lines_arithmetic():
    pack = hand_made_pack()
    a = gof.account(pack)
    g = len(pack["gof_pack"])
    assert g == 7 + 8 * 3
    assert (a["frames"], a["points"], a["weight_bits"], a["latent_bits"], a["side_bits"], a["gof_bits"]) == (
        3, 3500, 8000, 8 * 151, 8 * 18, 8 * g)
    assert a["gross_bpp"] == (8000 + 8 * 151 + 8 * 18 + 8 * g) / 3500.0
    assert a["own_bpp"] == [8 * 61 / 1000.0, 8 * 61 / 2000.0, 8 * 47 / 500.0]
    # the frames' own bpp, weighted by their points, are the total without the weights and the framing
    own = sum(b * n for b, n in zip(a["own_bpp"], (1000, 2000, 500)))
    assert abs(own - (a["gross_bpp"] * 3500 - 8000 - 8 * g)) < 1e-9
    assert gof.gof_lines(pack) == ["[GoF] frames: 3 points: 3500 weight bytes: 1000 latent bytes: 151 side bytes: 18",
                                   "[Latent code] Gross bpp: %.4f" % a["gross_bpp"]]
    assert gof.frame_line(9, 500, 3, 8 * 40, 8 * 7) == (
        "[Frame 0009] points: 500 blocks: 3 latent bytes: 40 side bytes: 7 own bpp: 0.7520")
