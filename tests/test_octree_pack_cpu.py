"""The octree as bytes (nvfpcc_amd/preprocess.py): per-level child-occupancy bytes, the `octree_pack` entry of pack.pk
that replaces the raw leaf origins, and the command-line flags that switch the device pre-processing on.  Host code
only; every comparison is exact."""
import hashlib
import os
import pickle

import numpy as np
import pytest

from nvfpcc_amd import preprocess as pp
from tests.golden_inputs import synthetic_cloud


def scattered_cloud():
    rng = np.random.default_rng(5)
    return np.unique(rng.integers(0, 1024, size=(3000, 3)), axis=0)


def duplicated_cloud():
    pts = synthetic_cloud()
    return np.concatenate([pts[::-1], pts[:1000], pts[5:6].repeat(7, 0)])


CLOUDS = {
    "synthetic": synthetic_cloud,
    "scattered": scattered_cloud,
    "single": lambda: np.array([[1023, 0, 517]], np.int64),
    "duplicates": duplicated_cloud,
}
# occupancy bytes of levels 0..4 (the pack is one header byte longer) against 6 bytes per leaf of raw int16 origins
PAYLOAD = {"synthetic": (53, 576), "scattered": (2729, 17304), "single": (5, 6)}


@pytest.mark.parametrize("name", list(CLOUDS))
def test_octree_pack_round_trip(name):
    pts = CLOUDS[name]()
    origins, subtree = pp.octree_level5(pts)
    levels = pp.octree_level_bytes(pts)
    assert len(levels) == 6 and [len(b) for b in levels][0] == 1 and len(levels[5]) == len(origins)
    assert pp.subtree_from_level_bytes(levels) == subtree
    pack = pp.write_octree_pack(levels)
    assert isinstance(pack, bytes) and len(pack) == 1 + sum(len(b) for b in levels[:5])
    back = pp.read_octree_pack(pack)
    assert back.dtype == np.int64 and np.array_equal(back, origins)          # same cubes, same traversal order
    assert pp.octree_pack_from_origins(origins) == pack                      # what the file-based encoder builds
    if name in PAYLOAD:
        assert (len(pack) - 1, 6 * len(origins)) == PAYLOAD[name]


def test_level_bytes_expand_to_the_golden_subtree(golden_dir):
    G = np.load(os.path.join(golden_dir, "octree.npz"))
    pts = synthetic_cloud()
    assert hashlib.sha256(pts.tobytes()).digest() == G["points_sha"].tobytes()
    levels = pp.octree_level_bytes(pts)
    s = pp.subtree_from_level_bytes(levels)
    assert len(s) == int(G["subtree_len"]) and hashlib.sha256(s.encode()).digest() == G["subtree_sha"].tobytes()
    assert np.array_equal(pp.read_octree_pack(pp.write_octree_pack(levels)), G["origins"])


def test_malformed_octree_pack_raises():
    good = pp.write_octree_pack(pp.octree_level_bytes(synthetic_cloud()))
    pp.read_octree_pack(good)
    bad = {
        "empty": b"",
        "header only": good[:1],
        "unknown header": bytes([9]) + good[1:],
        "trailing byte": good + b"\x01",
        "all children everywhere": bytes([5]) + b"\xff" * 64,     # asks for 1 + 8 + 64 + ... nodes, holds 64
        "node without children": good[:3] + b"\x00" + good[4:],
    }
    for cut in range(1, len(good)):
        bad[f"cut at {cut}"] = good[:cut]
    for data in bad.values():
        with pytest.raises(ValueError, match="octree_pack"):
            pp.read_octree_pack(data)
    with pytest.raises(ValueError):
        pp.write_octree_pack([b"\x01"] * 3)
    # the largest legal tree: every node of levels 0..4 full -> all 32768 leaves, still in Morton order
    full = pp.read_octree_pack(bytes([5]) + b"\xff" * (1 + 8 + 64 + 512 + 4096))
    assert full.shape == (32768, 3) and np.array_equal(full[:3], [[0, 0, 0], [32, 0, 0], [0, 32, 0]])
    assert np.array_equal(full[-1], [992, 992, 992])


def test_level_bytes_refuse_bad_clouds():
    with pytest.raises(ValueError):
        pp.octree_level_bytes(np.zeros((0, 3), np.int64))
    for p in ([[0, 0, 1024]], [[-1, 5, 5]]):
        with pytest.raises(ValueError):
            pp.octree_level_bytes(np.array(p))


def test_parser_knows_the_new_flags():
    import NVFPCC as cli
    p = cli.build_parser()
    a = p.parse_args(["encode", "cloud.ply", "--from_ply", "--pack_octree"])
    assert a.from_ply is True and a.pack_octree is True
    a = p.parse_args(["train", "cloud.ply"])                   # not given: today's namespace, nothing added
    assert not hasattr(a, "from_ply") and not hasattr(a, "pack_octree")


def test_decode_of_a_pack_without_octree_pack_takes_the_old_route(tmp_path, monkeypatch):
    """decode() asks the pack for `octree_pack` first; a pack without it reads `origins` and --N as before.  The net and
    the device are stubbed out: only the choice of the leaves is under test."""
    import torch
    import NVFPCC as cli
    from nvfpcc_amd import latent_codec, recon, weight_codec
    origins = (np.arange(12).reshape(4, 3) * 32).astype(np.int16)
    tree_origins, _ = pp.octree_level5(synthetic_cloud())
    seen = {}

    class Net:
        def load_state_dict(self, *a, **k): pass
        def to(self, dev): return self

    def fake_reconstruct(net, latents, org, thh, **kw):
        seen["origins"], seen["n"] = np.asarray(org), latents.shape[0]
        return np.zeros((0, 3), np.int32), None

    monkeypatch.setattr(cli, "_device", lambda args: (torch.device("cpu"), 0, 1))
    monkeypatch.setattr(cli, "_build_net", lambda args, dev: Net())
    monkeypatch.setattr(weight_codec, "entropy_decode", lambda *a: [])
    monkeypatch.setattr(latent_codec, "arithmetic_dec", lambda lp: torch.zeros(200, 3, 2, 2, 2))
    monkeypatch.setattr(recon, "reconstruct_points", fake_reconstruct)
    monkeypatch.setattr(recon, "write_ply_ascii", lambda fn, pts: None)
    wp = dict(bit_stream=b"", inv_codebook={}, element_length=0, shape_list=[], keys_quantize=[], keys_code_as_is=[],
              as_is_pool=[])
    old = {"net_weight_pack": wp, "origins": origins, "latent_pack": {}}
    new = {"net_weight_pack": wp, "latent_pack": {}, "octree_pack": pp.octree_pack_from_origins(tree_origins)}
    for name, pack in (("old.pk", old), ("new.pk", new)):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(pack, f)
    parse = lambda fn, *more: cli.build_parser().parse_args(["decode", str(tmp_path / fn), *more])
    cli.decode(parse("old.pk", "--N", "3"))
    assert seen["n"] == 3 and np.array_equal(seen["origins"], origins[:3])
    cli.decode(parse("new.pk", "--N", "3"))                                   # --N is not consulted
    assert seen["n"] == len(tree_origins) and np.array_equal(seen["origins"], tree_origins)
    assert seen["origins"].dtype == np.int16
