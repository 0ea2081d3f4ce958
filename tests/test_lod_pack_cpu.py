"""Host side of the level-of-detail decode: the `lod_pack` entry of pack.pk (nvfpcc_amd/lod_pack.py), the new
command-line flags, and the reduction of a reference cloud to a coarser lattice (recon.reduce_to_lattice)."""
import struct
import sys

import numpy as np
import pytest
import torch

from nvfpcc_amd import lod_pack as lp
from nvfpcc_amd.recon import reduce_to_lattice


def heads(chanstr, seed=5):
    """Four float16-representable tensors shaped like the coarse heads of a decoder with this channel string."""
    c1, c2 = lp.head_channels(chanstr)
    g = torch.Generator().manual_seed(seed)
    raw = [0.3 * torch.randn(1, c1, 3, 3, 3, generator=g), torch.randn(1, generator=g),
           0.3 * torch.randn(1, c2, 3, 3, 3, generator=g), torch.randn(1, generator=g)]
    return [lp.round_f16(t) for t in raw], raw


@pytest.mark.parametrize("chanstr", ["8,16,8,8", "16,32,16,16"])
def test_round_trip(chanstr):
    (k1, b1, k2, b2), _ = heads(chanstr)
    t1, t2 = float(np.float32(0.4375123)), float(np.float32(0.91))
    data = lp.write_lod_pack(t1, t2, k1, b1, k2, b2)
    c1, c2 = lp.head_channels(chanstr)
    assert isinstance(data, bytes) and len(data) == 13 + 2 * (27 * c1 + 1 + 27 * c2 + 1) and data[0] == lp.VERSION
    back = lp.read_lod_pack(data, chanstr)
    assert back["t"] == (t1, t2) and back["channels"] == (c1, c2)
    assert list(back["state"]) == list(lp.HEAD_KEYS)
    for k, ref in zip(lp.HEAD_KEYS, (k1, b1, k2, b2)):
        got = back["state"][k]
        assert got.dtype == torch.float32 and got.shape == ref.shape and torch.equal(got, ref), k
    assert lp.read_lod_pack(data)["t"] == (t1, t2)                    # no channel string: nothing to compare with
    assert lp.write_lod_pack(*back["t"], *[back["state"][k] for k in lp.HEAD_KEYS]) == data


def test_head_channels_follow_the_channel_string():
    assert lp.head_channels("8,16,8,8") == (8, 16) and lp.head_channels((16, 32, 16, 16)) == (16, 32)
    with pytest.raises(ValueError):
        lp.head_channels("8,16,8")


def test_float16_rounding_is_idempotent_and_what_the_pack_stores():
    (k1, b1, k2, b2), raw = heads("8,16,8,8")
    assert not torch.equal(raw[0], k1)                                 # the rounding does something ...
    assert torch.equal(lp.round_f16(k1), k1)                           # ... once
    assert torch.equal(k1, raw[0].half().float())
    # unrounded tensors in: the pack holds their float16 values, i.e. what an encoder that rounded first evaluates with
    a = lp.write_lod_pack(0.5, 0.5, *raw)
    assert a == lp.write_lod_pack(0.5, 0.5, k1, b1, k2, b2)
    with pytest.raises(ValueError):
        lp.round_f16(torch.tensor([1e6]))                              # not finite in float16


def test_round_heads_rounds_the_live_parameters_in_place():
    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.reconstructor = torch.nn.Module()
            for h, c in (("conv1_cls", 8), ("conv0_cls", 16)):
                m = torch.nn.Module()
                m.kernel = torch.nn.Parameter(0.1 * torch.randn(1, c, 3, 3, 3, generator=torch.Generator().manual_seed(c)))
                m.b = torch.nn.Parameter(torch.tensor([0.123456789]))
                setattr(self.reconstructor, h, m)
    net = Toy()
    before = net.reconstructor.conv1_cls.kernel.detach().clone()
    rounded = lp.round_heads_(net)
    assert list(rounded) == list(lp.HEAD_KEYS)
    assert torch.equal(net.reconstructor.conv1_cls.kernel.detach(), before.half().float())
    assert torch.equal(net.reconstructor.conv0_cls.b.detach(), rounded["reconstructor.conv0_cls.b"])
    with pytest.raises(KeyError, match="conv1_cls.kernel"):
        lp.head_tensors({})


def test_malformed_packs_raise():
    (k1, b1, k2, b2), _ = heads("8,16,8,8")
    good = lp.write_lod_pack(0.5, 0.6, k1, b1, k2, b2)
    bad = {
        "empty": b"",
        "version": bytes([lp.VERSION + 1]) + good[1:],
        "header cut": good[:7],
        "payload cut": good[:-2],
        "odd byte cut": good[:-1],
        "trailing bytes": good + b"\0\0",
        "zero channels": struct.pack("<BffHH", lp.VERSION, 0.5, 0.6, 0, 16) + good[13:],
        "nan threshold": struct.pack("<BffHH", lp.VERSION, float("nan"), 0.6, 8, 16) + good[13:],
        "inf weight": good[:13] + struct.pack("<e", float("inf")) + good[15:],
    }
    for what, data in bad.items():
        with pytest.raises(ValueError, match="lod_pack"):
            lp.read_lod_pack(data)
            pytest.fail(what)
    with pytest.raises(ValueError, match="chanstr"):
        lp.read_lod_pack(good, "16,32,16,16")                          # the other decoder's heads
    with pytest.raises(ValueError, match="chanstr"):
        lp.read_lod_pack(good, "8,16,16,8")
    with pytest.raises(ValueError):
        lp.write_lod_pack(0.5, 0.6, k1.reshape(-1), b1, k2, b2)         # not a head's kernel
    with pytest.raises(ValueError):
        lp.write_lod_pack(float("inf"), 0.6, k1, b1, k2, b2)


def test_lod_line():
    assert lp.lod_line(1, 0.25, 12) == "[LoD 1] t: 0.25 points: 12"
    assert lp.lod_line(2, np.float32(0.1), 3, 0.5, 1.0) == "[LoD 2] t: 0.100000001 points: 3 Pacc: 0.5000 Nacc: 1.0000"


def _cli():
    sys_argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        import NVFPCC as cli
    finally:
        sys.argv = sys_argv
    return cli


def test_parser_namespace_changes_only_with_the_new_flags():
    cli = _cli()
    today = {"command", "input", "checkpoint_dir", "batchsize", "lmbda", "load_weights", "load_extern", "lr", "alpha",
             "use_coords", "real", "dsep", "stat_latent", "stat_net", "w1", "w2", "notes", "load_meta", "shuffle",
             "phase_change", "wemb", "ch", "load_emb", "chanstr", "thh", "pack_fn", "N", "qp", "device", "epochs", "seed",
             "ref_ply", "thh_mode"}
    for cmd in (["encode", "x.ply"], ["decode", "pack.pk"]):
        assert set(vars(cli.build_parser().parse_args(cmd))) == today
    a = cli.build_parser().parse_args(["encode", "x.ply", "--pack_lod"])
    assert set(vars(a)) == today | {"pack_lod"} and a.pack_lod is True
    a = cli.build_parser().parse_args(["encode", "x.ply", "--pack_lod", "--lod_heads", "ckpts/0500.ckpt"])
    assert set(vars(a)) == today | {"pack_lod", "lod_heads"} and a.lod_heads == "ckpts/0500.ckpt"
    for level in (1, 2):
        a = cli.build_parser().parse_args(["decode", "pack.pk", "--lod", str(level)])
        assert set(vars(a)) == today | {"lod"} and a.lod == level
    for bad in ("0", "3", "x"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["decode", "pack.pk", "--lod", bad])


@pytest.mark.parametrize("lod", [1, 2])
def test_lattice_reduction_matches_numpy(lod):
    rng = np.random.default_rng(11 + lod)
    base = rng.integers(0, 4096 >> lod, size=(400, 3))
    # every coarse voxel several times over, at different fine positions: collisions by construction
    fine = np.concatenate([(base << lod) + rng.integers(0, 1 << lod, size=base.shape) for _ in range(3)])
    fine = np.concatenate([fine, [[4095, 4095, 4095], [4095, 4095, 4094], [0, 0, 0], [1, 0, 1]]])
    got = reduce_to_lattice(fine.astype(np.float64), lod)              # the PLY reader hands out doubles
    ref = np.unique(fine >> lod, axis=0)
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert got.shape[0] < fine.shape[0] and got.max() == 4095 >> lod
    assert np.array_equal(reduce_to_lattice(got, 0), got)
    assert len({tuple(r) for r in got.tolist()}) == got.shape[0]
    with pytest.raises(ValueError):
        reduce_to_lattice(np.array([[0, -1, 0]]), lod)
    with pytest.raises(ValueError):
        reduce_to_lattice(np.zeros((3, 4)), lod)
