"""Scalable lossless geometry through the command line: train a few epochs on the tiny synthetic cloud, encode with and
without --lossless_lod, decode at its three levels, and next to the other side packs.  One training run serves every
test."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_lod_cli import CLI, COMMON, N_BLOCKS, ROOT, gross_bpp, read, run, same

pytestmark = pytest.mark.gpu
OTHERS = ["--lossless", "--thh_mode", "count", "--pack_lod", "--lod_heads", "ckpts/0010.ckpt"]


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """train -> quantise -> encode (plain) -> encode --lossless_lod -> encode with the other side packs, without and
    with --lossless_lod, in one directory; the encoders' outputs kept aside."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    from tests.golden_inputs import write_cloud_ply
    cwd = str(tmp_path_factory.mktemp("lossless_lod_cli"))
    gts, _ = write_dataset(os.path.join(cwd, "toy"), N_BLOCKS)
    nz = np.argwhere(gts.reshape(N_BLOCKS, 32, 32, 32))
    cloud = nz[:, 1:] + make_origins(N_BLOCKS).astype(np.int64)[nz[:, 0]]      # the input's voxels, (block, raster) order
    write_cloud_ply(os.path.join(cwd, "cloud.ply"), cloud)
    run([CLI, "train", "toy.ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = [CLI, "encode", "toy.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt",
           "--thh", "0.5"] + COMMON
    out_plain = run(enc + ["--pack_fn", "plain.pk"], cwd)
    os.replace(os.path.join(cwd, "rc_enc.ply"), os.path.join(cwd, "rc_enc_plain.ply"))
    out_ll = run(enc + ["--pack_fn", "lod.pk", "--lossless_lod"], cwd)
    os.replace(os.path.join(cwd, "rc_enc.ply"), os.path.join(cwd, "rc_enc_lod.ply"))
    out_others = run(enc + ["--pack_fn", "others.pk"] + OTHERS, cwd)
    out_all = run(enc + ["--pack_fn", "all.pk", "--lossless_lod"] + OTHERS, cwd)
    return {"cwd": cwd, "cloud": cloud, "out_plain": out_plain, "out_ll": out_ll, "out_others": out_others, "out_all": out_all}


def load(cwd, name):
    with open(os.path.join(cwd, name), "rb") as f:
        return pickle.load(f)


def rows(a):
    """The set of points, in one order."""
    return np.unique(np.asarray(a, np.int64).reshape(-1, 3), axis=0)


def test_lossless_lod_adds_one_key_and_its_bits_and_changes_nothing_else(coded):
    from nvfpcc_amd import lossless_lod_pack as lp
    cwd, n_points = coded["cwd"], coded["cloud"].shape[0]
    plain, ll = load(cwd, "plain.pk"), load(cwd, "lod.pk")
    assert list(plain) == ['net_weight_pack', 'origins', 'latent_pack']
    assert list(ll) == list(plain) + ['lossless_lod_pack'] and isinstance(ll['lossless_lod_pack'], bytes)
    side = ll.pop('lossless_lod_pack')
    assert same(plain, ll), "the packs differ beyond the lossless_lod_pack key"
    info = lp.read(side, N_BLOCKS)
    n_used = int(info["used"].sum())
    assert info["group"] == 64 and len(side) == lp.size(N_BLOCKS, 64, int(info["nwords"].sum()), n_used)
    # Gross bpp is printed with four decimals: the two printed values are each within 5e-5 of the exact ones
    rise = gross_bpp(coded["out_ll"]) - gross_bpp(coded["out_plain"])
    assert abs(rise - 8 * len(side) / n_points) <= 1.0001e-4, (rise, 8 * len(side) / n_points)
    # the lossy outputs of the encoder are the same with and without the flag, and one line is new
    assert np.array_equal(read(cwd, "rc_enc_lod.ply"), read(cwd, "rc_enc_plain.ply"))
    strip = lambda s: [ln for ln in s.splitlines() if ln.startswith("[") and not ln.startswith("[LosslessLoD]") and "Gross bpp" not in ln]
    assert strip(coded["out_ll"]) == strip(coded["out_plain"]) and "[Lossless" not in coded["out_plain"]
    m = re.search(r"^\[LosslessLoD\] bytes: (\d+) bpp: ([0-9.]+) ideal bpp: ([0-9.]+) contexts: (\d+) symbols: (\d+) group: 64$",
                  coded["out_ll"], re.M)
    assert m, coded["out_ll"][-2000:]
    assert int(m.group(1)) == len(side) and abs(float(m.group(2)) - 8 * len(side) / n_points) <= 5.0001e-5
    assert int(m.group(4)) == n_used and N_BLOCKS * 512 < int(m.group(5)) < N_BLOCKS * 32768
    # the coder's bound: the headers and the table, 4096 bits of states per group, log2(1 + 2^-15) per coded symbol
    over = 8 * len(side) - float(m.group(3)) * n_points
    assert -0.5e-4 * n_points <= over <= 8 * (9 + 384 + 2 * n_used + 4) + 4096 + int(m.group(5)) * np.log2(1 + 2.0 ** -15) + 0.5e-4 * n_points
    # with the other side packs: the same bytes, after them; their keys and bytes as without the flag
    others, every = load(cwd, "others.pk"), load(cwd, "all.pk")
    assert list(every) == list(others) + ['lossless_lod_pack'] == ['net_weight_pack', 'origins', 'latent_pack', 'thh_pack',
                                                                  'lod_pack', 'lossless_pack', 'lossless_lod_pack']
    assert every.pop('lossless_lod_pack') == side and same(others, every)
    rise = gross_bpp(coded["out_all"]) - gross_bpp(coded["out_others"])
    assert abs(rise - 8 * len(side) / n_points) <= 1.0001e-4
    assert m.group(0) in coded["out_all"] and "[Lossless] bytes:" in coded["out_all"] and "[LoD 1]" in coded["out_all"]


@pytest.mark.parametrize("level", [0, 1, 2])
def test_decode_lossless_lod_writes_exactly_the_input_at_the_level(coded, level):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "all.pk" if level == 1 else "lod.pk", "--batchsize", "7" if level == 1 else "1", "--N",
               str(N_BLOCKS), "--lossless_lod", str(level), "--ref_ply", "cloud.ply"] + COMMON, cwd)
    dec = read(cwd, "rc_dec.ply")
    want = rows(coded["cloud"] >> level)
    assert dec.shape == want.shape and np.array_equal(rows(dec), want)           # no point twice, none missing, none added
    if level == 0:
        assert np.array_equal(dec, coded["cloud"])                               # in (block, raster) order
    assert "[LosslessLoD] level: %d points: %d" % (level, len(dec)) in out
    assert re.search(r"^\[PCError\] D1 PSNR: inf D2 PSNR: \S+$", out, re.M), out[-2000:]


@pytest.mark.parametrize("flags", [["--thh", "0.5"], ["--lossless"], ["--lod", "1"], ["--lod", "2"]], ids=" ".join)
def test_the_other_decodes_ignore_lossless_lod_pack(coded, flags):
    """A plain decode, decode --lossless and decode --lod of a pack that carries every side pack: the same output and
    the same cloud as from the pack without lossless_lod_pack."""
    cwd = coded["cwd"]
    args = flags + ["--batchsize", "1", "--N", str(N_BLOCKS)] + COMMON
    out_a = run([CLI, "decode", "others.pk"] + args, cwd)
    a = read(cwd, "rc_dec.ply")
    out_b = run([CLI, "decode", "all.pk"] + args, cwd)
    b = read(cwd, "rc_dec.ply")
    assert a.shape[0] > 0 and np.array_equal(a, b)
    assert out_a == out_b and "[LosslessLoD" not in out_a
    if flags == ["--lossless"]:
        assert np.array_equal(a, coded["cloud"])


REFUSALS = {
    "no side pack": ("others.pk", ["--lossless_lod", "1"], "decode --lossless_lod 1: others.pk carries no lossless_lod_pack"),
    "with --lod": ("all.pk", ["--lossless_lod", "1", "--lod", "1"], "--lossless_lod and --lod exclude each other"),
    "with --lossless": ("all.pk", ["--lossless_lod", "0", "--lossless"], "--lossless_lod and --lossless exclude each other"),
    "--lossless --lod still": ("all.pk", ["--lossless", "--lod", "1"], "--lossless and --lod exclude each other"),
    # a pack whose stream is damaged: level 0 says so; and one that codes another number of blocks
    "damaged stream": ("damaged.pk", ["--lossless_lod", "0"],
                       "decode --lossless_lod 0: lossless_lod_pack: the stream of group 0 is damaged"),
    "another block count": ("lod.pk", ["--lossless_lod", "2", "--N", str(N_BLOCKS - 1)],
                            "codes %d blocks, the pack holds %d" % (N_BLOCKS, N_BLOCKS - 1)),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_exit_with_their_message(coded, case):
    cwd = coded["cwd"]
    name, flags, message = REFUSALS[case]
    if name == "damaged.pk":
        pack = load(cwd, "lod.pk")
        side = bytearray(pack["lossless_lod_pack"])
        side[-2] ^= 0x40
        with open(os.path.join(cwd, name), "wb") as f:
            pickle.dump(dict(pack, lossless_lod_pack=bytes(side)), f)
    out = run([CLI, "decode", name, "--batchsize", "1", "--N", str(N_BLOCKS)] + flags + COMMON, cwd, ok=False)
    assert message in out and "Traceback" not in out
