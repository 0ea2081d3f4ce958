"""Lossless geometry through the command line: train a few epochs on the tiny synthetic cloud, encode with and without
--lossless, decode with and without it.  One training run serves every test."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_lod_cli import CLI, COMMON, N_BLOCKS, ROOT, gross_bpp, read, run, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """train -> quantise -> encode (plain) -> encode --lossless, in one directory; the encoders' outputs kept aside."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    from tests.golden_inputs import write_cloud_ply
    cwd = str(tmp_path_factory.mktemp("lossless_cli"))
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
    out_ll = run(enc + ["--pack_fn", "lossless.pk", "--lossless"], cwd)
    return {"cwd": cwd, "cloud": cloud, "out_plain": out_plain, "out_ll": out_ll, "enc": enc}


def test_lossless_adds_one_key_and_its_bits_and_changes_nothing_else(coded):
    from nvfpcc_amd import lossless_pack as lp
    cwd, n_points = coded["cwd"], coded["cloud"].shape[0]
    with open(os.path.join(cwd, "plain.pk"), "rb") as f:
        plain = pickle.load(f)
    with open(os.path.join(cwd, "lossless.pk"), "rb") as f:
        ll = pickle.load(f)
    assert list(plain) == ['net_weight_pack', 'origins', 'latent_pack']
    assert list(ll) == list(plain) + ['lossless_pack'] and isinstance(ll['lossless_pack'], bytes)
    side = ll.pop('lossless_pack')
    assert same(plain, ll), "the packs differ beyond the lossless_pack key"
    info = lp.read(side, N_BLOCKS)
    assert info["group"] == 64 and len(side) == lp.size(N_BLOCKS, 64, int(info["nwords"].sum()))
    # Gross bpp is printed with four decimals: the two printed values are each within 5e-5 of the exact ones
    rise = gross_bpp(coded["out_ll"]) - gross_bpp(coded["out_plain"])
    assert abs(rise - 8 * len(side) / n_points) <= 1.0001e-4, (rise, 8 * len(side) / n_points)
    # the lossy outputs of the encoder are the same with and without the flag, and one line is new
    assert np.array_equal(read(cwd, "rc_enc.ply"), read(cwd, "rc_enc_plain.ply"))
    strip = lambda s: [ln for ln in s.splitlines() if ln.startswith("[") and not ln.startswith("[Lossless") and "Gross bpp" not in ln]
    assert strip(coded["out_ll"]) == strip(coded["out_plain"]) and "[Lossless" not in coded["out_plain"]
    m = re.search(r"^\[Lossless\] bytes: (\d+) bpp: ([0-9.]+) ideal bpp: ([0-9.]+) contexts: 256 group: 64$", coded["out_ll"], re.M)
    assert m, coded["out_ll"][-2000:]
    assert int(m.group(1)) == len(side) and abs(float(m.group(2)) - 8 * len(side) / n_points) <= 5.0001e-5
    # the coder's bound: the table and the headers, 4096 bits of states per group, log2(1 + 2^-15) per symbol
    over = 8 * len(side) - float(m.group(3)) * n_points
    assert -0.5e-4 * n_points <= over <= 8 * (9 + 512 + 4) + 4096 + N_BLOCKS * 32768 * np.log2(1 + 2.0 ** -15) + 0.5e-4 * n_points


def test_decode_lossless_writes_exactly_the_input(coded):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "lossless.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lossless", "--ref_ply",
               "cloud.ply"] + COMMON, cwd)
    dec = read(cwd, "rc_dec.ply")
    assert dec.shape == coded["cloud"].shape and np.array_equal(dec, coded["cloud"])      # the set, in (block, raster) order
    assert "[Lossless] points: %d" % len(dec) in out
    assert re.search(r"^\[PCError\] D1 PSNR: inf D2 PSNR: inf$", out, re.M), out[-2000:]


def test_plain_decode_ignores_lossless_pack(coded):
    cwd = coded["cwd"]
    args = ["--batchsize", "1", "--thh", "0.5", "--N", str(N_BLOCKS)] + COMMON
    out_a = run([CLI, "decode", "plain.pk"] + args, cwd)
    a = read(cwd, "rc_dec.ply")
    out_b = run([CLI, "decode", "lossless.pk"] + args, cwd)
    b = read(cwd, "rc_dec.ply")
    assert a.shape[0] > 0 and np.array_equal(a, b) and np.array_equal(a, read(cwd, "rc_enc_plain.ply"))
    assert out_a == out_b and "[Lossless" not in out_a


def test_refusals_exit_with_their_message(coded):
    cwd = coded["cwd"]
    base = ["--batchsize", "1", "--N", str(N_BLOCKS)] + COMMON
    out = run([CLI, "decode", "plain.pk", "--lossless"] + base, cwd, ok=False)
    assert "carries no lossless_pack" in out and "--lossless" in out and "Traceback" not in out
    out = run([CLI, "decode", "lossless.pk", "--lossless", "--lod", "1"] + base, cwd, ok=False)
    assert "--lossless and --lod exclude each other" in out and "Traceback" not in out
    # a pack whose stream is damaged, and one that codes another number of blocks
    with open(os.path.join(cwd, "lossless.pk"), "rb") as f:
        pack = pickle.load(f)
    side = bytearray(pack["lossless_pack"])
    side[-2] ^= 0x40
    with open(os.path.join(cwd, "damaged.pk"), "wb") as f:
        pickle.dump(dict(pack, lossless_pack=bytes(side)), f)
    out = run([CLI, "decode", "damaged.pk", "--lossless"] + base, cwd, ok=False)
    assert "decode --lossless: lossless_pack: the stream of group 0 is damaged" in out and "Traceback" not in out
    out = run([CLI, "decode", "lossless.pk", "--lossless", "--batchsize", "1", "--N", str(N_BLOCKS - 1)] + COMMON, cwd, ok=False)
    assert "codes %d blocks, the pack holds %d" % (N_BLOCKS, N_BLOCKS - 1) in out and "Traceback" not in out


def test_lossless_combines_with_the_other_side_packs(coded):
    cwd = coded["cwd"]
    out = run(coded["enc"] + ["--pack_fn", "all.pk", "--lossless", "--thh_mode", "count", "--pack_lod", "--lod_heads",
                              "ckpts/0010.ckpt"], cwd)
    with open(os.path.join(cwd, "all.pk"), "rb") as f:
        pack = pickle.load(f)
    with open(os.path.join(cwd, "lossless.pk"), "rb") as f:
        alone = pickle.load(f)
    assert list(pack) == ['net_weight_pack', 'origins', 'latent_pack', 'thh_pack', 'lod_pack', 'lossless_pack']
    assert pack['lossless_pack'] == alone['lossless_pack']          # the field is the full-resolution decoder's, whatever else travels
    assert "[Lossless] bytes: %d " % len(pack['lossless_pack']) in out and "[LoD 1]" in out
    run([CLI, "decode", "all.pk", "--batchsize", "7", "--N", str(N_BLOCKS), "--lossless"] + COMMON, cwd)
    assert np.array_equal(read(cwd, "rc_dec.ply"), coded["cloud"])
