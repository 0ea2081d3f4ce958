"""A latents-only pack through the command line: frame 0 trained, quantised and encoded as the reference; frame 1 fitted
under its frozen decoder (train --freeze_decoder), encoded with --ref_pack and decoded with it.  One setup serves every
test.  The centre: the P pack joined with its reference IS the pack the same encode writes without --ref_pack."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_gof_cli import load, raw
from tests.test_gpu_lod_cli import CLI, COMMON, ROOT, read, run, same

pytestmark = pytest.mark.gpu
BLOCKS = 8
TRAIN = ["--checkpoint_dir", "ckpts", "--lambda", "200", "--lr", "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5"] + COMMON
DEC = ["--batchsize", "1", "--thh", "0.5", "--N", str(BLOCKS)] + COMMON


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    cwd = str(tmp_path_factory.mktemp("pframe_cli"))
    clouds, points = [], []
    for k, seed in enumerate((20221, 21221)):
        gts, _ = write_dataset(os.path.join(cwd, "frame%d" % k), BLOCKS, base_seed=seed)
        nz = np.argwhere(gts.reshape(BLOCKS, 32, 32, 32))
        clouds.append(nz[:, 1:] + make_origins(BLOCKS).astype(np.int64)[nz[:, 0]])
        points.append(int(gts.astype(bool).sum()))
    run([CLI, "train", "frame0.ply", "--epochs", "11", "--phase_change", "5", "--batchsize", "1", "--shuffle", "True"] + TRAIN, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q3.ckpt", "8"], cwd)
    enc = ["--batchsize", "5", "--load_weights", "q4.ckpt", "--thh", "0.5"] + COMMON
    run([CLI, "encode", "frame0.ply", "--load_emb", "ckpts/0010_emb.ckpt", "--pack_fn", "ref.pk"] + enc, cwd)
    out_fit = run([CLI, "train", "frame1.ply", "--freeze_decoder", "--load_weights", "q4.ckpt", "--ref_pack", "ref.pk",
                   "--load_emb", "ckpts/0010_emb.ckpt", "--epochs", "21"] + TRAIN[2:] + ["--checkpoint_dir", "fit"], cwd)
    enc1 = [CLI, "encode", "frame1.ply", "--load_emb", "fit/0020_emb.ckpt", "--lossless"] + enc
    out_plain = run(enc1 + ["--pack_fn", "plain1.pk"], cwd)
    os.replace(os.path.join(cwd, "rc_enc.ply"), os.path.join(cwd, "rc_enc_plain.ply"))
    out_p = run(enc1 + ["--pack_fn", "p.pk", "--ref_pack", "ref.pk"], cwd)
    return {"cwd": cwd, "clouds": clouds, "points": points, "out_fit": out_fit, "out_plain": out_plain, "out_p": out_p, "enc": enc}


def test_the_p_pack_is_the_plain_pack_without_its_weights(coded):
    from nvfpcc_amd import pframe
    cwd = coded["cwd"]
    p, ref, plain = load(cwd, "p.pk"), load(cwd, "ref.pk"), load(cwd, "plain1.pk")
    assert list(p) == ["ref_pack", "origins", "latent_pack", "lossless_pack"] and "net_weight_pack" not in p
    assert p["ref_pack"] == b"\x01" + pframe.digest(ref["net_weight_pack"])
    assert same(pframe.join(p, ref), plain)
    assert raw(cwd, "rc_enc.ply") == raw(cwd, "rc_enc_plain.ply")


def test_decode_with_the_reference(coded):
    cwd = coded["cwd"]
    run([CLI, "decode", "p.pk", "--ref_pack", "ref.pk"] + DEC, cwd)
    assert raw(cwd, "rc_dec.ply") == raw(cwd, "rc_enc.ply")
    out = run([CLI, "decode", "p.pk", "--ref_pack", "ref.pk", "--lossless"] + DEC, cwd)
    dec = read(cwd, "rc_dec.ply")
    assert dec.shape == coded["clouds"][1].shape and np.array_equal(dec, coded["clouds"][1])
    assert "[Lossless] points: %d" % coded["points"][1] in out
    assert coded["clouds"][0].tobytes() != coded["clouds"][1].tobytes(), "the two frames differ"


def test_refusals_exit_with_their_message(coded):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "p.pk"] + DEC, cwd, ok=False)
    assert "--ref_pack" in out and "Traceback" not in out
    ref = load(cwd, "ref.pk")
    stream = bytearray(ref["net_weight_pack"]["bit_stream"])
    assert len(stream) > 8, "the reference's kernels do not all round to one value: there are weight bytes to damage"
    stream[len(stream) // 2] ^= 0x04
    with open(os.path.join(cwd, "badref.pk"), "wb") as f:
        pickle.dump(dict(ref, net_weight_pack=dict(ref["net_weight_pack"], bit_stream=bytes(stream))), f)
    out = run([CLI, "decode", "p.pk", "--ref_pack", "badref.pk"] + DEC, cwd, ok=False)
    assert "--ref_pack" in out and "badref.pk" in out and "Traceback" not in out
    out = run([CLI, "decode", "p.pk", "--ref_pack", "p.pk"] + DEC, cwd, ok=False)      # a P pack is no reference
    assert "--ref_pack" in out and "net_weight_pack" in out and "Traceback" not in out
    # a checkpoint quantised at another qp is another decoder
    enc = [CLI, "encode", "frame1.ply", "--load_emb", "fit/0020_emb.ckpt", "--batchsize", "5", "--load_weights", "q3.ckpt",
           "--qp", "8", "--thh", "0.5", "--pack_fn", "never.pk", "--ref_pack", "ref.pk"] + COMMON
    out = run(enc, cwd, ok=False)
    assert "q3.ckpt" in out and "ref.pk" in out and "Traceback" not in out
    assert not os.path.exists(os.path.join(cwd, "never.pk"))
    out = run([CLI, "train", "frame1.ply", "--freeze_decoder", "--epochs", "3"] + TRAIN, cwd, ok=False)
    assert "--load_weights" in out and "Traceback" not in out and "[data]" not in out


def test_printed_values(coded):
    p, out = load(coded["cwd"], "p.pk"), coded["out_p"]
    lat, side = 8 * len(p["latent_pack"]["latent_byte_stream"]), 8 * len(p["lossless_pack"])
    gross = re.findall(r"^\[Latent code\] Gross bpp: ([0-9.]+)$", out, re.M)
    exact = (lat + side + 33 * 8) / float(coded["points"][1])
    assert len(gross) == 1 and abs(float(gross[0]) - exact) <= 5.0001e-5, (gross, exact)
    plain = re.findall(r"^\[Latent code\] Gross bpp: ([0-9.]+)$", coded["out_plain"], re.M)
    assert float(plain[0]) > float(gross[0])
    fit = re.findall(r"^\[Fit (\d{4}) [0-9.]+ seconds\] J: ([0-9.e+-]+) improved: (\d+) / (\d+) b_latent: ([0-9.]+)$",
                     coded["out_fit"], re.M)
    assert [int(f[0]) for f in fit] == [0, 10, 20, 21], coded["out_fit"][-2000:]
    sums = [float(f[1]) for f in fit]
    print("[pframe cli] fit cost sums:", sums, "improved:", [int(f[2]) for f in fit])
    assert all(b <= a for a, b in zip(sums, sums[1:])), sums
    assert int(fit[0][2]) == 0 and all(int(f[3]) == BLOCKS for f in fit)
    emb = torch.load(os.path.join(coded["cwd"], "fit", "0020_emb.ckpt"), map_location="cpu")
    assert tuple(emb.shape) == (BLOCKS, 3, 2, 2, 2)
