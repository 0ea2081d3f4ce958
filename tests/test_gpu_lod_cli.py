"""Level-of-detail decode through the command line: train a few epochs on the tiny synthetic cloud, encode with and
without --pack_lod, decode at level 0, 1 and 2.  One training run serves every test of the 10-bit cloud."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "NVFPCC.py")
COMMON = ["--chanstr", "8,16,8,8", "--ch", "3"]
N_BLOCKS = 24


def run(cmd, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert (r.returncode == 0) == ok, r.stdout[-3000:]
    return r.stdout


def read(cwd, name):
    from nvfpcc_amd.recon import read_ply_ascii
    return read_ply_ascii(os.path.join(cwd, name))


def same(a, b):
    """Equal types and equal values, through the containers, arrays and tensors a pack holds."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.detach().cpu(), b.detach().cpu())
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def gross_bpp(out):
    return float(re.search(r"Gross bpp: ([0-9.]+)", out).group(1))


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """train -> quantise -> encode (plain) -> encode --pack_lod, in one directory; the encoders' outputs kept aside."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import write_dataset
    cwd = str(tmp_path_factory.mktemp("lod_cli"))
    gts, _ = write_dataset(os.path.join(cwd, "toy"), N_BLOCKS)
    run([CLI, "train", "toy.ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = [CLI, "encode", "toy.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt",
           "--thh", "0.5"] + COMMON
    out_plain = run(enc + ["--pack_fn", "plain.pk"], cwd)
    os.replace(os.path.join(cwd, "rc_enc.ply"), os.path.join(cwd, "rc_enc_plain.ply"))
    assert not os.path.exists(os.path.join(cwd, "rc_enc_lod1.ply"))
    out_lod = run(enc + ["--pack_fn", "lod.pk", "--pack_lod", "--lod_heads", "ckpts/0010.ckpt"], cwd)
    return {"cwd": cwd, "n_points": int(gts.astype(bool).sum()), "out_plain": out_plain, "out_lod": out_lod, "gts": gts}


def test_pack_lod_adds_one_key_and_its_bits_and_changes_nothing_else(coded):
    from nvfpcc_amd import lod_pack as lp
    cwd = coded["cwd"]
    with open(os.path.join(cwd, "plain.pk"), "rb") as f:
        plain = pickle.load(f)
    with open(os.path.join(cwd, "lod.pk"), "rb") as f:
        lod = pickle.load(f)
    assert list(plain) == ['net_weight_pack', 'origins', 'latent_pack']
    assert list(lod) == list(plain) + ['lod_pack'] and isinstance(lod['lod_pack'], bytes)
    side = lod.pop('lod_pack')
    assert same(plain, lod), "the packs differ beyond the lod_pack key"
    assert len(side) == 13 + 2 * (27 * 8 + 1 + 27 * 16 + 1)
    info = lp.read_lod_pack(side, "8,16,8,8")
    # Gross bpp is printed with four decimals: the two printed values are each within 5e-5 of the exact ones
    rise = gross_bpp(coded["out_lod"]) - gross_bpp(coded["out_plain"])
    assert abs(rise - 8 * len(side) / coded["n_points"]) <= 1.0001e-4, (rise, 8 * len(side) / coded["n_points"])
    # the level-0 outputs of the encoder are the same with and without the flag
    assert np.array_equal(read(cwd, "rc_enc.ply"), read(cwd, "rc_enc_plain.ply"))
    strip = lambda s: [ln for ln in s.splitlines() if ln.startswith("[") and not ln.startswith("[LoD") and "Gross bpp" not in ln]
    assert strip(coded["out_lod"]) == strip(coded["out_plain"])
    # one [LoD l] line per level, with the threshold the pack carries and the count rule's lower bound
    g = torch.from_numpy(coded["gts"]).float()
    for level in (1, 2):
        g = torch.nn.functional.max_pool3d(g, 2)
        m = re.search(r"^\[LoD %d\] t: (\S+) points: (\d+) Pacc: ([0-9.]+) Nacc: ([0-9.]+)$" % level, coded["out_lod"], re.M)
        assert m, coded["out_lod"][-2000:]
        assert float(np.float32(float(m.group(1)))) == float(np.float32(info["t"][level - 1]))
        pts = read(cwd, "rc_enc_lod%d.ply" % level)
        assert int(m.group(2)) == len(pts) >= int(g.sum())
        assert 0.0 <= float(m.group(3)) <= 1.0 and 0.0 <= float(m.group(4)) <= 1.0


@pytest.mark.parametrize("level", [1, 2])
def test_decode_lod_writes_the_encoders_coarse_cloud(coded, level):
    from nvfpcc_amd.synth import make_origins
    cwd = coded["cwd"]
    out = run([CLI, "decode", "lod.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lod", str(level)] + COMMON, cwd)
    dec, enc = read(cwd, "rc_dec.ply"), read(cwd, "rc_enc_lod%d.ply" % level)
    assert enc.shape[0] > 0 and enc.shape == dec.shape and np.array_equal(enc, dec)
    m = re.search(r"^\[LoD %d\] t: (\S+) points: (\d+)$" % level, out, re.M)
    assert m and int(m.group(2)) == len(dec)
    assert m.group(0) in [ln.split(" Pacc")[0] for ln in coded["out_lod"].splitlines()]
    # the coarse lattice: every point inside the cube (origin >> level) + [0, 32 >> level)^3 of one of the blocks
    cubes = {tuple(r) for r in (make_origins(N_BLOCKS).astype(np.int64) >> level).tolist()}
    d = 32 >> level
    assert {tuple(r) for r in ((dec.astype(np.int64) // d) * d).tolist()} <= cubes


def test_decode_without_lod_ignores_lod_pack(coded):
    cwd = coded["cwd"]
    args = ["--batchsize", "1", "--thh", "0.5", "--N", str(N_BLOCKS)] + COMMON
    out_a = run([CLI, "decode", "plain.pk"] + args, cwd)
    a = read(cwd, "rc_dec.ply")
    out_b = run([CLI, "decode", "lod.pk"] + args, cwd)
    b = read(cwd, "rc_dec.ply")
    assert a.shape[0] > 0 and np.array_equal(a, b) and np.array_equal(a, read(cwd, "rc_enc_plain.ply"))
    assert "[LoD" not in out_a and "[LoD" not in out_b


def test_decode_lod_needs_lod_pack_and_encode_needs_the_heads(coded):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "plain.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lod", "1"] + COMMON, cwd, ok=False)
    assert "carries no lod_pack" in out and "--pack_lod" in out and "Traceback" not in out
    # the quantised checkpoint holds no coarse heads: encode says where to find them
    out = run([CLI, "encode", "toy.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb",
               "ckpts/0010_emb.ckpt", "--pack_fn", "never.pk", "--pack_lod"] + COMMON, cwd, ok=False)
    assert "--lod_heads" in out and "conv1_cls" in out and "Traceback" not in out
    assert not os.path.exists(os.path.join(cwd, "never.pk"))
    # heads of another decoder
    out = run([CLI, "decode", "lod.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lod", "2", "--chanstr",
               "16,32,16,16", "--ch", "3"], cwd, ok=False)
    assert "do not fit --chanstr" in out and "Traceback" not in out


@pytest.mark.timeout(600)
def test_eleven_bit_cloud_decodes_on_the_coarser_lattice(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd import preprocess as pp
    from tests.golden_inputs import write_cloud_ply
    from tests.test_gpu_preprocess_deep import shell_patch
    pts = np.unique(shell_patch((1024, 1024, 1024), 12.0, 3000, 5), axis=0)     # the eight blocks around one corner
    origins = pp.octree_partition(pts, 11)[0]
    assert len(origins) == 8
    cwd = str(tmp_path)
    write_cloud_ply(os.path.join(cwd, "cloud.ply"), pts)
    run([CLI, "train", "cloud.ply", "--from_ply", "--bits", "11", "--checkpoint_dir", "ckpts", "--batchsize", "4",
         "--lambda", "200", "--lr", "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True",
         "--epochs", "2", "--phase_change", "1"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0000.ckpt", "q4.ckpt", "16"], cwd)
    out = run([CLI, "encode", "cloud.ply", "--from_ply", "--pack_octree", "--bits", "11", "--pack_lod", "--lod_heads",
               "ckpts/0000.ckpt", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0000_emb.ckpt"]
              + COMMON, cwd)
    assert "[LoD 1]" in out and "[LoD 2]" in out
    with open(os.path.join(cwd, "pack.pk"), "rb") as f:
        assert list(pickle.load(f)) == ['net_weight_pack', 'latent_pack', 'octree_pack', 'lod_pack']
    for level in (1, 2):
        out = run([CLI, "decode", "pack.pk", "--batchsize", "3", "--lod", str(level), "--ref_ply", "cloud.ply"] + COMMON, cwd)
        dec, enc = read(cwd, "rc_dec.ply"), read(cwd, "rc_enc_lod%d.ply" % level)
        assert len(dec) > 0 and np.array_equal(dec, enc)
        # bits - l = 10 or 9 bits per axis
        top = 2048 >> level
        assert dec.min() >= 0 and dec.max() < top
        d = 32 >> level
        cubes = {tuple(r) for r in (np.asarray(origins, np.int64) >> level).tolist()}
        assert {tuple(r) for r in ((dec.astype(np.int64) // d) * d).tolist()} <= cubes
        ref_n = len(np.unique(pts >> level, axis=0))
        assert "[PCError] LoD %d: %d reference points on the %d-bit lattice, peak %d" % (level, ref_n, 11 - level, top - 1) in out
        m = re.search(r"\[PCError\] D1 PSNR: (\S+) D2 PSNR: (\S+)", out)
        assert m and np.isfinite(float(m.group(1)))
