"""--voxelize through the command line, on the 24-block toy cloud and the flags of tests/test_gpu_lod_cli.py: the integer
cloud coded with --from_ply, and the same cloud as float32 points in a frame of its own -- jittered, every tenth point
twice, shuffled -- coded with --from_ply --voxelize under the lattice that maps it back.  One training run serves every
test."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import voxelize_ref as R
from tests.test_gpu_lod_cli import CLI, COMMON, N_BLOCKS, ROOT, gross_bpp, read, run, same

pytestmark = pytest.mark.gpu
O, S = (-3.2, 1e3, 7.5), 0.0137
LAT = R.RefLattice(10, O, S)
VOX = ["--from_ply", "--voxelize", "--vox_step", repr(S), "--vox_origin"] + [repr(v) for v in O]
DECODE = ["--batchsize", "1", "--N", str(N_BLOCKS)] + COMMON


def write_float32_ply(path, xyz):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n" % len(xyz)).encode())
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes())


def rows(a):
    """The rows of an [n, 3] array in lexicographic order."""
    a = np.asarray(a)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def lines(out):
    return [ln for ln in out.splitlines() if ln.startswith("[") and "Gross bpp" not in ln and not ln.startswith("[Voxelize]")]


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """cloud.ply / cloud_f.ply -> train cloud.ply --from_ply -> quantise -> encode both, each with --lossless_lod and the
    threshold chosen by count (eleven epochs need not lift a probability over a fixed threshold)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd import ply_io
    from nvfpcc_amd.synth import make_blocks, make_origins
    cwd = str(tmp_path_factory.mktemp("voxelize_cli"))
    gts, _ = make_blocks(N_BLOCKS)
    origins = make_origins(N_BLOCKS).astype(np.int64)
    q = np.concatenate([origins[b] + np.argwhere(gts[b, 0]) for b in range(N_BLOCKS)])
    assert len(np.unique(q, axis=0)) == len(q)
    ply_io.write_ply(os.path.join(cwd, "cloud.ply"), q)
    rng = np.random.default_rng(7)
    twice = np.concatenate([q, q[::10]])
    xf = np.asarray(O) + (twice + rng.uniform(-0.25, 0.25, size=twice.shape)) * S
    xf = xf[rng.permutation(len(xf))].astype(np.float32)
    write_float32_ply(os.path.join(cwd, "cloud_f.ply"), xf)
    run([CLI, "train", "cloud.ply", "--from_ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr",
         "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"]
        + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = ["--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt", "--thh_mode", "count",
           "--lossless_lod"] + COMMON
    out_plain = run([CLI, "encode", "cloud.ply", "--from_ply", "--pack_fn", "plain.pk"] + enc, cwd)
    os.replace(os.path.join(cwd, "rc_enc.ply"), os.path.join(cwd, "rc_enc_plain.ply"))
    out_vox = run([CLI, "encode", "cloud_f.ply", "--pack_fn", "vox.pk"] + VOX + enc, cwd)
    return {"cwd": cwd, "q": q, "n_in": len(xf), "out_plain": out_plain, "out_vox": out_vox}


def test_encode_of_the_float_cloud_equals_encode_of_the_integer_cloud(coded):
    from nvfpcc_amd import voxelize as vx
    cwd, m = coded["cwd"], len(coded["q"])
    with open(os.path.join(cwd, "plain.pk"), "rb") as f:
        plain = pickle.load(f)
    with open(os.path.join(cwd, "vox.pk"), "rb") as f:
        vox = pickle.load(f)
    assert "vox_pack" not in plain and list(vox) == list(plain) + ["vox_pack"]
    side = vox.pop("vox_pack")
    assert isinstance(side, bytes) and len(side) == 34 and vx.unpack(side) == vx.Lattice(*LAT)
    assert same(plain, vox), "the packs differ beyond the vox_pack key"
    assert np.array_equal(read(cwd, "rc_enc.ply"), read(cwd, "rc_enc_plain.ply")) and len(read(cwd, "rc_enc.ply")) > 0
    # every [...] line but Gross bpp and [Voxelize]: the counts downstream are the voxels', not the points'
    assert lines(coded["out_vox"]) == lines(coded["out_plain"]) and len(lines(coded["out_vox"])) >= 4
    assert "[data] %d leaf blocks, %d points" % (N_BLOCKS, m) in coded["out_vox"]
    # Gross bpp is printed with four decimals: the two printed values are each within 5e-5 of the exact ones
    rise = gross_bpp(coded["out_vox"]) - gross_bpp(coded["out_plain"])
    assert abs(rise - 8 * 34 / m) <= 1.0001e-4, (rise, 8 * 34 / m)
    assert "[Voxelize]" not in coded["out_plain"]
    v = re.search(r"^\[Voxelize\] points: (\d+) voxels: (\d+) bits: 10 step: (\S+) origin: (\S+) (\S+) (\S+) rms err: (\S+) "
                  r"\((\S+) steps\) max err: (\S+)$", coded["out_vox"], re.M)
    assert v, coded["out_vox"][-2000:]
    assert (int(v.group(1)), int(v.group(2))) == (coded["n_in"], m) and coded["n_in"] == m + len(coded["q"][::10])
    assert float(v.group(3)) == S and tuple(float(v.group(k)) for k in (4, 5, 6)) == O
    assert 0.0 < float(v.group(8)) < 0.25 * np.sqrt(3.0) and abs(float(v.group(7)) / S - float(v.group(8))) < 1e-3
    assert float(v.group(7)) <= float(v.group(9)) < 0.26 * np.sqrt(3.0) * S


@pytest.mark.parametrize("fmt", ["ascii", "binary"])
def test_decode_source_frame_writes_to_source_of_the_decoded_cloud(coded, fmt):
    from nvfpcc_amd import ply_io, voxelize as vx
    cwd = coded["cwd"]
    run([CLI, "decode", "vox.pk", "--source_frame", "--ply_format", fmt] + DECODE, cwd)
    dec = ply_io.read_ply(os.path.join(cwd, "rc_dec.ply"))[0]
    src = ply_io.read_ply(os.path.join(cwd, "rc_dec_src.ply"), coords="float")[0]
    with open(os.path.join(cwd, "rc_dec_src.ply"), "rb") as f:
        assert (b"format ascii" if fmt == "ascii" else b"format binary_little_endian") in f.read(64)
    assert len(dec) > 0 and np.array_equal(dec, read(cwd, "rc_enc_plain.ply").astype(np.int64))
    want = vx.to_source(dec, vx.Lattice(*LAT), "cuda").cpu().numpy()
    assert src.dtype == np.float64 and np.array_equal(src.view(np.int64), want.view(np.int64))       # bit for bit
    assert np.array_equal(want.view(np.int64), R.to_source(dec, LAT).view(np.int64))


@pytest.mark.parametrize("level", [0, 1])
def test_lossless_decode_in_the_source_frame_is_the_inputs_voxels(coded, level):
    from nvfpcc_amd import ply_io
    cwd = coded["cwd"]
    out = run([CLI, "decode", "vox.pk", "--source_frame", "--lossless_lod", str(level), "--ref_ply", "cloud_f.ply"] + DECODE, cwd)
    dec = ply_io.read_ply(os.path.join(cwd, "rc_dec.ply"))[0]
    src = ply_io.read_ply(os.path.join(cwd, "rc_dec_src.ply"), coords="float")[0]
    voxels = np.unique(coded["q"] >> level, axis=0)
    assert np.array_equal(rows(dec), voxels)
    # at level L the step is s 2^L and the origin is the lattice's
    want = np.asarray(O) + voxels.astype(np.float64) * (S * 2.0 ** level)
    assert np.array_equal(rows(src).view(np.int64), rows(want).view(np.int64))
    assert np.array_equal(src.view(np.int64), R.to_source(dec, LAT, level=level).view(np.int64))
    # the reference has float coordinates: voxelised under the pack's lattice, it is the decoded cloud
    assert re.search(r"^\[PCError\] D1 PSNR: inf ", out, re.M), out[-2000:]


def test_decode_without_source_frame_is_the_plain_packs_decode(coded):
    cwd = coded["cwd"]
    out_a = run([CLI, "decode", "plain.pk"] + DECODE, cwd)
    a = read(cwd, "rc_dec.ply")
    for name in os.listdir(cwd):
        if name.startswith("rc_dec_src"):
            os.remove(os.path.join(cwd, name))
    out_b = run([CLI, "decode", "vox.pk"] + DECODE, cwd)
    b = read(cwd, "rc_dec.ply")
    assert len(a) > 0 and np.array_equal(a, b) and out_a == out_b
    assert not [name for name in os.listdir(cwd) if name.startswith("rc_dec_src")]


def test_source_frame_needs_vox_pack(coded):
    out = run([CLI, "decode", "plain.pk", "--source_frame"] + DECODE, coded["cwd"], ok=False)
    assert "carries no vox_pack" in out and "--voxelize" in out and "Traceback" not in out


def test_the_module_writes_the_integer_cloud(coded):
    from nvfpcc_amd import ply_io
    cwd = coded["cwd"]
    out = run(["-m", "nvfpcc_amd.voxelize", "cloud_f.ply", "out.ply"] + VOX[2:], cwd)
    assert ("[Voxelize] points: %d voxels: %d bits: 10" % (coded["n_in"], len(coded["q"]))) in out
    got = ply_io.read_ply(os.path.join(cwd, "out.ply"))[0]
    assert np.array_equal(got, rows(coded["q"]))          # ascending key order is lexicographic order
    # the cloud's own fit holds every point: its extent is 1023 steps and a bit, so the jitter merges a few more points
    out = run(["-m", "nvfpcc_amd.voxelize", "cloud_f.ply", "out_fit.ply", "--bits", "11", "--ply_format", "binary"], cwd)
    m = re.search(r"^\[Voxelize\] points: (\d+) voxels: (\d+) bits: 11 ", out, re.M)
    fit = ply_io.read_ply(os.path.join(cwd, "out_fit.ply"))[0]
    assert m and int(m.group(1)) == coded["n_in"] and int(m.group(2)) == len(fit) and 0 <= fit.min() and fit.max() == 2047
