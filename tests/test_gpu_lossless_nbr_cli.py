"""The neighbour contexts through the command line, on the toy cloud and the recipe of tests/test_gpu_lossless_lod_cli.py:
encode --lossless_lod --lossless_ctx nbr, decode --lossless_lod 0 | 1 | 2 with no new flag, and the same encode without
--lossless_ctx, which must go on writing the field contexts' pack.  One training run serves every test."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_lod_cli import CLI, COMMON, N_BLOCKS, ROOT, gross_bpp, read, run, same
from tests.test_gpu_lossless_lod_cli import load, rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """train -> quantise -> encode --lossless_lod, with --lossless_ctx field, with --lossless_ctx nbr."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    from tests.golden_inputs import write_cloud_ply
    cwd = str(tmp_path_factory.mktemp("lossless_nbr_cli"))
    gts, _ = write_dataset(os.path.join(cwd, "toy"), N_BLOCKS)
    nz = np.argwhere(gts.reshape(N_BLOCKS, 32, 32, 32))
    cloud = nz[:, 1:] + make_origins(N_BLOCKS).astype(np.int64)[nz[:, 0]]      # the input's voxels, (block, raster) order
    write_cloud_ply(os.path.join(cwd, "cloud.ply"), cloud)
    run([CLI, "train", "toy.ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = [CLI, "encode", "toy.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt",
           "--thh", "0.5", "--lossless_lod"] + COMMON
    out = {"cwd": cwd, "cloud": cloud}
    for name, flags in (("lod", []), ("field", ["--lossless_ctx", "field"]), ("nbr", ["--lossless_ctx", "nbr"])):
        out[name] = run(enc + ["--pack_fn", name + ".pk"] + flags, cwd)
    return out


def lod_line(out):
    m = re.search(r"^\[LosslessLoD\] bytes: (\d+) bpp: ([0-9.]+) ideal bpp: ([0-9.]+) contexts: (\d+) symbols: (\d+) group: 64$",
                  out, re.M)
    assert m, out[-2000:]
    return m


def test_without_the_flag_encode_writes_the_field_contexts_pack(coded):
    """Version 1, the layout lossless_lod_pack.read knows, the same bytes as with --lossless_ctx field and the same
    output: tests/test_gpu_lossless_lod.py holds those bytes to the numpy reference, which this change leaves alone."""
    from nvfpcc_amd import lossless_lod_pack as llp
    cwd = coded["cwd"]
    lod, field = load(cwd, "lod.pk"), load(cwd, "field.pk")
    assert list(lod) == ['net_weight_pack', 'origins', 'latent_pack', 'lossless_lod_pack']
    assert same(lod, field) and coded["lod"] == coded["field"]
    side = lod['lossless_lod_pack']
    assert side[0] == 1 and struct_contexts(side) == 3072
    info = llp.read(side, N_BLOCKS)
    assert len(side) == llp.size(N_BLOCKS, 64, int(info["nwords"].sum()), int(info["used"].sum()))
    assert int(lod_line(coded["lod"]).group(1)) == len(side)


def struct_contexts(side):
    return int.from_bytes(side[7:9], "little")


def test_nbr_changes_only_the_side_pack_and_its_line(coded):
    from nvfpcc_amd import lossless_nbr_pack as lp
    cwd, n_points = coded["cwd"], coded["cloud"].shape[0]
    lod, nbr = load(cwd, "lod.pk"), load(cwd, "nbr.pk")
    assert list(nbr) == list(lod)
    side, was = nbr.pop('lossless_lod_pack'), lod.pop('lossless_lod_pack')
    assert same(lod, nbr) and isinstance(side, bytes) and side[0] == 3 and struct_contexts(side) == 35840
    assert lp.module_of(side) is lp and lp.module_of(was) is not lp
    info = lp.read(side, N_BLOCKS)
    n_used = int(info["used"].sum())
    slots0 = int(info["used"][3072:].reshape(32, 1024).any(0).sum())
    assert info["group"] == 64 and len(side) == lp.size(N_BLOCKS, 64, int(info["nwords"].sum()), n_used, slots0)
    m, m_was = lod_line(coded["nbr"]), lod_line(coded["lod"])
    assert int(m.group(1)) == len(side) and int(m.group(4)) == n_used and m.group(5) == m_was.group(5)
    print("field: %s\nnbr:   %s" % (m_was.group(0), m.group(0)))
    rise = gross_bpp(coded["nbr"]) - gross_bpp(coded["lod"])
    assert abs(rise - 8 * (len(side) - len(was)) / n_points) <= 1.0001e-4
    strip = lambda s: [ln for ln in s.splitlines() if ln.startswith("[") and not ln.startswith("[LosslessLoD]") and "Gross bpp" not in ln]
    assert strip(coded["nbr"]) == strip(coded["lod"])
    # the coder's bound: headers and table, 4096 bits of states per group, log2(1 + 2^-15) per coded symbol
    over = 8 * len(side) - float(m.group(3)) * n_points
    table = 9 + 384 + 4 * slots0 + 2 * n_used + 4
    assert -0.5e-4 * n_points <= over <= 8 * table + 4096 + int(m.group(5)) * np.log2(1 + 2.0 ** -15) + 0.5e-4 * n_points


@pytest.mark.parametrize("level", [0, 1, 2])
def test_decode_tells_the_pack_by_itself_and_writes_exactly_the_input_at_the_level(coded, level):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "nbr.pk", "--batchsize", "7" if level == 1 else "1", "--N", str(N_BLOCKS), "--lossless_lod",
               str(level), "--ref_ply", "cloud.ply"] + COMMON, cwd)
    dec = read(cwd, "rc_dec.ply")
    want = rows(coded["cloud"] >> level)
    assert dec.shape == want.shape and np.array_equal(rows(dec), want)
    if level == 0:
        assert np.array_equal(dec, coded["cloud"])                               # in (block, raster) order
    assert "[LosslessLoD] level: %d points: %d" % (level, len(dec)) in out
    assert re.search(r"^\[PCError\] D1 PSNR: inf D2 PSNR: \S+$", out, re.M), out[-2000:]


REFUSALS = {
    "ctx without lossless_lod": (None, "--lossless_ctx nbr chooses the contexts of --lossless_lod"),
    "damaged stream": (lambda b: b[:-2] + bytes([b[-2] ^ 0x40]) + b[-1:],
                       "decode --lossless_lod 0: lossless_lod_pack: the stream of group 0 is damaged"),
    "unknown version": (lambda b: b"\x02" + b[1:], "decode --lossless_lod 0: lossless_lod_pack: version 2, the readers know 1"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_exit_with_their_message(coded, case):
    cwd = coded["cwd"]
    edit, message = REFUSALS[case]
    if edit is None:
        out = run([CLI, "encode", "toy.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt",
                   "--thh", "0.5", "--pack_fn", "never.pk", "--lossless_ctx", "nbr"] + COMMON, cwd, ok=False)
        assert not os.path.exists(os.path.join(cwd, "never.pk"))
    else:
        pack = load(cwd, "nbr.pk")
        with open(os.path.join(cwd, "edited.pk"), "wb") as f:
            pickle.dump(dict(pack, lossless_lod_pack=edit(pack["lossless_lod_pack"])), f)
        out = run([CLI, "decode", "edited.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lossless_lod", "0"] + COMMON, cwd, ok=False)
    assert message in out and "Traceback" not in out
