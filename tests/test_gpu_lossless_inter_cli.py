"""The inter contexts through the command line, on the toy cloud and the recipe of tests/test_gpu_lossless_nbr_cli.py.
Frame A is coded with --lossless_lod and decoded to its rc_dec.ply; frame B is A with a third of its blocks' points moved
by one voxel, coded with --lossless_ctx inter --lossless_ref under A's decoded cloud (and A's latents: the stream is exact
under any field) and decoded at the three levels with the same reference.  One training run serves every test."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

from tests import occ_inter_ref as I
from tests.test_gpu_lod_cli import CLI, COMMON, N_BLOCKS, ROOT, read, run, same
from tests.test_gpu_lossless_lod_cli import load, rows

pytestmark = pytest.mark.gpu


def cloud_of(gts, origins):
    nz = np.argwhere(gts.reshape(N_BLOCKS, 32, 32, 32))
    return nz[:, 1:] + origins.astype(np.int64)[nz[:, 0]]        # the voxels, (block, raster) order


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """train A -> quantise -> encode A --lossless_lod -> decode it (a_dec.ply) -> encode B: plain contexts, nbr, inter."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    from tests.golden_inputs import write_cloud_ply
    cwd = str(tmp_path_factory.mktemp("lossless_inter_cli"))
    gts, dists = write_dataset(os.path.join(cwd, "toy"), N_BLOCKS)
    origins = make_origins(N_BLOCKS)
    moved = gts.reshape(N_BLOCKS, -1).astype(bool)
    moved[::3] = I.shifted(moved[::3], 0, 1, 0)                    # every third block: its points one voxel along y
    gts_b = moved.reshape(gts.shape).astype(gts.dtype)
    dists_b = dists.copy()
    dists_b[::3] = np.roll(dists[::3], 1, axis=3)                  # only the [Recon] line reads the distances
    np.save(os.path.join(cwd, "toyb_l5_origins.npy"), origins)
    np.save(os.path.join(cwd, "toyb_l5_gt_grid.npy"), gts_b)
    np.save(os.path.join(cwd, "toyb_l5_dist.npy"), dists_b)
    cloud_a, cloud_b = cloud_of(gts, origins), cloud_of(gts_b, origins)
    write_cloud_ply(os.path.join(cwd, "cloud_b.ply"), cloud_b)
    run([CLI, "train", "toy.ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = ["--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt", "--thh", "0.5",
           "--lossless_lod"] + COMMON
    out = {"cwd": cwd, "cloud_a": cloud_a, "cloud_b": cloud_b}
    out["a"] = run([CLI, "encode", "toy.ply", "--pack_fn", "a.pk"] + enc, cwd)
    run([CLI, "decode", "a.pk", "--batchsize", "7", "--N", str(N_BLOCKS), "--lossless_lod", "0"] + COMMON, cwd)
    shutil.copy(os.path.join(cwd, "rc_dec.ply"), os.path.join(cwd, "a_dec.ply"))
    for name, flags in (("b_lod", []), ("b_nbr", ["--lossless_ctx", "nbr"]),
                        ("b_inter", ["--lossless_ctx", "inter", "--lossless_ref", "a_dec.ply"])):
        out[name] = run([CLI, "encode", "toyb.ply", "--pack_fn", name + ".pk"] + enc + flags, cwd)
    return out


def lod_line(out):
    m = re.search(r"^\[LosslessLoD\] bytes: (\d+) bpp: ([0-9.]+) ideal bpp: ([0-9.]+) contexts: (\d+) symbols: (\d+) group: 64$",
                  out, re.M)
    assert m, out[-2000:]
    return m


def test_the_reference_is_frame_a_and_b_moved(coded):
    a, b = coded["cloud_a"], coded["cloud_b"]
    assert np.array_equal(read(coded["cwd"], "a_dec.ply"), a)
    both = len(rows(np.concatenate([a, b])))
    assert 0.5 * len(a) < len(a) + len(b) - both < len(a) and len(b) <= len(a)      # two thirds stand still, not all


def test_inter_changes_only_the_side_pack_and_is_smaller_than_nbr(coded):
    from nvfpcc_amd import lossless_inter_pack as lp, lossless_lod_pack as llp
    cwd = coded["cwd"]
    lod, nbr, inter = load(cwd, "b_lod.pk"), load(cwd, "b_nbr.pk"), load(cwd, "b_inter.pk")
    assert list(inter) == list(lod) == ['net_weight_pack', 'origins', 'latent_pack', 'lossless_lod_pack']
    side, three, one = inter.pop('lossless_lod_pack'), nbr.pop('lossless_lod_pack'), lod.pop('lossless_lod_pack')
    assert same(lod, inter) and same(lod, nbr)
    # without the new flag and choice: version 1 and version 3, as before
    assert one[0] == 1 and three[0] == 3 and lp.module_of(one) is llp and llp.read(one, N_BLOCKS)["f1"].size == 3072
    assert isinstance(side, bytes) and side[0] == 4 and int.from_bytes(side[7:9], "little") == 52224
    assert lp.module_of(side) is lp
    info = lp.read(side, N_BLOCKS)
    n_used = int(info["used"].sum())
    slots0 = int(info["used"][3072:].reshape(48, 1024).any(0).sum())
    assert info["group"] == 64 and len(side) == lp.size(N_BLOCKS, 64, int(info["nwords"].sum()), n_used, slots0)
    ref, dropped = I.reference_words(coded["cloud_a"], load(cwd, "b_lod.pk")["origins"])
    assert dropped == 0 and info["digest"] == lp.digest(I.H.words_of(ref))
    m, m_nbr = lod_line(coded["b_inter"]), lod_line(coded["b_nbr"])
    assert int(m.group(1)) == len(side) and int(m.group(4)) == n_used and m.group(5) == m_nbr.group(5)
    assert int(m_nbr.group(1)) == len(three)
    print("nbr:   %s\ninter: %s" % (m_nbr.group(0), m.group(0)))
    assert len(side) < len(three)
    assert "[LosslessLoD] reference: a_dec.ply points: %d dropped: 0" % len(coded["cloud_a"]) in coded["b_inter"]
    strip = lambda s: [ln for ln in s.splitlines() if ln.startswith("[") and not ln.startswith("[LosslessLoD]") and "Gross bpp" not in ln]
    assert strip(coded["b_inter"]) == strip(coded["b_lod"])


@pytest.mark.parametrize("level", [0, 1, 2])
def test_decode_with_the_reference_writes_exactly_frame_b_at_the_level(coded, level):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "b_inter.pk", "--batchsize", "7" if level == 1 else "1", "--N", str(N_BLOCKS), "--lossless_lod",
               str(level), "--lossless_ref", "a_dec.ply", "--ref_ply", "cloud_b.ply"] + COMMON, cwd)
    dec = read(cwd, "rc_dec.ply")
    want = rows(coded["cloud_b"] >> level)
    assert dec.shape == want.shape and np.array_equal(rows(dec), want)
    if level == 0:
        assert np.array_equal(dec, coded["cloud_b"])                             # in (block, raster) order
    assert "[LosslessLoD] level: %d points: %d" % (level, len(dec)) in out
    assert "[LosslessLoD] reference: a_dec.ply points: %d dropped: 0" % len(coded["cloud_a"]) in out
    assert re.search(r"^\[PCError\] D1 PSNR: inf D2 PSNR: \S+$", out, re.M), out[-2000:]


DECODE_B = [CLI, "decode", "b_inter.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lossless_lod", "0"] + COMMON


def test_decode_without_the_flag_exits_with_its_reason(coded):
    out = run(DECODE_B, coded["cwd"], ok=False)
    assert "was coded under a reference cloud (--lossless_ctx inter); name that cloud with --lossless_ref" in out
    assert "Traceback" not in out


def test_decode_under_another_reference_exits_on_the_digest(coded):
    out = run(DECODE_B + ["--lossless_ref", "cloud_b.ply"], coded["cwd"], ok=False)      # B's own cloud: not what B was coded under
    assert "decode --lossless_lod 0: lossless_lod_pack: the reference is not the one the pack was coded under" in out
    assert "the reference sets %d voxels" % len(coded["cloud_b"]) in out and "Traceback" not in out


def test_a_pack_that_refers_to_no_cloud_leaves_the_file_unread(coded):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "b_nbr.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lossless_lod", "0", "--lossless_ref",
               "no_such.ply"] + COMMON, cwd)
    assert "refers to no other cloud; --lossless_ref no_such.ply is not read" in out
    assert np.array_equal(read(cwd, "rc_dec.ply"), coded["cloud_b"])


def test_encode_inter_without_a_reference_writes_no_pack(coded):
    cwd = coded["cwd"]
    out = run([CLI, "encode", "toyb.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt",
               "--pack_fn", "never.pk", "--lossless_lod", "--lossless_ctx", "inter"] + COMMON, cwd, ok=False)
    assert "name it with --lossless_ref" in out and not os.path.exists(os.path.join(cwd, "never.pk"))
