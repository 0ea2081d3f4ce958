"""Block motion compensation through the command line, on the toy cloud and the recipe of
tests/test_gpu_lossless_inter_cli.py.  Frame A is coded with --lossless_lod and decoded to a_dec.ply; frame B is A with
every third block's points moved by (0, 2, -1) and every third-plus-one's by (-2, 0, 1), coded under A's decoded cloud
with and without --lossless_mv 2 and decoded at the three levels with the same reference and no new flag.  One training
run serves every test."""
import os
import pickle
import re
import shutil

import numpy as np
import pytest
import torch

from tests import occ_inter_ref as I
from tests import occ_motion_ref as M
from tests.test_gpu_lod_cli import CLI, COMMON, N_BLOCKS, ROOT, read, run, same
from tests.test_gpu_lossless_inter_cli import cloud_of, lod_line
from tests.test_gpu_lossless_lod_cli import load, rows

pytestmark = pytest.mark.gpu
INTER = ["--lossless_ctx", "inter", "--lossless_ref", "a_dec.ply"]


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """train A -> quantise -> encode A --lossless_lod -> decode it (a_dec.ply) -> encode B under it: inter (twice), inter
    with --lossless_mv 2."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    from tests.golden_inputs import write_cloud_ply
    cwd = str(tmp_path_factory.mktemp("lossless_mv_cli"))
    gts, dists = write_dataset(os.path.join(cwd, "toy"), N_BLOCKS)
    origins = make_origins(N_BLOCKS)
    moved = gts.reshape(N_BLOCKS, -1).astype(bool)
    moved[0::3] = I.shifted(moved[0::3], 0, 2, -1)
    moved[1::3] = I.shifted(moved[1::3], -2, 0, 1)
    gts_b = moved.reshape(gts.shape).astype(gts.dtype)
    np.save(os.path.join(cwd, "toyb_l5_origins.npy"), origins)
    np.save(os.path.join(cwd, "toyb_l5_gt_grid.npy"), gts_b)
    np.save(os.path.join(cwd, "toyb_l5_dist.npy"), dists)            # only the [Recon] line reads the distances
    cloud_a, cloud_b = cloud_of(gts, origins), cloud_of(gts_b, origins)
    write_cloud_ply(os.path.join(cwd, "cloud_b.ply"), cloud_b)
    run([CLI, "train", "toy.ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = ["--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt", "--thh", "0.5",
           "--lossless_lod"] + COMMON
    out = {"cwd": cwd, "cloud_a": cloud_a, "cloud_b": cloud_b, "gts_b": moved, "origins": origins.astype(np.int64)}
    run([CLI, "encode", "toy.ply", "--pack_fn", "a.pk"] + enc, cwd)
    run([CLI, "decode", "a.pk", "--batchsize", "7", "--N", str(N_BLOCKS), "--lossless_lod", "0"] + COMMON, cwd)
    shutil.copy(os.path.join(cwd, "rc_dec.ply"), os.path.join(cwd, "a_dec.ply"))
    for name, flags in (("b_inter", INTER), ("b_again", INTER), ("b_mv", INTER + ["--lossless_mv", "2"])):
        out[name] = run([CLI, "encode", "toyb.ply", "--pack_fn", name + ".pk"] + enc + flags, cwd)
    return out


def test_the_new_pack_has_one_more_key_and_the_vectors_of_the_numpy_search(coded):
    from nvfpcc_amd import lossless_inter_pack as lp, lossless_mv_pack as mp
    cwd = coded["cwd"]
    inter, mv = load(cwd, "b_inter.pk"), load(cwd, "b_mv.pk")
    assert list(inter) == ['net_weight_pack', 'origins', 'latent_pack', 'lossless_lod_pack']
    assert list(mv) == list(inter) + ['lossless_mv_pack'] and isinstance(mv['lossless_mv_pack'], bytes)
    vectors, side, plain = mv.pop('lossless_mv_pack'), mv.pop('lossless_lod_pack'), inter.pop('lossless_lod_pack')
    assert same(inter, mv), "the packs differ beyond the two lossless keys"
    want_mv, want_cost = M.search(coded["gts_b"], coded["cloud_a"], coded["origins"], 2)
    assert want_mv[0::3].tolist() == [[0, 2, -1]] * 8 and want_mv[1::3].tolist() == [[-2, 0, 1]] * 8 and not want_mv[2::3].any()
    info = mp.read(vectors, N_BLOCKS)
    assert info["radius"] == 2 and np.array_equal(info["mv"], want_mv) and len(vectors) == mp.size(N_BLOCKS, 16) == 57
    # the version-4 pack is over R': its digest is that of the reference fetched under the vectors
    assert side[0] == plain[0] == 4 and lp.module_of(side) is lp
    comp = M.compensated(coded["cloud_a"], coded["origins"], want_mv)
    assert lp.read(side, N_BLOCKS)["digest"] == lp.digest(I.H.words_of(comp))
    assert lp.read(plain, N_BLOCKS)["digest"] == lp.digest(I.H.words_of(I.reference_words(coded["cloud_a"], coded["origins"])[0]))
    print("inter: %d bytes; with --lossless_mv 2: %d + %d bytes" % (len(plain), len(side), len(vectors)))
    assert len(side) + len(vectors) < len(plain)
    m, m_plain = lod_line(coded["b_mv"]), lod_line(coded["b_inter"])
    assert int(m.group(1)) == len(side) and int(m_plain.group(1)) == len(plain) and m.group(5) == m_plain.group(5)
    assert "[LosslessLoD] motion: radius 2 moved: 16 of %d blocks bytes: 57" % N_BLOCKS in coded["b_mv"]
    assert "[LosslessLoD] motion" not in coded["b_inter"]
    gross = lambda s: float(re.search(r"Gross bpp: ([0-9.]+)$", s, re.M).group(1))
    n = len(coded["cloud_b"])
    assert abs((gross(coded["b_inter"]) - gross(coded["b_mv"])) - 8 * (len(plain) - len(side) - len(vectors)) / n) < 2e-4
    strip = lambda s: [ln for ln in s.splitlines() if ln.startswith("[") and not ln.startswith("[LosslessLoD]") and "Gross bpp" not in ln]
    assert strip(coded["b_mv"]) == strip(coded["b_inter"])


def test_without_the_flag_the_encode_writes_what_it_wrote(coded):
    """The recipe of tests/test_gpu_lossless_inter_cli.py's b_inter.pk: the same four keys, version 4 over the plain
    reference words, the same lines, and every entry the same bytes from one run to the next (the pickle around them
    is not compared: it may differ where the entries do not)."""
    cwd = coded["cwd"]
    first, again = load(cwd, "b_inter.pk"), load(cwd, "b_again.pk")
    assert list(first) == ['net_weight_pack', 'origins', 'latent_pack', 'lossless_lod_pack'] and same(first, again)
    assert isinstance(first['lossless_lod_pack'], bytes) and first['lossless_lod_pack'] == again['lossless_lod_pack']
    assert "[LosslessLoD] reference: a_dec.ply points: %d dropped: 0" % len(coded["cloud_a"]) in coded["b_inter"]
    drop = lambda s: [ln for ln in s.splitlines() if ln.startswith("[")]
    assert drop(coded["b_inter"]) == drop(coded["b_again"])


@pytest.mark.parametrize("level", [0, 1, 2])
def test_decode_needs_no_new_flag_and_writes_exactly_frame_b_at_the_level(coded, level):
    cwd = coded["cwd"]
    out = run([CLI, "decode", "b_mv.pk", "--batchsize", "7" if level == 1 else "1", "--N", str(N_BLOCKS), "--lossless_lod",
               str(level), "--lossless_ref", "a_dec.ply", "--ref_ply", "cloud_b.ply"] + COMMON, cwd)
    dec = read(cwd, "rc_dec.ply")
    want = rows(coded["cloud_b"] >> level)
    assert dec.shape == want.shape and np.array_equal(rows(dec), want)
    if level == 0:
        assert np.array_equal(dec, coded["cloud_b"])                             # in (block, raster) order
    assert "[LosslessLoD] level: %d points: %d" % (level, len(dec)) in out
    assert "[LosslessLoD] motion: radius 2 moved: 16 of %d blocks bytes: 57" % N_BLOCKS in out
    assert re.search(r"^\[PCError\] D1 PSNR: inf D2 PSNR: \S+$", out, re.M), out[-2000:]


DECODE = [CLI, "decode", "b_mv.pk", "--batchsize", "1", "--N", str(N_BLOCKS), "--lossless_lod", "0"] + COMMON


def test_decode_under_another_reference_or_other_vectors_exits_on_the_digest(coded):
    from nvfpcc_amd import lossless_mv_pack as mp
    cwd = coded["cwd"]
    out = run(DECODE + ["--lossless_ref", "cloud_b.ply"], cwd, ok=False)
    assert "decode --lossless_lod 0: lossless_lod_pack: the reference is not the one the pack was coded under" in out
    assert "Traceback" not in out
    pack = load(cwd, "b_mv.pk")
    mv = mp.read(pack["lossless_mv_pack"], N_BLOCKS)["mv"]
    mv[0] = (0, 2, 0)                                                            # one block fetched one voxel off
    pack["lossless_mv_pack"] = mp.write(2, mv)
    with open(os.path.join(cwd, "b_off.pk"), "wb") as f:
        pickle.dump(pack, f)
    out = run([CLI, "decode", "b_off.pk"] + DECODE[3:] + ["--lossless_ref", "a_dec.ply"], cwd, ok=False)
    assert "the reference is not the one the pack was coded under" in out and "Traceback" not in out
    out = run(DECODE, cwd, ok=False)
    assert "name that cloud with --lossless_ref" in out


def test_vectors_beside_a_pack_that_refers_to_no_cloud_are_refused(coded):
    cwd = coded["cwd"]
    pack = load(cwd, "b_mv.pk")
    pack["lossless_lod_pack"] = load(cwd, "a.pk")["lossless_lod_pack"]           # version 1: coded under no reference
    assert pack["lossless_lod_pack"][0] == 1
    with open(os.path.join(cwd, "b_mixed.pk"), "wb") as f:
        pickle.dump(pack, f)
    out = run([CLI, "decode", "b_mixed.pk"] + DECODE[3:] + ["--lossless_ref", "a_dec.ply"], cwd, ok=False)
    assert "carries a lossless_mv_pack" in out and "is not version 4" in out and "Traceback" not in out


def test_the_refusals_of_the_flag_write_no_pack(coded):
    cwd = coded["cwd"]
    enc = [CLI, "encode", "toyb.ply", "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt",
           "--pack_fn", "never.pk", "--lossless_lod"] + COMMON
    out = run(enc + INTER + ["--lossless_mv", "9"], cwd, ok=False)
    assert "--lossless_mv 9: the search radius is 1..8" in out
    out = run(enc + ["--lossless_ctx", "nbr", "--lossless_mv", "2"], cwd, ok=False)
    assert "--lossless_mv 2 moves the reference of --lossless_ctx inter" in out
    assert not os.path.exists(os.path.join(cwd, "never.pk"))
