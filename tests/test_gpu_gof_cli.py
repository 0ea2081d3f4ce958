"""A group of frames through the command line: train --gof 3 on three tiny synthetic frames, encode them into one pack,
decode one frame or all.  One training run serves every test of the file-based route.  The centre: a frame inside a group
is coded by the same code, to the same bytes, as that frame coded alone under the same weights."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_lod_cli import CLI, COMMON, ROOT, read, run, same

pytestmark = pytest.mark.gpu
START, F, BLOCKS = 7, 3, 8
TRAIN = ["--checkpoint_dir", "ckpts", "--lambda", "200", "--lr", "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5",
         "--shuffle", "True"] + COMMON
GOF = ["--gof", str(F), "--frame_start", str(START)]
DEC = ["--batchsize", "1", "--thh", "0.5"] + COMMON


def load(cwd, name):
    with open(os.path.join(cwd, name), "rb") as f:
        return pickle.load(f)


def raw(cwd, name):
    with open(os.path.join(cwd, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """three frames -> train --gof 3 -> quantise -> encode --gof 3 --thh 0.5 --lossless, in one directory."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd.synth import make_origins, write_dataset
    cwd = str(tmp_path_factory.mktemp("gof_cli"))
    clouds, points = [], []
    for k in range(F):
        gts, _ = write_dataset(os.path.join(cwd, "toy_%04d" % (START + k)), BLOCKS, base_seed=20221 + 1000 * k)
        nz = np.argwhere(gts.reshape(BLOCKS, 32, 32, 32))
        clouds.append(nz[:, 1:] + make_origins(BLOCKS).astype(np.int64)[nz[:, 0]])      # the frame's voxels, (block, raster) order
        points.append(int(gts.astype(bool).sum()))
    out_train = run([CLI, "train", "toy_%04d.ply"] + GOF + ["--epochs", "11", "--phase_change", "5", "--batchsize", "8"] + TRAIN, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = ["--batchsize", "5", "--load_weights", "q4.ckpt", "--thh", "0.5", "--lossless"] + COMMON
    out_enc = run([CLI, "encode", "toy_%04d.ply"] + GOF + ["--load_emb", "ckpts/0010_emb.ckpt", "--pack_fn", "gof.pk"] + enc, cwd)
    return {"cwd": cwd, "clouds": clouds, "points": points, "out_train": out_train, "out_enc": out_enc, "enc": enc}


def test_training_saw_the_group(coded):
    assert re.search(r"^\[data\] 24 leaf blocks, %d points$" % sum(coded["points"]), coded["out_train"], re.M), coded["out_train"][:2000]
    assert coded["out_train"].count("[data]") == 1
    emb = torch.load(os.path.join(coded["cwd"], "ckpts", "0010_emb.ckpt"), map_location="cpu")
    assert tuple(emb.shape) == (F * BLOCKS, 3, 2, 2, 2)
    assert len(set(coded["points"])) == F, "the three frames differ"


def test_pack_layout(coded):
    from nvfpcc_amd import gof
    pack = load(coded["cwd"], "gof.pk")
    assert list(pack) == ["net_weight_pack", "gof_pack", "frames"]
    assert gof.read_gof_pack(pack["gof_pack"]) == {"start": START, "n_leaf": [BLOCKS] * F, "n_points": coded["points"]}
    assert len(pack["frames"]) == F
    for f in pack["frames"]:
        assert list(f) == ["origins", "latent_pack", "lossless_pack"]


def test_a_frame_in_a_group_is_the_frame_alone(coded):
    from nvfpcc_amd import gof
    cwd = coded["cwd"]
    emb = torch.load(os.path.join(cwd, "ckpts", "0010_emb.ckpt"), map_location="cpu")
    torch.save(emb[8:16].clone(), os.path.join(cwd, "emb_0008.ckpt"))
    in_group = raw(cwd, "rc_enc_0008.ply")
    out = run([CLI, "encode", "toy_0008.ply", "--load_emb", "emb_0008.ckpt", "--pack_fn", "alone.pk"] + coded["enc"], cwd)
    assert same(load(cwd, "alone.pk"), gof.extract(load(cwd, "gof.pk"), 1)), "the frame's pack differs from the frame coded alone"
    assert raw(cwd, "rc_enc.ply") == in_group and raw(cwd, "rc_enc_0008.ply") == in_group
    # and its lines are the frame's lines inside the group, but for the Gross bpp line, which is the group's
    lines = coded["out_enc"].splitlines()
    lo = lines.index(next(ln for ln in lines if ln.startswith("[Frame 0008]")))
    hi = lines.index(next(ln for ln in lines if ln.startswith("[Frame 0009]")))
    alone = [ln for ln in out.splitlines() if "Gross bpp" not in ln]
    alone = alone[alone.index(next(ln for ln in alone if ln.startswith("Estimated bit rate"))):]
    assert lines[lo + 1:hi] == alone, (lines[lo + 1:hi], alone)


def damaged_copy(coded):
    """gof.pk with one byte flipped in frame 0's latent stream and one near the end of frame 2's lossless_pack."""
    cwd = coded["cwd"]
    pack = load(cwd, "gof.pk")
    f0, f2 = dict(pack["frames"][0]), dict(pack["frames"][2])
    stream = bytearray(f0["latent_pack"]["latent_byte_stream"])
    stream[len(stream) // 2] ^= 0x10
    f0["latent_pack"] = dict(f0["latent_pack"], latent_byte_stream=type(f0["latent_pack"]["latent_byte_stream"])(stream))
    side = bytearray(f2["lossless_pack"])
    side[-2] ^= 0x40
    f2["lossless_pack"] = bytes(side)
    with open(os.path.join(cwd, "damaged.pk"), "wb") as f:
        pickle.dump(dict(pack, frames=[f0, pack["frames"][1], f2]), f)


def test_random_access(coded):
    cwd = coded["cwd"]
    want = raw(cwd, "rc_enc_0008.ply")
    run([CLI, "decode", "gof.pk", "--frame", "8"] + DEC, cwd)
    assert raw(cwd, "rc_dec.ply") == want
    os.remove(os.path.join(cwd, "rc_dec.ply"))
    damaged_copy(coded)
    # frame 8 is reached without touching the damaged frames on either side of it; --N means nothing to a group
    run([CLI, "decode", "damaged.pk", "--frame", "8", "--N", "3"] + DEC, cwd)
    assert raw(cwd, "rc_dec.ply") == want
    out = run([CLI, "decode", "damaged.pk", "--frame", "8", "--lossless"] + DEC, cwd)
    dec = read(cwd, "rc_dec.ply")
    assert dec.shape == coded["clouds"][1].shape and np.array_equal(dec, coded["clouds"][1])
    assert "[Lossless] points: %d" % coded["points"][1] in out
    out = run([CLI, "decode", "damaged.pk", "--frame", "9", "--lossless"] + DEC, cwd, ok=False)
    assert "frame 0009" in out and "damaged" in out and "Traceback" not in out
    # all frames of the damaged copy: the exit status says so, the frame is named, frame 8 is written all the same
    os.makedirs(os.path.join(cwd, "all_damaged"))
    out = run([CLI, "decode", "../damaged.pk", "--lossless"] + DEC, os.path.join(cwd, "all_damaged"), ok=False)
    assert "frame 0009" in out and "Traceback" not in out
    assert np.array_equal(read(os.path.join(cwd, "all_damaged"), "rc_dec_0008.ply"), coded["clouds"][1])


def test_all_frames(coded):
    """decode without --frame: every frame into rc_dec_%04d.ply, each equal to its rc_enc_%04d.ply, and the three not
    all equal to each other.  The last is asked of the --lossless decode, where this fixture can show it: after 11 epochs
    the latents of all 24 blocks still round to the same symbols (measured on one MI355X: the three frames' 45-byte
    latent streams are byte-identical, and so are the plain encoder's rc_enc.ply of toy_0007 and toy_0008 coded alone:
    17 616 points each), so the three lossy clouds are one and the same file whatever code decodes them.  What does
    distinguish the frames is their occupancy: decoded --lossless, each file holds exactly its own frame's voxels."""
    cwd = coded["cwd"]
    run([CLI, "decode", "gof.pk"] + DEC, cwd)
    got = [raw(cwd, "rc_dec_%04d.ply" % (START + k)) for k in range(F)]
    assert got == [raw(cwd, "rc_enc_%04d.ply" % (START + k)) for k in range(F)]
    assert all(len(g) > 200 for g in got)
    out = run([CLI, "decode", "gof.pk", "--lossless"] + DEC, cwd)
    exact = [read(cwd, "rc_dec_%04d.ply" % (START + k)) for k in range(F)]
    for k in range(F):
        assert exact[k].shape == coded["clouds"][k].shape and np.array_equal(exact[k], coded["clouds"][k]), k
    assert len({e.tobytes() for e in exact}) == F, "the three frames are not all equal to each other"
    assert [int(n) for n in re.findall(r"^\[Lossless\] points: (\d+)$", out, re.M)] == coded["points"]


def test_accounting(coded):
    from nvfpcc_amd import gof
    pack, out = load(coded["cwd"], "gof.pk"), coded["out_enc"]
    points = coded["points"]
    w = 8 * len(pack["net_weight_pack"]["bit_stream"])
    lat = [8 * len(f["latent_pack"]["latent_byte_stream"]) for f in pack["frames"]]
    side = [8 * len(f["lossless_pack"]) for f in pack["frames"]]
    g = 8 * len(pack["gof_pack"])
    assert g == 8 * (7 + 8 * F)
    gross = re.findall(r"^\[Latent code\] Gross bpp: ([0-9.]+)$", out, re.M)
    assert len(gross) == 1 and out.rstrip().splitlines()[-1].startswith("[Latent code] Gross bpp")
    exact = (w + sum(lat) + sum(side) + g) / float(sum(points))
    assert abs(float(gross[0]) - exact) <= 5.0001e-5, (gross, exact)
    assert "[GoF] frames: %d points: %d weight bytes: %d latent bytes: %d side bytes: %d" % (
        F, sum(points), w // 8, sum(lat) // 8, sum(side) // 8) in out
    frames = re.findall(r"^\[Frame (\d{4})\] points: (\d+) blocks: (\d+) latent bytes: (\d+) side bytes: (\d+) own bpp: ([0-9.]+)$", out, re.M)
    assert [(int(a), int(b), int(c), int(d), int(e)) for a, b, c, d, e, _ in frames] == [
        (START + k, points[k], BLOCKS, lat[k] // 8, side[k] // 8) for k in range(F)]
    own = [float(f[5]) for f in frames]
    for k in range(F):
        assert abs(own[k] - (lat[k] + side[k]) / float(points[k])) <= 5.0001e-5
    # weighted by points, the frames' own bpp are the total without the weights and gof_pack (each printed to 5e-5)
    total = sum(o * n for o, n in zip(own, points))
    assert abs(total - (exact * sum(points) - w - g)) <= 5.0001e-5 * sum(points)
    assert abs(total - (float(gross[0]) * sum(points) - w - g)) <= 2 * 5.0001e-5 * sum(points)
    assert gof.gof_lines(pack) == out.rstrip().splitlines()[-2:]
    for k in range(F):      # each frame's own lines follow its [Frame] line
        assert out.count("[Lossless] bytes: %d " % (side[k] // 8)) >= 1
    assert out.count("[Recon]") == F and out.count("Start to reconstruct") == F


def test_refusals_exit_with_their_message(coded):
    cwd = coded["cwd"]
    if not os.path.exists(os.path.join(cwd, "alone.pk")):
        run([CLI, "encode", "toy_0008.ply", "--load_emb", "ckpts/0010_emb.ckpt", "--pack_fn", "alone.pk", "--batchsize", "5",
             "--load_weights", "q4.ckpt", "--thh", "0.5"] + COMMON, cwd)
    out = run([CLI, "decode", "alone.pk", "--frame", "8", "--N", str(BLOCKS)] + DEC, cwd, ok=False)
    assert "carries no gof_pack" in out and "--frame 8" in out and "Traceback" not in out
    out = run([CLI, "decode", "gof.pk", "--frame", "10"] + DEC, cwd, ok=False)
    assert "--frame 10" in out and "7 .. 9" in out and "Traceback" not in out
    pack = load(cwd, "gof.pk")
    with open(os.path.join(cwd, "badgof.pk"), "wb") as f:
        pickle.dump(dict(pack, gof_pack=pack["gof_pack"][:-1]), f)
    out = run([CLI, "decode", "badgof.pk", "--frame", "8"] + DEC, cwd, ok=False)
    assert "gof_pack" in out and "bytes" in out and "Traceback" not in out
    enc = ["--load_emb", "ckpts/0010_emb.ckpt", "--pack_fn", "never.pk"] + coded["enc"]
    out = run([CLI, "encode", "toy.ply"] + GOF + enc, cwd, ok=False)
    assert "toy.ply" in out and "no frame pattern" in out and "Traceback" not in out
    # ... and when toy_0009's files are absent
    moved = [os.path.join(cwd, "toy_0009_l5_%s.npy" % k) for k in ("origins", "gt_grid", "dist")]
    for fn in moved:
        os.replace(fn, fn + ".away")
    try:
        out = run([CLI, "encode", "toy_%04d.ply"] + GOF + enc, cwd, ok=False)
    finally:
        for fn in moved:
            os.replace(fn + ".away", fn)
    assert "toy_0009_l5_origins.npy" in out and "Traceback" not in out
    assert not os.path.exists(os.path.join(cwd, "never.pk"))


def test_device_route(tmp_path):
    """--from_ply --gof 2: the clouds themselves, pre-processed on the device; the leaves travel as octree bytes and the
    threshold is chosen per frame, so decode needs neither --N nor --thh."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from nvfpcc_amd import gof, preprocess as pp, thh_select as ts
    from tests.golden_inputs import write_cloud_ply
    from tests.test_gpu_preprocess_deep import shell_patch
    cwd = str(tmp_path)
    clouds = [np.unique(shell_patch((512 + k, 512, 512 - k), 12.0 + k, 3000, 5 + k), axis=0) for k in range(2)]
    for k, pts in enumerate(clouds):
        assert len(pp.octree_partition(pts, 10)[0]) == 8
        write_cloud_ply(os.path.join(cwd, "cloud%d.ply" % (3 + k)), pts)
    flags = ["--from_ply", "--gof", "2", "--frame_start", "3"]
    out = run([CLI, "train", "cloud%d.ply"] + flags + ["--epochs", "1", "--phase_change", "1", "--batchsize", "4"] + TRAIN, cwd)
    assert "[data] 16 leaf blocks, %d points" % sum(len(p) for p in clouds) in out
    assert tuple(torch.load(os.path.join(cwd, "ckpts", "0000_emb.ckpt"), map_location="cpu").shape) == (16, 3, 2, 2, 2)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0000.ckpt", "q4.ckpt", "16"], cwd)
    out = run([CLI, "encode", "cloud%d.ply"] + flags + ["--pack_octree", "--thh_mode", "count", "--batchsize", "5", "--load_weights",
               "q4.ckpt", "--load_emb", "ckpts/0000_emb.ckpt"] + COMMON, cwd)
    pack = load(cwd, "pack.pk")
    assert list(pack) == ["net_weight_pack", "gof_pack", "frames"]
    assert gof.read_gof_pack(pack["gof_pack"]) == {"start": 3, "n_leaf": [8, 8], "n_points": [len(p) for p in clouds]}
    for k, f in enumerate(pack["frames"]):
        assert list(f) == ["latent_pack", "octree_pack", "thh_pack"]
        assert np.array_equal(pp.read_octree_pack(f["octree_pack"]), pp.octree_partition(clouds[k], 10)[0])
        assert ts.read_thh_pack(f["thh_pack"])[0] == "count"
    assert len(clouds[0]) != len(clouds[1])
    run([CLI, "decode", "pack.pk", "--batchsize", "3"] + COMMON, cwd)
    for n in (3, 4):
        assert raw(cwd, "rc_dec_%04d.ply" % n) == raw(cwd, "rc_enc_%04d.ply" % n)
