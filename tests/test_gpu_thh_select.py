"""Threshold selection on the GPU (csrc/occ_select.hip, nvfpcc_amd/thh_select.py, `NVFPCC.py --thh_mode`).

Everything here is integer or bit exact: histograms against numpy.bincount, selection against the sort-based numpy
restatement (tests/thh_select_ref.py), the curve's squared-error rider against nvfpcc_amd.pc_metrics, and the command
line round trip (encode at batch 5, decode at batch 1 with no --thh) for every mode.

The d1 test runs on the trained narrow golden (tests/golden/trained_S_pack.pk): tests/test_thh_select_cpu.py checks
that its shortlist holds at least 3 distinct thresholds inside the 2/3..3/2 window."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import thh_select_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ((21, 11), (10, 11), (0, 10))


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def field(kind, blocks, voxels, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((blocks, voxels), dtype=np.float32)
    if kind == "equal":
        return np.full((blocks, voxels), 0.3125, np.float32)
    assert kind == "saturated"                    # > 90 % exact zeros, a few thousand exact ones per block
    p = np.zeros((blocks, voxels), np.float32)
    u = rng.random((blocks, voxels))
    p[u > 0.92] = 1.0
    mid = u > 0.985
    p[mid] = rng.random(int(mid.sum()), dtype=np.float32)
    p[:, ::97] = np.float32(0.75)                  # a handful of repeated values
    return p


def bincount_rows(p, shift, nbits, prefix, d2, gt):
    k = R.keys(p)
    ok = k <= 0x3F800000
    if prefix is not None and shift + nbits < 32:
        ok &= (k >> (shift + nbits)) == prefix[:, None]
    nb = 1 << nbits
    flat = ((np.arange(p.shape[0])[:, None] * nb) + ((k >> shift) & (nb - 1)))[ok]
    size = p.shape[0] * nb
    count = np.bincount(flat, minlength=size).reshape(-1, nb)
    s = g = None
    if d2 is not None:
        s = np.bincount(flat, weights=d2[ok].astype(np.float64), minlength=size).astype(np.int64).reshape(-1, nb)
    if gt is not None:
        g = np.bincount(flat, weights=(gt[ok] != 0), minlength=size).astype(np.int64).reshape(-1, nb)
    return count, s, g


@pytest.mark.timeout(600)
@pytest.mark.parametrize("blocks,voxels", [(1, 32768), (600, 32768), (3, 1000)])
@pytest.mark.parametrize("kind", ["uniform", "saturated", "equal"])
def test_occ_hist_equals_bincount(kind, blocks, voxels):
    need_gpu()
    from nvfpcc_amd import ops
    p = field(kind, blocks, voxels, seed=blocks)
    rng = np.random.default_rng(7)
    d2 = rng.integers(0, 3 * 1023 ** 2 + 1, p.shape).astype(np.int32)       # sums per bin pass 2^32
    gt = (rng.random(p.shape) < 0.03).astype(np.uint8)
    P, D, G = dev(p), dev(d2), dev(gt)
    for shift, nbits in PASSES:
        pre = (R.keys(p[:, 5]) >> (shift + nbits)).astype(np.int32) if shift + nbits < 32 else np.zeros(blocks, np.int32)
        for prefix in (None, pre):
            for riders in (False, True):
                count, s, g, bad = ops.occ_hist(P, shift, nbits, None if prefix is None else dev(prefix),
                                                d2=D if riders else None, gt=G if riders else None)
                wc, ws, wg = bincount_rows(p, shift, nbits, None if prefix is None else prefix.astype(np.int64),
                                           d2 if riders else None, gt if riders else None)
                tag = (kind, blocks, shift, prefix is not None, riders)
                assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), wc), tag
                assert int(bad.sum()) == 0
                if riders:
                    assert s.dtype == torch.int64 and np.array_equal(s.cpu().numpy(), ws), tag
                    assert np.array_equal(g.cpu().numpy(), wg), tag
                else:
                    assert s is None and g is None
                if prefix is None:
                    assert int(count.sum()) == p.size


@pytest.mark.timeout(300)
def test_occ_hist_counts_bad_keys_and_select_raises():
    need_gpu()
    from nvfpcc_amd import ops, thh_select as ts
    p = field("uniform", 4, 32768, seed=11)
    p[1, 17], p[1, 40000 % 32768], p[3, 5], p[3, 6] = np.nan, 2.0, -1.0, np.inf
    p[0, 3] = -0.0                                     # folded onto +0.0, not an error
    count, _, _, bad = ops.occ_hist(dev(p), 21, 11)
    assert bad.tolist() == [0, 2, 0, 2] and int(count.sum()) == p.size - 4 and int(count[0, 0]) >= 1
    with pytest.raises(ValueError, match="outside"):
        ts.kth_largest(dev(p), 10)
    with pytest.raises(ValueError, match="outside"):
        ts.curve(dev(p), None, None, [0.5])


def tie_field(blocks=6, voxels=32768, seed=2):
    """Uniform values with a constructed tie: 0.5 exactly, 40 times per block, and nothing else in (0.49, 0.51)."""
    rng = np.random.default_rng(seed)
    p = rng.random((blocks, voxels), dtype=np.float32)
    p[(p > 0.49) & (p < 0.51)] = 0.25
    for b in range(blocks):
        p[b, rng.choice(voxels, 40, replace=False)] = 0.5
    return p


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", ["tie", "saturated", "equal"])
def test_select_equals_the_numpy_restatement(kind):
    need_gpu()
    from nvfpcc_amd import thh_select as ts
    p = tie_field() if kind == "tie" else field(kind, 6, 32768, seed=4)
    P = dev(p)
    B, V = p.shape
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    # per block: k in {0, 1, a tie boundary, voxels - 1, voxels, beyond}
    above = (p > 0.5).sum(1)
    for ks in ([0] * B, [1] * B, list(above + 1), list(above + 20), list(above + 40), [V - 1] * B, [V] * B, [V + 9] * B,
               [0, 1, int(above[2]) + 3, V - 1, V, V + 1]):
        k = torch.tensor([int(x) for x in ks])
        v, t = ts.kth_largest(P, k.cuda()).cpu().numpy(), ts.threshold_for_count(P, k.cuda()).cpu().numpy()
        assert np.array_equal(bits(v), bits(R.kth_largest_blocks(p, ks))), ks
        assert np.array_equal(bits(t), bits(R.threshold_for_count_blocks(p, ks))), ks
    if kind == "tie":
        k = torch.tensor([int(x) + 7 for x in above]).cuda()          # inside the tie: all 40 are kept
        t = ts.threshold_for_count(P, k).cpu().numpy()
        sel = (p > t[:, None]).sum(1)
        assert np.array_equal(sel, above + 40) and np.all(sel > k.cpu().numpy())
    # whole cloud
    n_above = int(above.sum())
    for k in (0, 1, n_above + 1, n_above + 100, n_above + 40 * B, p.size - 1, p.size, p.size + 3):
        v, t = ts.kth_largest(P, k), ts.threshold_for_count(P, k)
        assert v.dim() == 0 and bits(v.item()) == bits(R.kth_largest(p, k)), k
        assert bits(t.item()) == bits(R.threshold_for_count(p, k)), k
    if kind == "tie":
        t = ts.threshold_for_count(P, n_above + 100).item()
        assert int((p > np.float32(t)).sum()) == n_above + 40 * B


@pytest.mark.timeout(300)
def test_threshold_points_per_block_and_scalar():
    need_gpu()
    from nvfpcc_amd import ops
    from nvfpcc_amd._lib import lib
    rng = np.random.default_rng(9)
    B, D = 7, 32
    p = rng.random((B, 1, D, D, D), dtype=np.float32)
    thh = np.array([0.5, 0.99, 0.0, 1.0, -1e-45, 0.9999, 0.123], np.float32)
    origins = rng.integers(0, 31, (B, 3)).astype(np.int32) * 32
    P = dev(p)
    pts, counts = ops.threshold_points(P, dev(thh), dev(origins))
    want = [torch.nonzero(P[b, 0] > float(thh[b])).cpu().numpy() + origins[b] for b in range(B)]
    assert counts.tolist() == [w.shape[0] for w in want] and counts[3] == 0 and counts[4] == D ** 3
    assert pts.dtype == torch.int32 and np.array_equal(pts.cpu().numpy(), np.concatenate(want))
    # a float keeps the scalar kernels: the same bits as the scalar entry points called directly
    st = torch.cuda.current_stream().cuda_stream
    for t in (0.64, 0.5):
        got, gc = ops.threshold_points(P, t, dev(origins))
        c = torch.empty(B, dtype=torch.int32, device="cuda")
        assert lib().nvf_threshold_count(P.data_ptr(), t, c.data_ptr(), B, D ** 3, st) == 0
        off = (torch.cumsum(c, 0, dtype=torch.int32) - c).contiguous()
        out = torch.empty((int(c.sum()), 3), dtype=torch.int32, device="cuda")
        assert lib().nvf_threshold_compact(P.data_ptr(), t, off.data_ptr(), dev(origins).data_ptr(), out.data_ptr(), B, D,
                                           st) == 0
        assert torch.equal(gc, c) and torch.equal(got, out)
        # and one threshold repeated per block gives the same points
        same, sc = ops.threshold_points(P, torch.full((B,), t, device="cuda"), dev(origins))
        assert torch.equal(same, got) and torch.equal(sc, gc)
    with pytest.raises(RuntimeError):
        ops.threshold_points(P, torch.zeros(B + 1, device="cuda"))


# ---------------------------------------------------------------- the trained narrow golden (12 blocks)
@pytest.fixture(scope="module")
def golden():
    """Probabilities of the trained narrow decoder on its 12 blocks, the blocks' ground truth, and the exact
    squared-distance grid of the whole cloud (nvf_nearest_dist2 through preprocess.build_grids)."""
    need_gpu()
    from nvfpcc_amd import network, thh_select as ts
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.preprocess import build_grids
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    from tests.test_trained_golden import CFG, load_pack, state_from_pack
    pack, G = load_pack(os.path.join(ROOT, "tests", "golden"), "S")
    ch, channels = CFG["S"]
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", ch, ",".join(str(c) for c in channels), verbose=False)
    net.load_state_dict(state_from_pack(pack), strict=False)
    net = net.to("cuda")
    lat = torch.from_numpy(G["latents"].astype(np.float32)).to("cuda")
    with torch.no_grad():
        p = torch.cat([net.reconstruct(lat[i:i + 5].contiguous(), 2) for i in range(0, lat.shape[0], 5)])
    n = lat.shape[0]
    gt = torch.from_numpy(make_blocks(n)[0]).cuda()
    origins = pack["origins"].astype(np.int64)
    orig = ts.original_points(gt, origins)
    gt2, dist = build_grids(orig, origins)
    assert np.array_equal(gt2, gt.cpu().numpy())
    return {"p": p, "gt": gt, "d2": ts.d2_from_dist(dist).cuda().contiguous(), "origins": origins, "orig": orig,
            "net": net, "lat": lat}


@pytest.mark.timeout(600)
def test_count_modes_on_the_trained_golden(golden):
    from nvfpcc_amd import ops, thh_select as ts
    p, gt = golden["p"], golden["gt"]
    pn = p.cpu().numpy().reshape(p.shape[0], -1)
    K = int(gt.sum())
    sel = ts.choose("count", p, n_points=K)
    vk = R.kth_largest(pn, K)
    pts, counts = ops.threshold_points(p, sel["t"], torch.from_numpy(golden["origins"]))
    assert sel["mode"] == "count" and pts.shape[0] >= K and pts.shape[0] == int((pn >= vk).sum())
    want = np.concatenate([np.argwhere(pn[b].reshape(32, 32, 32) >= vk) + golden["origins"][b] for b in range(pn.shape[0])])
    assert np.array_equal(pts.cpu().numpy(), want)
    kb = gt.reshape(gt.shape[0], -1).long().sum(1)
    selb = ts.choose("block-count", p, block_counts=kb.cpu().numpy())
    assert selb["t"].shape == (p.shape[0],) and selb["t"].dtype == torch.float32
    ptsb, cb = ops.threshold_points(p, selb["t"], torch.from_numpy(golden["origins"]))
    vb = R.kth_largest_blocks(pn, kb.tolist())
    wantb = [np.argwhere(pn[b].reshape(32, 32, 32) >= vb[b]) + golden["origins"][b] for b in range(pn.shape[0])]
    assert cb.tolist() == [w.shape[0] for w in wantb] and all(c >= k for c, k in zip(cb.tolist(), kb.tolist()))
    assert np.array_equal(ptsb.cpu().numpy(), np.concatenate(wantb))
    # the decoder's path: the same thresholds recomputed batch by batch from the counts alone
    from nvfpcc_amd.recon import reconstruct_points
    used = []
    dec, dc = reconstruct_points(golden["net"], golden["lat"], golden["origins"], None, batch=1,
                                 block_counts=kb.cpu().numpy(), thh_out=used)
    assert np.array_equal(dec, ptsb.cpu().numpy()) and torch.equal(torch.cat(used), selb["t"])


@pytest.mark.timeout(600)
def test_curve_ties_to_the_merged_metric(golden):
    from nvfpcc_amd import ops, pc_metrics, thh_select as ts
    p, gt, d2 = golden["p"], golden["gt"], golden["d2"]
    pn = p.cpu().numpy().reshape(-1)
    cands = np.array([0.05, 0.3, 0.5, 0.6, 0.64, 0.65, 0.9], np.float32)
    cur = ts.curve(p, gt, d2, cands)
    ref = R.curve(pn, gt.cpu().numpy(), d2.cpu().numpy(), cands)
    for k in ("count", "tp", "sse"):
        assert cur[k].dtype == np.int64 and cur[k].tolist() == ref[k], k
    assert ts.curve(p, None, d2, cands)["tp"] is None and ts.curve(p, gt, None, cands)["sse"] is None
    for i in (1, 4):
        dec, _ = ops.threshold_points(p, float(cands[i]), torch.from_numpy(golden["origins"]))
        dec = dec.cpu().numpy()
        back = pc_metrics.nearest(dec, golden["orig"])[1]
        assert back.dtype == np.int64 and int(back.sum()) == int(cur["sse"][i]) and dec.shape[0] == int(cur["count"][i])
        r = pc_metrics.geometry_psnr(golden["orig"], dec, d2=False)
        assert r["test_to_ref"]["d1_mse"] == int(cur["sse"][i]) / int(cur["count"][i])


@pytest.mark.timeout(900)
def test_d1_mode_picks_the_best_of_its_shortlist(golden):
    from nvfpcc_amd import ops, pc_metrics, thh_select as ts
    p = golden["p"]
    K = int(golden["gt"].sum())
    sel = ts.choose("d1", p, origins=golden["origins"], n_points=K, gt=golden["gt"], d2=golden["d2"])
    assert sel["mode"] == "d1" and sel["note"] is None
    cands = sel["candidates"]
    assert len(set(c["t"] for c in cands)) >= 3, "the shortlist must hold at least 3 distinct thresholds"
    psnr = {}
    for c in cands:
        dec, _ = ops.threshold_points(p, c["t"], torch.from_numpy(golden["origins"]))
        assert dec.shape[0] == c["count"] and 2 / 3 * K <= c["count"] <= 3 / 2 * K
        psnr[c["t"]] = pc_metrics.geometry_psnr(golden["orig"], dec.cpu().numpy(), d2=False)["d1_psnr"]
        assert psnr[c["t"]] == c["psnr"]
    print("d1 shortlist (t, count, PSNR):", [(c["t"], c["count"], round(c["psnr"], 4)) for c in cands], "chosen", sel["t"])
    assert psnr[sel["t"]] == max(psnr.values())
    tied = [c for c in cands if c["psnr"] == psnr[sel["t"]]]
    assert abs([c for c in tied if c["t"] == sel["t"]][0]["count"] - K) == min(abs(c["count"] - K) for c in tied)


# ---------------------------------------------------------------- command line round trips on a toy dataset
COMMON = ["--chanstr", "8,16,8,8", "--ch", "3"]
N_TOY = 24


def run(cmd, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert (r.returncode == 0) == ok, r.stdout[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """tests/test_gpu_cli.py's recipe: synth.write_dataset, 11 epochs, manipulate_weights; then a plain encode."""
    need_gpu()
    from nvfpcc_amd.synth import write_dataset
    cwd = str(tmp_path_factory.mktemp("toy"))
    gts, _ = write_dataset(os.path.join(cwd, "toy"), N_TOY)
    cli = os.path.join(ROOT, "NVFPCC.py")
    run([cli, "train", "toy.ply", "--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + COMMON, cwd)
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], cwd)
    enc = run(encode_cmd("plain.pk", ["--thh", "0.5"]), cwd)
    os.replace(os.path.join(cwd, "rc_enc.ply"), os.path.join(cwd, "plain_enc.ply"))
    return {"cwd": cwd, "cli": cli, "n_points": int(gts.sum()), "kb": gts.reshape(N_TOY, -1).sum(1), "plain_out": enc}


def encode_cmd(pack, extra):
    return [os.path.join(ROOT, "NVFPCC.py"), "encode", "toy.ply", "--batchsize", "5", "--load_weights", "q4.ckpt",
            "--load_emb", "ckpts/0010_emb.ckpt", "--pack_fn", pack] + extra + COMMON


def decode_cmd(pack, extra):
    return [os.path.join(ROOT, "NVFPCC.py"), "decode", pack, "--batchsize", "1", "--N", str(N_TOY)] + extra + COMMON


def field_of(out, head):
    lines = [ln for ln in out.splitlines() if ln.startswith(head)]
    assert len(lines) == 1, (head, out[-2000:])
    return lines[0]


def pack_bits(pack):
    return 8 * len(pack["latent_pack"]["latent_byte_stream"]) + 8 * len(pack["net_weight_pack"]["bit_stream"])


@pytest.mark.timeout(900)
def test_cli_without_thh_mode_is_unchanged(toy):
    """No --thh_mode: today's three pack keys, no [Threshold] line, and the PLYs the scalar entry points give."""
    from nvfpcc_amd import network
    from nvfpcc_amd._lib import lib
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.recon import read_ply_ascii
    from nvfpcc_amd import latent_codec
    from tests.test_trained_golden import state_from_pack
    cwd = toy["cwd"]
    out = run(decode_cmd("plain.pk", ["--thh", "0.5"]), cwd)
    assert "[Threshold]" not in out and "[Threshold]" not in toy["plain_out"]
    with open(os.path.join(cwd, "plain.pk"), "rb") as f:
        pack = pickle.load(f)
    assert list(pack) == ["net_weight_pack", "origins", "latent_pack"]
    assert field_of(toy["plain_out"], "[Latent code] Gross bpp") == \
        "[Latent code] Gross bpp: %.4f" % (pack_bits(pack) / toy["n_points"])
    enc, dec = read_ply_ascii(os.path.join(cwd, "plain_enc.ply")), read_ply_ascii(os.path.join(cwd, "rc_dec.ply"))
    assert enc.shape[0] > 0 and np.array_equal(enc, dec)
    # the parent's recipe, by hand: decode()'s network, nvf_threshold_count / nvf_threshold_compact at --thh
    network.reset_seed()
    net = Net(None, "Gaussian", 3, "8,16,8,8", verbose=False)
    net.load_state_dict(state_from_pack(pack), strict=False)
    net = net.to("cuda")
    lat = latent_codec.arithmetic_dec(pack["latent_pack"]).to("cuda")
    st = torch.cuda.current_stream().cuda_stream
    want = []
    with torch.no_grad():
        for b in range(N_TOY):
            p = net.reconstruct(lat[b:b + 1].contiguous(), 2)
            c = torch.empty(1, dtype=torch.int32, device="cuda")
            assert lib().nvf_threshold_count(p.data_ptr(), 0.5, c.data_ptr(), 1, 32768, st) == 0
            o = torch.empty((max(int(c), 1), 3), dtype=torch.int32, device="cuda")
            org = torch.from_numpy(pack["origins"][b:b + 1].astype(np.int32)).cuda()
            assert lib().nvf_threshold_compact(p.data_ptr(), 0.5, torch.zeros(1, dtype=torch.int32, device="cuda").data_ptr(),
                                               org.data_ptr(), o.data_ptr(), 1, 32, st) == 0
            want.append(o[:int(c)].cpu().numpy())
    assert np.array_equal(dec.astype(np.int64), np.concatenate(want))
    # a mode asked of a pack that carries none is an error that says so
    msg = run(decode_cmd("plain.pk", ["--thh_mode", "count"]), cwd, ok=False)
    assert "carries no thh_pack" in msg


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["count", "block-count", "d1"])
def test_cli_round_trip_carries_the_threshold(toy, mode):
    from nvfpcc_amd import thh_select as ts
    from nvfpcc_amd.recon import read_ply_ascii
    cwd = toy["cwd"]
    pk = f"pack_{mode}.pk"
    e = run(encode_cmd(pk, ["--thh_mode", mode]), cwd)
    d = run(decode_cmd(pk, []), cwd)                                   # no --thh: the pack carries it
    with open(os.path.join(cwd, pk), "rb") as f:
        pack = pickle.load(f)
    with open(os.path.join(cwd, "plain.pk"), "rb") as f:
        plain = pickle.load(f)
    assert list(pack) == ["net_weight_pack", "origins", "latent_pack", "thh_pack"]
    assert pack["latent_pack"]["latent_byte_stream"] == plain["latent_pack"]["latent_byte_stream"]
    enc, dec = read_ply_ascii(os.path.join(cwd, "rc_enc.ply")), read_ply_ascii(os.path.join(cwd, "rc_dec.ply"))
    assert enc.shape[0] > 0 and enc.shape == dec.shape and np.array_equal(enc, dec)
    le, ld = field_of(e, "[Threshold] mode"), field_of(d, "[Threshold] mode")
    print(mode, le, field_of(e, "[Latent code] Gross bpp"), field_of(e, "[Recon]"))
    assert le == ld
    got_mode, value = ts.read_thh_pack(pack["thh_pack"])
    side = 8 * len(pack["thh_pack"])
    if mode == "block-count":
        assert got_mode == mode and value.tolist() == toy["kb"].tolist() and side == 8 + 16 * N_TOY
    else:
        assert got_mode in (mode, "count") and side == 40               # d1 may say it fell back to count
        assert got_mode == mode or "using count" in e
        assert f"mode: {got_mode} t: %.9g" % np.float32(value) in le
    if mode == "count":
        assert enc.shape[0] >= toy["n_points"]
    assert field_of(e, "[Latent code] Gross bpp") == "[Latent code] Gross bpp: %.4f" % ((pack_bits(pack) + side) / toy["n_points"])
    assert field_of(toy["plain_out"], "[Latent code] Gross bpp") == "[Latent code] Gross bpp: %.4f" % (pack_bits(plain) / toy["n_points"])
    assert pack_bits(pack) == pack_bits(plain)
    # --thh_mode fixed overrides the pack and uses --thh: the plain decode's points
    run(decode_cmd(pk, ["--thh_mode", "fixed", "--thh", "0.5"]), cwd)
    fixed = read_ply_ascii(os.path.join(cwd, "rc_dec.ply"))
    assert np.array_equal(fixed, read_ply_ascii(os.path.join(cwd, "plain_enc.ply")))
