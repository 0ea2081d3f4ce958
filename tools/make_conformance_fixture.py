#!/usr/bin/env python3
"""Generate tests/golden/conformance_{S,W}.npz: what the eval route of THIS build gives for the two committed trained
decoders (tests/golden/trained_{S,W}_pack.pk), written down bit for bit, and every side pack encode writes under it.

The float32 bits of the eval forward are part of the format of lossless_pack, lossless_lod_pack (versions 1 and 3),
lod_pack and thh_pack ("What the side packs fix"): tests/test_conformance_cpu.py and
tests/test_gpu_conformance.py hold every later build to this file.  Run it on the commit whose bits are the format --
never to make a failing test pass; a change that moves the bits on purpose bumps the packs' version bytes first.

    python tools/make_conformance_fixture.py [--out DIR] [--parent HASH]

Needs an MI355X, is deterministic, reads nothing outside the repository; run it twice and compare the files byte for
byte before committing them.  --parent: the commit the library was built from (default: git rev-parse HEAD).

Per tag, the members (tests/conformance_ref.py reads them):
    parent                         the commit hash
    p_sha, cls1_sha, cls0_sha      uint8 [12, 32]: sha256 of each block's p / 16^3 head / 8^3 head, little-endian float32
    p_sample_index, p_sample_bits  every 61st voxel: the raw uint32 patterns [12, 538]; cls1_*, cls0_* likewise
    ctx0, ctx0_blocks              uint8 [n, 32768] the v1 context of every voxel of the blocks ctx0_blocks
    heads/<state-dict key>         float16: the coarse heads the lod forward ran with (seed-derived: the packs carry none)
    lossless_g<G>, lossless_lod_g<G>, lossless_nbr_g<G>     the encoders' bytes at group 64 and 2, batch 5
    lod_pack, lod_k, lod_ties, lod_counts, lod_occ1, lod_occ2       encode --pack_lod: bytes, occupied coarse cells of the
                                   input, head probabilities equal to the k-th largest, kept per block, kept cells (packbits)
    thh_count_pack, thh_count_counts, thh_count_ties                --thh_mode count: bytes, points per block, ties
    thh_block_pack, thh_block_counts, thh_block_ties                --thh_mode block-count, ties per block
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import conformance_ref as C          # noqa: E402
from tests import occ_rans_ref as R             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def record(tag, parent):
    import torch
    from nvfpcc_amd import lod_pack, lossless_lod_pack, lossless_nbr_pack, lossless_pack, thh_select as ts
    from nvfpcc_amd.recon import eval_batches, reconstruct_points
    dev = torch.device("cuda")
    torch.set_grad_enabled(False)
    heads = C.seed_heads(tag)
    net, lat, origins = C.build_decoder(GOLDEN, tag, dev, heads)
    gt = C.ground_truth()
    levels = C.unpack_levels(gt)
    gt_dev = torch.from_numpy(gt.reshape(-1, 1, 32, 32, 32)).float().to(dev)
    out = {"parent": np.array(parent)}
    out.update({"heads/" + k: v for k, v in heads.items()})

    # the field, block by block at batch 1, and the two coarse heads
    p_dev = torch.cat([o for _, _, o in eval_batches(net, lat, 1)], 0)
    p = p_dev.reshape(C.N_BLOCKS, -1).cpu().numpy()
    fields = {"p": p}
    for lod, name in ((1, "cls1"), (2, "cls0")):
        fields[name] = torch.cat([o[1] for _, _, o in eval_batches(net, lat, 1, lod, return_p=True)], 0) \
            .reshape(C.N_BLOCKS, -1).cpu().numpy()
    index = {"p": np.arange(0, C.VOX, C.SAMPLE_STRIDE), **C.HEAD_SAMPLES}
    for name, f in fields.items():
        assert np.isfinite(f).all() and f.min() >= 0 and f.max() <= 1
        out[name + "_sha"] = C.sha_rows(f)
        out[name + "_sample_index"] = index[name].astype(np.int32)
        out[name + "_sample_bits"] = C.bits_of(f[:, index[name]])
    out["ctx0"] = R.contexts(p).astype(np.uint8)
    out["ctx0_blocks"] = np.arange(C.N_BLOCKS, dtype=np.int32)

    # the three occupancy coders
    for name, mod in (("lossless", lossless_pack), ("lossless_lod", lossless_lod_pack), ("lossless_nbr", lossless_nbr_pack)):
        for group in C.GROUPS:
            data, _ = mod.encode_occupancy(net, lat, gt_dev, batch=C.ENCODE_BATCH, group=group)
            out[f"{name}_g{group}"] = np.frombuffer(data, np.uint8)

    # encode --pack_lod
    sel = C.lod_selection(net, lat, origins, levels, C.ENCODE_BATCH)
    sd = net.state_dict()
    out["lod_pack"] = np.frombuffer(lod_pack.write_lod_pack(sel["t"][0], sel["t"][1], *[sd[k] for k in lod_pack.HEAD_KEYS]),
                                    np.uint8)
    out["lod_k"], out["lod_ties"] = np.asarray(sel["k"], np.int64), np.asarray(sel["ties"], np.int64)
    out["lod_counts"] = np.stack(sel["counts"])
    out["lod_occ1"], out["lod_occ2"] = (np.packbits(o, axis=1) for o in sel["occ"])

    # encode --thh_mode count / block-count
    p_all = torch.cat([o for _, _, o in eval_batches(net, lat, C.ENCODE_BATCH)], 0)
    n_points, k_b = int(gt.sum()), gt.sum(1)
    t = ts.choose("count", p_all, n_points=n_points)["t"]
    out["thh_count_pack"] = np.frombuffer(ts.write_thh_pack("count", t=t), np.uint8)
    out["thh_count_counts"] = reconstruct_points(net, lat, origins, t, batch=C.ENCODE_BATCH)[1].astype(np.int32)
    out["thh_count_ties"] = np.asarray(int((p_all == ts.kth_largest(p_all, n_points)).sum().item()), np.int64)
    tb = ts.choose("block-count", p_all, block_counts=k_b)["t"]
    out["thh_block_pack"] = np.frombuffer(ts.write_thh_pack("block-count", block_counts=k_b), np.uint8)
    out["thh_block_counts"] = reconstruct_points(net, lat, origins, None, batch=C.ENCODE_BATCH,
                                                 block_counts=k_b)[1].astype(np.int32)
    v_b = ts.kth_largest(p_all, torch.from_numpy(k_b.astype(np.int64)).to(dev))
    assert torch.equal(ts.threshold_below(v_b), tb)
    out["thh_block_ties"] = (p_all.reshape(C.N_BLOCKS, -1) == v_b[:, None]).sum(1).cpu().numpy().astype(np.int64)
    return out


def fit(path, arrays):
    """Write, and while the file is over the cap drop the last block of ctx0 (ctx0_blocks says which are left)."""
    while True:
        C.write_npz(path, arrays)
        if os.path.getsize(path) < C.SIZE_CAP:
            return
        if len(arrays["ctx0_blocks"]) == 0:
            raise SystemExit(f"{path}: over {C.SIZE_CAP} bytes without any context")
        arrays["ctx0"], arrays["ctx0_blocks"] = arrays["ctx0"][:-1], arrays["ctx0_blocks"][:-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    parent = a.parent or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, stdout=subprocess.PIPE,
                                        text=True).stdout.strip()
    os.makedirs(a.out, exist_ok=True)
    for tag in C.TAGS:
        arrays = record(tag, parent)
        path = C.fixture_path(a.out, tag)
        fit(path, arrays)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, ctx0 of blocks {arrays['ctx0_blocks'].tolist()}, "
              f"lod k {arrays['lod_k'].tolist()} ties {arrays['lod_ties'].tolist()}, count ties "
              f"{int(arrays['thh_count_ties'])}, block ties {arrays['thh_block_ties'].tolist()}")
        for k in sorted(arrays):
            print("   ", k, arrays[k].dtype, arrays[k].shape)


if __name__ == "__main__":
    main()
