#!/usr/bin/env python3
"""RD effect of the threshold modes at ONE lambda, on tools/rd_sweep.py's recipe (synthetic 10-bit surface ->
pre-process -> train -> 4-bit weights): the same trained network encoded and decoded with --thh 0.64 and with
--thh_mode count / block-count / d1.  bpp comes from the real stream lengths, the side information of thh_pack
included; D1 is the symmetric point-to-point PSNR of nvfpcc_amd.pc_metrics (peak 1023) of rc_dec.ply against the
input cloud.  The table is a measurement, not a claim that any mode wins.

    python tools/thh_mode_rd.py --lmbda 400 --out profiles/thh_modes_rd_narrow.md
"""
import argparse
import os
import pickle
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lmbda", type=float, default=400.0)
    ap.add_argument("--epochs", type=int, default=301)
    ap.add_argument("--phase_change", type=int, default=100)
    ap.add_argument("--radius", type=float, default=150.0)
    ap.add_argument("--n_dir", type=int, default=1500000)
    ap.add_argument("--chanstr", default="8,16,8,8")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--thh", type=float, default=0.64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from rd_sweep import make_cloud, run
    from nvfpcc_amd.pc_metrics import geometry_psnr
    from nvfpcc_amd.preprocess import preprocess
    from nvfpcc_amd.recon import read_ply_ascii
    from tests.golden_inputs import write_cloud_ply
    wd = tempfile.mkdtemp(prefix="nvf_thh_")
    os.chdir(wd)
    log = open("thh_mode_rd.log", "w")
    pts = make_cloud(7, a.radius, a.n_dir)
    write_cloud_ply("cloud.ply", pts)
    origins, _, _ = preprocess("cloud.ply")
    n_pts, n_blk = len(pts), len(origins)
    cli = os.path.join(ROOT, "NVFPCC.py")
    common = ["--chanstr", a.chanstr, "--ch", str(a.ch)]
    t0 = time.time()
    run([cli, "train", "cloud.ply", "--checkpoint_dir", "ck", "--batchsize", "16", "--lambda", str(a.lmbda), "--lr", "1e-3",
         "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True", "--epochs", str(a.epochs), "--phase_change",
         str(a.phase_change)] + common, wd, log)
    t_train = time.time() - t0
    last = (a.epochs - 1) // 10 * 10
    run([os.path.join(ROOT, "manipulate_weights.py"), f"ck/{last:04d}.ckpt", "q.ckpt", "16"], wd, log)
    lines = [f"Threshold modes at one lambda, tools/rd_sweep.py's recipe: synthetic 10-bit surface, {n_pts} points, {n_blk} "
             f"level-5 cubes; lambda {a.lmbda:g}, ch={a.ch}, chanstr={a.chanstr}, {a.epochs} epochs (phase change "
             f"{a.phase_change}), batch 16, lr 1e-3, w1 10, w2 57, wemb 5, qp 16; training {t_train:.0f} s; 1 x MI355X.",
             "", "Command: `python tools/thh_mode_rd.py " + " ".join(sys.argv[1:]) + "`", "",
             "| mode | threshold | bpp | side info (bits) | decoded points | decoded / input | D1 PSNR sym. (dB) | "
             "D1 mse input->decoded | D1 mse decoded->input | rc_enc == rc_dec | encode s |", "|" + "---|" * 11]
    for mode in ("fixed", "count", "block-count", "d1"):
        extra = ["--thh", str(a.thh)] if mode == "fixed" else ["--thh_mode", mode]
        t0 = time.time()
        out = run([cli, "encode", "cloud.ply", "--batchsize", "64", "--load_weights", "q.ckpt", "--load_emb",
                   f"ck/{last:04d}_emb.ckpt", "--pack_fn", "pack.pk"] + extra + common, wd, log)
        t_enc = time.time() - t0
        run([cli, "decode", "pack.pk", "--batchsize", "64", "--N", str(n_blk)] + (extra if mode == "fixed" else []) + common,
            wd, log)
        enc, dec = read_ply_ascii("rc_enc.ply"), read_ply_ascii("rc_dec.ply")
        same = enc.shape == dec.shape and np.array_equal(enc, dec)
        pack = pickle.load(open("pack.pk", "rb"))
        side = 8 * len(pack.get("thh_pack", b""))
        bits = 8 * len(pack["latent_pack"]["latent_byte_stream"]) + 8 * len(pack["net_weight_pack"]["bit_stream"]) + side
        th = [ln for ln in out.splitlines() if ln.startswith("[Threshold] mode")]
        shown = th[0].split("mode: ")[1].split(" ", 1)[1] if th else f"t: {a.thh}"
        if len(dec):
            r = geometry_psnr(pts, dec.astype(np.int64), d2=False)
            d1 = "%.2f | %.4f | %.4f" % (r["d1_psnr"], r["ref_to_test"]["d1_mse"], r["test_to_ref"]["d1_mse"])
        else:
            d1 = "- | - | -"
        lines.append(f"| {mode}{'' if mode != 'fixed' else ' ' + str(a.thh)} | {shown} | {bits / n_pts:.4f} | {side} | "
                     f"{len(dec)} | {len(dec) / n_pts:.3f} | {d1} | {same} | {t_enc:.1f} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
