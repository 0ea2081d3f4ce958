#!/usr/bin/env python3
"""Frames 1-3 of the tools/gof_rd.py sequence coded as latents-only packs under frame 0's frozen decoder, against the
same four frames coded alone (the `alone` rows of profiles/gof_rd.md: same clouds, lambda and flags).  Frame 0 is trained
and coded alone and is the reference pack; each later frame is fitted by train --freeze_decoder, once warm-started from
frame 0's latents (--ref_pack --load_emb) and once from the table of ones, encoded with --ref_pack and decoded with it.
Per frame the table gives bpp split into weights, latents and side packs (from the real stream lengths; a P pack's
"weights" are its 33-byte ref_pack), the symmetric D1 PSNR that decode --ref_ply prints, and the fit's wall clock.
A measurement, not a test: whichever way it falls is written down.

    python tools/pframe_rd.py --lambda 200 --epochs 301 --fit_steps 301 --out profiles/pframe_rd.md

Every step is a subprocess under its own time limit; the first one that fails ends the run.
"""
import argparse
import os
import pickle
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "NVFPCC.py")


def main():
    from nvfpcc_amd import gof
    from tests.golden_inputs import write_cloud_ply
    from tools.gof_rd import FRAMES, SHIFT, d1_lines, run
    from tools.rd_sweep import make_cloud
    ap = argparse.ArgumentParser()
    ap.add_argument("--lambda", type=float, default=200.0, dest="lmbda")
    ap.add_argument("--epochs", type=int, default=301, help="training epochs of frame 0")
    ap.add_argument("--fit_steps", type=int, default=301, help="latent steps of each frozen fit")
    ap.add_argument("--phase_change", type=int, default=100)
    ap.add_argument("--radius", type=float, default=150.0)
    ap.add_argument("--growth", type=float, default=0.75, help="radius added per frame")
    ap.add_argument("--n_dir", type=int, default=1500000)
    ap.add_argument("--chanstr", default="8,16,8,8")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--start", type=int, default=1300)
    ap.add_argument("--train_limit", type=int, default=300, help="seconds one training run or fit may take")
    ap.add_argument("--step_limit", type=int, default=120, help="seconds any other step may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--workdir", default="")
    a = ap.parse_args()
    wd = a.workdir or tempfile.mkdtemp(prefix="nvf_pframe_")
    os.makedirs(wd, exist_ok=True)
    log = open(os.path.join(wd, "pframe_rd.log"), "w")
    numbers = [a.start + k for k in range(FRAMES)]
    points = []
    for k, n in enumerate(numbers):
        pts = make_cloud(7, a.radius + a.growth * k, a.n_dir) + SHIFT * k
        points.append(len(pts))
        write_cloud_ply(os.path.join(wd, "seq_%04d.ply" % n), pts)
    last = (a.epochs - 1) // 10 * 10
    common = ["--chanstr", a.chanstr, "--ch", str(a.ch)]
    hyper = ["--from_ply", "--lambda", str(a.lmbda), "--lr", "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5"] + common
    train = ["--batchsize", "16", "--shuffle", "True", "--epochs", str(a.epochs), "--phase_change", str(a.phase_change)] + hyper
    code = ["--from_ply", "--pack_octree", "--thh_mode", "count", "--batchsize", "64"] + common
    dec = ["--batchsize", "64"] + common

    def pack_of(name):
        with open(os.path.join(wd, name), "rb") as f:
            return pickle.load(f)

    # ---- frame 0: trained and coded alone; its pack is the reference
    name0 = "seq_%04d.ply" % numbers[0]
    t0 = time.time()
    run([CLI, "train", name0, "--checkpoint_dir", "ref"] + train, wd, log, a.train_limit)
    t_train = time.time() - t0
    run([os.path.join(ROOT, "manipulate_weights.py"), f"ref/{last:04d}.ckpt", "q_ref.ckpt", "16"], wd, log, a.step_limit)
    run([CLI, "encode", name0, "--load_weights", "q_ref.ckpt", "--load_emb", f"ref/{last:04d}_emb.ckpt", "--pack_fn", "ref.pk"]
        + code, wd, log, a.step_limit)
    out = run([CLI, "decode", "ref.pk", "--ref_ply", name0] + dec, wd, log, a.step_limit)
    ref = pack_of("ref.pk")
    lat, side = gof.frame_bits(ref)
    rows = [("I (alone)", numbers[0], points[0], 8 * len(ref["net_weight_pack"]["bit_stream"]), lat, side, d1_lines(out)[0],
             t_train, "")]
    print(rows[-1], flush=True)

    # ---- frames 1 ..: latents only, under the reference's decoder
    for route, warm in (("P, warm start", ["--ref_pack", "ref.pk", "--load_emb", f"ref/{last:04d}_emb.ckpt"]), ("P, from ones", [])):
        for k in range(1, FRAMES):
            n, name, ck = numbers[k], "seq_%04d.ply" % numbers[k], "fit_%s_%04d" % ("warm" if warm else "ones", numbers[k])
            t0 = time.time()
            fit = run([CLI, "train", name, "--freeze_decoder", "--load_weights", "q_ref.ckpt", "--checkpoint_dir", ck, "--epochs",
                       str(a.fit_steps)] + warm + hyper, wd, log, a.train_limit)
            t_fit = time.time() - t0
            run([CLI, "encode", name, "--load_weights", "q_ref.ckpt", "--load_emb", f"{ck}/{a.fit_steps - 1:04d}_emb.ckpt", "--pack_fn",
                 f"{ck}.pk", "--ref_pack", "ref.pk"] + code, wd, log, a.step_limit)
            out = run([CLI, "decode", f"{ck}.pk", "--ref_pack", "ref.pk", "--ref_ply", name] + dec, wd, log, a.step_limit)
            p = pack_of(f"{ck}.pk")
            assert "net_weight_pack" not in p
            lat, side = gof.frame_bits(p)
            J = [float(v) for v in re.findall(r"^\[Fit \d{4} \S+ seconds\] J: (\S+) ", fit, re.M)]
            imp = re.findall(r"improved: (\d+) / (\d+)", fit)[-1]
            note = "fit: sum J %.4e -> %.4e, %s of %s blocks improved" % (J[0], J[-1], imp[0], imp[1])
            if lat / float(points[k]) < 1e-3:
                note += "; COLLAPSED: the latent table ended constant, not an operating point"
            rows.append((route, n, points[k], 8 * len(p["ref_pack"]), lat, side, d1_lines(out)[0], t_fit, note))
            print(rows[-1], flush=True)

    lines = ["| route | frame | points | bpp | bpp weights | bpp latents | bpp side | D1 PSNR sym. (dB) | train / fit wall clock (s) | note |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]:04d} | {r[2]} | {(r[3] + r[4] + r[5]) / r[2]:.4f} | {r[3] / r[2]:.4f} | {r[4] / r[2]:.4f} | "
                     f"{r[5] / r[2]:.4f} | {r[6]:.2f} | {r[7]:.1f} | {r[8]} |")
    for route in ("P, warm start", "P, from ones"):     # the sequence: frame 0 alone + three P frames
        rs = [rows[0]] + [r for r in rows if r[0] == route]
        n = float(sum(r[2] for r in rs))
        lines.append(f"| I + 3 x {route} | all | {int(n)} | {sum(r[3] + r[4] + r[5] for r in rs) / n:.4f} | {sum(r[3] for r in rs) / n:.4f} | "
                     f"{sum(r[4] for r in rs) / n:.4f} | {sum(r[5] for r in rs) / n:.4f} | {sum(r[6] for r in rs) / len(rs):.2f} (mean) | "
                     f"{sum(r[7] for r in rs):.1f} | |")
    table = "\n".join(lines)
    head = (f"Frame 0 coded alone and frames 1-3 as latents-only packs under its frozen decoder, on the sequence of tools/gof_rd.py "
            f"(synthetic 10-bit surface of tools/rd_sweep.py, radius {a.radius:g} + {a.growth:g} per frame, moved by {SHIFT.tolist()} "
            f"voxels per frame): lambda {a.lmbda:g}, ch={a.ch}, chanstr={a.chanstr}; frame 0: {a.epochs} epochs (phase change "
            f"{a.phase_change}), batch 16; every fit: {a.fit_steps} latent steps, evaluated every 10; lr 1e-3, w1 10, w2 57, wemb 5, "
            f"qp 16, --from_ply --pack_octree --thh_mode count; 1 x MI355X.  A P pack's weights column is its 33-byte ref_pack; side "
            f"= octree_pack + thh_pack.  Wall clock is that of the train command with start-up.  The comparison row is `alone | all` "
            f"of profiles/gof_rd.md.\n\n")
    print(head + table)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(head + table + "\n")


if __name__ == "__main__":
    main()
