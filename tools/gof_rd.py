#!/usr/bin/env python3
"""Four frames coded alone against the same four frames as one group (--gof 4), at one lambda, on the synthetic surface
of tools/rd_sweep.py: the surface moves one or two voxels per frame and its radius grows slightly.  Both routes run the
same command lines but for --gof: --from_ply, --pack_octree, --thh_mode count, the same epochs.  Per frame the table
gives bpp split into weights, latents and side packs (from the real stream lengths) and the symmetric D1 PSNR that
decode --ref_ply prints; per route the training seconds.  A measurement, not a test: whichever way it falls is written down.

    python tools/gof_rd.py --lambda 200 --epochs 301 --out profiles/gof_rd.md

Every step is a subprocess under its own time limit; the first one that fails ends the run.
"""
import argparse
import os
import pickle
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "NVFPCC.py")
SHIFT = np.array([1, 2, 1])     # voxels per frame
FRAMES = 4


def run(cmd, cwd, log, limit):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=limit)
    log.write("$ " + " ".join(cmd) + "\n" + r.stdout)
    log.flush()
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stdout[-2000:]))
    return r.stdout


def d1_lines(out):
    return [float(v) for v in re.findall(r"^\[PCError\] D1 PSNR: (\S+) D2 PSNR", out, re.M)]


def main():
    from nvfpcc_amd import gof
    from tests.golden_inputs import write_cloud_ply
    from tools.rd_sweep import make_cloud
    ap = argparse.ArgumentParser()
    ap.add_argument("--lambda", type=float, default=200.0, dest="lmbda")
    ap.add_argument("--epochs", type=int, default=301)
    ap.add_argument("--phase_change", type=int, default=100)
    ap.add_argument("--radius", type=float, default=150.0)
    ap.add_argument("--growth", type=float, default=0.75, help="radius added per frame")
    ap.add_argument("--n_dir", type=int, default=1500000)
    ap.add_argument("--chanstr", default="8,16,8,8")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--start", type=int, default=1300)
    ap.add_argument("--train_limit", type=int, default=300, help="seconds one training run may take")
    ap.add_argument("--step_limit", type=int, default=120, help="seconds any other step may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--workdir", default="")
    a = ap.parse_args()
    wd = a.workdir or tempfile.mkdtemp(prefix="nvf_gof_")
    os.makedirs(wd, exist_ok=True)
    log = open(os.path.join(wd, "gof_rd.log"), "w")
    numbers = [a.start + k for k in range(FRAMES)]
    clouds = []
    for k, n in enumerate(numbers):
        pts = make_cloud(7, a.radius + a.growth * k, a.n_dir) + SHIFT * k
        clouds.append(pts)
        write_cloud_ply(os.path.join(wd, "seq_%04d.ply" % n), pts)
    points = [len(p) for p in clouds]
    last = (a.epochs - 1) // 10 * 10
    common = ["--chanstr", a.chanstr, "--ch", str(a.ch)]
    train = ["--from_ply", "--batchsize", "16", "--lambda", str(a.lmbda), "--lr", "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5",
             "--shuffle", "True", "--epochs", str(a.epochs), "--phase_change", str(a.phase_change)] + common
    code = ["--from_ply", "--pack_octree", "--thh_mode", "count", "--batchsize", "64"] + common

    def collapsed(lat_bits, n):
        # every latent codes to the same symbol and the stream is a few bytes: the rate term won the first epochs.  A
        # property of (lambda, noise seed), not an operating point (tools/rd_sweep.py): said in the table, and the route
        # is trained once more with the next noise seed
        return lat_bits / float(n) < 1e-3

    # ---- every frame alone
    rows, t_alone, t_group = [], 0.0, 0.0
    for k, n in enumerate(numbers):
        for seed in range(3):
            name, ck = "seq_%04d.ply" % n, "alone_%04d_s%d" % (n, seed)
            t0 = time.time()
            run([CLI, "train", name, "--checkpoint_dir", ck, "--seed", str(seed)] + train, wd, log, a.train_limit)
            t_alone += time.time() - t0
            run([os.path.join(ROOT, "manipulate_weights.py"), f"{ck}/{last:04d}.ckpt", f"q_{n:04d}.ckpt", "16"], wd, log, a.step_limit)
            run([CLI, "encode", name, "--load_weights", f"q_{n:04d}.ckpt", "--load_emb", f"{ck}/{last:04d}_emb.ckpt", "--pack_fn",
                 f"alone_{n:04d}.pk"] + code, wd, log, a.step_limit)
            out = run([CLI, "decode", f"alone_{n:04d}.pk", "--batchsize", "64", "--ref_ply", name] + common, wd, log, a.step_limit)
            with open(os.path.join(wd, f"alone_{n:04d}.pk"), "rb") as f:
                pack = pickle.load(f)
            w = 8 * len(pack["net_weight_pack"]["bit_stream"])
            lat, side = gof.frame_bits(pack)
            rows.append(("alone", n, points[k], w, lat, side, d1_lines(out)[0], seed, collapsed(lat, points[k])))
            print(rows[-1], flush=True)
            if not rows[-1][8]:
                break
    # ---- the four as one group
    flags = ["--gof", str(FRAMES), "--frame_start", str(a.start)]
    for seed in range(3):
        ck = "group_s%d" % seed
        t0 = time.time()
        run([CLI, "train", "seq_%04d.ply", "--checkpoint_dir", ck, "--seed", str(seed)] + flags + train, wd, log, a.train_limit)
        t_group += time.time() - t0
        run([os.path.join(ROOT, "manipulate_weights.py"), f"{ck}/{last:04d}.ckpt", "q_group.ckpt", "16"], wd, log, a.step_limit)
        run([CLI, "encode", "seq_%04d.ply", "--load_weights", "q_group.ckpt", "--load_emb", f"{ck}/{last:04d}_emb.ckpt", "--pack_fn",
             "group.pk"] + flags + code, wd, log, a.step_limit * FRAMES)
        out = run([CLI, "decode", "group.pk", "--batchsize", "64", "--ref_ply", "seq_%04d.ply"] + common, wd, log, a.step_limit * FRAMES)
        with open(os.path.join(wd, "group.pk"), "rb") as f:
            pack = pickle.load(f)
        acc, d1 = gof.account(pack), d1_lines(out)
        assert len(d1) == FRAMES, out[-2000:]
        bad = collapsed(acc["latent_bits"], acc["points"])
        for k, n in enumerate(numbers):
            lat, side = gof.frame_bits(pack["frames"][k])
            # a frame's share of the group's weights and framing: in proportion to its points
            share = (acc["weight_bits"] + acc["gof_bits"]) * points[k] / float(acc["points"])
            rows.append(("group", n, points[k], share, lat, side, d1[k], seed, bad))
            print(rows[-1], flush=True)
        if not bad:
            break

    lines = ["| route | noise seed | frame | points | bpp | bpp weights | bpp latents | bpp side | D1 PSNR sym. (dB) | note |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    note = lambda r: "COLLAPSED RUN: the latent table ended constant; not an operating point%s" % (
        ", retrained with the next seed" if r[7] < 2 else "") if r[8] else ""
    for route in ("alone", "group"):
        for r in [r for r in rows if r[0] == route]:
            lines.append(f"| {route} | {r[7]} | {r[1]:04d} | {r[2]} | {(r[3] + r[4] + r[5]) / r[2]:.4f} | {r[3] / r[2]:.4f} | "
                         f"{r[4] / r[2]:.4f} | {r[5] / r[2]:.4f} | {r[6]:.2f} | {note(r)} |")
        rs = [r for r in rows if r[0] == route and not r[8]]     # the runs that are operating points
        if len(rs) == FRAMES:
            n = float(sum(r[2] for r in rs))
            lines.append(f"| {route} | | all | {int(n)} | {sum(r[3] + r[4] + r[5] for r in rs) / n:.4f} | {sum(r[3] for r in rs) / n:.4f} | "
                         f"{sum(r[4] for r in rs) / n:.4f} | {sum(r[5] for r in rs) / n:.4f} | {np.mean([r[6] for r in rs]):.2f} (mean) | |")
        else:
            lines.append(f"| {route} | | all | | | | | | | no operating point for every frame within three noise seeds |")
    table = "\n".join(lines)
    head = (f"Four frames alone against one group of four (--gof 4) on the synthetic 10-bit surface of tools/rd_sweep.py (radius "
            f"{a.radius:g} + {a.growth:g} per frame, moved by {SHIFT.tolist()} voxels per frame): lambda {a.lmbda:g}, ch={a.ch}, "
            f"chanstr={a.chanstr}, {a.epochs} epochs (phase change {a.phase_change}), batch 16, lr 1e-3, w1 10, w2 57, wemb 5, qp 16, "
            f"--from_ply --pack_octree --thh_mode count on both routes; 1 x MI355X.  A group frame's weights column is its share, by "
            f"points, of the group's one net_weight_pack and gof_pack; side = octree_pack + thh_pack.  Training, wall clock of "
            f"the train commands with start-up, collapsed runs included: {t_alone:.0f} s for the runs alone, {t_group:.0f} s for the "
            f"group's.\n\n")
    print(head + table)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write(head + table + "\n")


if __name__ == "__main__":
    main()
