#!/usr/bin/env python3
"""Times the lossless occupancy coder on N resident blocks, next to the eval forward it follows.

    python tools/lossless_bench.py --blocks 917 --batch 64 --chanstr 8,16,8,8 --ch 3 --reps 10 --warmup 2

What is timed is a whole call, latents and ground truth on the device in, bytes (encode) or occupancy words on the
device (decode) out:

    forward          Net.reconstruct over all blocks in calls of --batch: what both coder routes contain (the encoder twice)
    encode G         lossless_pack.encode_occupancy: forward + nvf_occ_ctx_hist, the table, forward + nvf_occ_rans_encode,
                     the copy of states and words to the host and the pack's bytes
    decode G         lossless_pack.decode_occupancy: the pack's bytes to the device, forward + nvf_occ_rans_decode, status
    coder G          nvf_occ_rans_encode / nvf_occ_rans_decode alone on one span of resident probabilities (what one
                     launch of the whole calls takes: lossless_pack.SPAN_GROUPS groups, one wave each), bracketed by
                     device events; the encoder's includes trimming each group's region to its words

for G = 16, 32 and 64 blocks per group.  --lod adds the scalable coder (lossless_lod_pack, csrc/occ_hier.hip) to the
same run, its routes alternating with v1's inside every repetition:

    lod_encode G     lossless_lod_pack.encode_occupancy: forward + pyramid + cell lists + histogram, the table, forward +
                     pyramid + cell lists + nvf_occ_hier_encode, the copies and the pack's bytes
    lod_decodeL G    lossless_lod_pack.decode_occupancy at level L = 0, 1, 2: forward + pyramid + the section launches
                     down to L with the cell-list launches between them
    lod_pyramid G    nvf_occ_hier_pyramid and the two cell lists alone on the span (the encoder's side, with ground truth)
    lod_coder G      nvf_occ_hier_encode alone, and the decoder's launches down to level 0, 1 and 2, on the span
--lod --ctx nbr adds the neighbour contexts (lossless_nbr_pack, nvf_occ_nbr_*) as a third coder, its routes nbr_encode,
nbr_decodeL, nbr_coder_encode and nbr_coder_decodeL alternating with the other two's in the same repetitions, and the
bytes and bpp of its packs ("nbr_packs") next to the scalable coder's ("lod_packs") on the same cloud.
--lod --ctx inter adds the inter contexts (lossless_inter_pack, nvf_occ_inter_*) as a fourth, next to the neighbour
contexts in the same repetitions: inter_encode, inter_decodeL, inter_coder_encode, inter_coder_decodeL, "inter_packs",
and ref_words: nvf_occ_ref_words with its key sort over the whole reference cloud, which is the benchmark's cloud moved
by one voxel along x on the lattice of synth.make_origins.
--lod --ctx inter --mv R adds block motion compensation (lossless_mv_pack, csrc/occ_motion.hip) in the same repetitions:
mv_ref_blocks (the reference on its own blocks: keys, unique and nvf_occ_ref_words), mv_search (nvf_occ_mv_search at radius
R over all blocks, with the copy of nothing: vectors stay on the device), mv_words (nvf_occ_mv_words over all blocks) and
inter_mv_encode G: the whole compensated encode from the reference's points -- its own blocks, the frame's words, the
search, the vectors' pack, the compensated words and lossless_inter_pack.encode_occupancy under them -- next to
inter_encode G, which is handed finished reference words (ref_words is its share of that work); "inter_mv_packs" and
"motion" (the vectors' bytes and how many blocks moved) say what it buys on this cloud.
  Every whole call ends in a synchronise (its result is on the host or its
status was read); the routes alternate inside every repetition, the first --warmup repetitions are dropped and the
median, minimum and maximum of the rest are reported in milliseconds.  Each pack is decoded and compared with the
ground truth's occupancy words first.  Weights and latents are seeded random numbers and the ground truth is a seeded
draw from the decoder's own probabilities, so the coder has a calibrated field to work with; its time depends on the
values only through the number of words it moves.  Prints one JSON line.  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=917)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--chanstr", default="8,16,8,8")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--groups", default="16,32,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lod", action="store_true", help="time the scalable coder (lossless_lod_pack) next to v1")
    ap.add_argument("--ctx", choices=["field", "nbr", "inter"], default="field",
                    help="nbr (with --lod): time the neighbour contexts (lossless_nbr_pack) next to the scalable coder; "
                         "inter: the inter contexts (lossless_inter_pack) next to both")
    ap.add_argument("--mv", type=int, default=0, metavar="R",
                    help="with --lod --ctx inter: time the motion search of radius R (1..8), the compensated words and the "
                         "whole compensated encode next to the inter contexts'")
    a = ap.parse_args()
    if a.ctx != "field" and not a.lod:
        raise SystemExit(f"lossless_bench.py: --ctx {a.ctx} is a route of the scalable coder; give --lod too")
    if a.mv and (a.ctx != "inter" or not 1 <= a.mv <= 8):
        raise SystemExit(f"lossless_bench.py: --mv {a.mv} is a search radius in 1..8 for the reference of --ctx inter")
    if not torch.cuda.is_available():
        raise SystemExit("lossless_bench.py needs a HIP device: nothing here can be timed on a CPU")
    from nvfpcc_amd import lossless_inter_pack as ilp, lossless_lod_pack as llp, lossless_nbr_pack as nlp
    from nvfpcc_amd import lossless_mv_pack as mp, lossless_pack as lp, network, ops
    from nvfpcc_amd.model import Net
    from nvfpcc_amd.recon import eval_batches
    from nvfpcc_amd.seeds import synthetic_seed
    dev = torch.device("cuda")
    network.reset_seed(synthetic_seed())
    net = Net(None, "Gaussian", a.ch, a.chanstr, verbose=False)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith("kernel") or n.endswith(".b"):
                p.add_(0.03 * torch.randn(p.shape, generator=g))
    net = net.to(dev)
    lat = torch.round(2.0 * torch.randn(a.blocks, a.ch, 2, 2, 2, generator=g)).to(dev)
    groups = [int(v) for v in a.groups.split(",")]
    gd = torch.Generator(device=dev).manual_seed(4)
    gts = []
    with torch.no_grad():
        for _, _, p in eval_batches(net, lat, a.batch):
            # sharpened so that the cloud is sparse, as a leaf block is
            gts.append((torch.rand(p.shape, device=dev, generator=gd) < p ** 8).float())
    gt = torch.cat(gts, 0)
    n_points = int(gt.sum().item())

    def forward():
        with torch.no_grad():
            for _ in eval_batches(net, lat, a.batch):
                pass
        torch.cuda.synchronize()

    packs, info = {}, {}
    for G in groups:
        packs[G], side = lp.encode_occupancy(net, lat, gt, batch=a.batch, group=G)
        words, counts = lp.decode_occupancy(net, lat, packs[G], batch=a.batch)
        if not torch.equal(words, side["gt_words"]) or int(counts.sum().item()) != n_points:
            raise SystemExit(f"group {G}: the pack does not decode to the ground truth")
        info[G] = {"bytes": len(packs[G]), "bpp": round(8 * len(packs[G]) / n_points, 4),
                   "ideal_bpp": round(side["ideal_bits"] / n_points, 4)}
    ref, ref_pts, ref_org, ref_dropped = (), None, None, 0
    if a.ctx == "inter":                    # the cloud itself, one voxel along x, as a decoder would hold it: as points
        from nvfpcc_amd.synth import make_origins
        ref_org = torch.from_numpy(make_origins(a.blocks)).to(torch.int32).to(dev)
        nz = gt.reshape(a.blocks, 32, 32, 32).nonzero()
        ref_pts = (ref_org[nz[:, 0]] + nz[:, 1:].to(torch.int32) + torch.tensor([0, 0, 1], dtype=torch.int32, device=dev)).contiguous()
        words, dropped = ops.occ_ref_words(ref_pts, ref_org)
        ref, ref_dropped = (words,), int(dropped.item())
    lod_packs, lod_info, nbr_packs, nbr_info, inter_packs, inter_info = {}, {}, {}, {}, {}, {}
    mv_packs, mv_info, motion, ref_mv = {}, {}, {}, ()

    def compensated():
        """From the reference's points to (the vectors' pack, R'): everything --lossless_mv adds to an inter encode."""
        own = mp.reference_blocks(ref_pts, dev)
        mv = mp.search(mp.frame_words(gt), own, ref_org, a.mv)[0]
        return mp.write(a.mv, mv), mp.compensated_words(own, ref_org, mv)
    if a.mv:
        own = mp.reference_blocks(ref_pts, dev)
        gt_w0 = mp.frame_words(gt)
        mv_dev, cost = mp.search(gt_w0, own, ref_org, a.mv)
        vec_pack, rprime = compensated()
        ref_mv = (rprime,)
        moved = int((mv_dev != 0).any(1).sum().item())
        motion = {"radius": a.mv, "bytes": len(vec_pack), "moved": moved, "ref_blocks": int(own[1].shape[0]),
                  "distance": int(cost[:, 0].sum().item()), "distance_at_0": int(cost[:, 1].sum().item()),
                  "words_equal_frame": bool(torch.equal(rprime, gt_w0))}
    coders = ([("scalable", llp, lod_packs, lod_info, ())] if a.lod else []) + \
             ([("neighbour", nlp, nbr_packs, nbr_info, ())] if a.ctx in ("nbr", "inter") else []) + \
             ([("inter", ilp, inter_packs, inter_info, ref)] if a.ctx == "inter" else []) + \
             ([("compensated inter", ilp, mv_packs, mv_info, ref_mv)] if a.mv else [])
    for what, mod, out_packs, out_info, extra in coders:
        for G in groups:
            out_packs[G], side = mod.encode_occupancy(net, lat, gt, *extra, batch=a.batch, group=G)
            for level in (0, 1, 2):
                words, counts = mod.decode_occupancy(net, lat, out_packs[G], *extra, level=level, batch=a.batch)
                if not torch.equal(words, side["gt_words"][level]) or (level == 0 and int(counts.sum().item()) != n_points):
                    raise SystemExit(f"group {G}: the {what} pack does not decode to the ground truth at level {level}")
            out_info[G] = {"bytes": len(out_packs[G]), "bpp": round(8 * len(out_packs[G]) / n_points, 4),
                           "ideal_bpp": round(side["ideal_bits"] / n_points, 4), "contexts": side["contexts"],
                           "symbols": side["symbols"], "v1_symbols": a.blocks * 32768}
    routes = {"forward": forward}
    if a.ctx == "inter":
        routes["ref_words"] = lambda: ops.occ_ref_words(ref_pts, ref_org)
    if a.mv:
        routes["mv_ref_blocks"] = lambda: mp.reference_blocks(ref_pts, dev)
        routes["mv_search"] = lambda: mp.search(gt_w0, own, ref_org, a.mv)
        routes["mv_words"] = lambda: mp.compensated_words(own, ref_org, mv_dev)
    for G in groups:
        routes[f"encode_G{G}"] = lambda G=G: lp.encode_occupancy(net, lat, gt, batch=a.batch, group=G)
        routes[f"decode_G{G}"] = lambda G=G: lp.decode_occupancy(net, lat, packs[G], batch=a.batch)
        for tag, mod, its_packs, extra in (("lod", llp, lod_packs, ()), ("nbr", nlp, nbr_packs, ()), ("inter", ilp, inter_packs, ref)):
            if G not in its_packs:
                continue
            routes[f"{tag}_encode_G{G}"] = lambda G=G, mod=mod, extra=extra: \
                mod.encode_occupancy(net, lat, gt, *extra, batch=a.batch, group=G)
            if tag == "inter" and a.mv:
                routes[f"inter_mv_encode_G{G}"] = lambda G=G: \
                    ilp.encode_occupancy(net, lat, gt, compensated()[1], batch=a.batch, group=G)
            for level in (0, 1, 2):
                routes[f"{tag}_decode{level}_G{G}"] = lambda G=G, level=level, mod=mod, its_packs=its_packs, extra=extra: \
                    mod.decode_occupancy(net, lat, its_packs[G], *extra, level=level, batch=a.batch)
    times = {k: [] for k in routes}
    for rep in range(a.warmup + a.reps):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[name].append(1e3 * (time.perf_counter() - t0))

    # the coder kernels alone, on one span of resident probabilities
    span = {}
    with torch.no_grad():
        for G in groups:
            nb = min(lp._span(a.batch, G, lp.SPAN_GROUPS), a.blocks)
            p = net.reconstruct(lat[:nb].contiguous(), 2)
            cnt, occ, _ = ops.occ_ctx_hist(p, gt[:nb].contiguous())
            f1 = torch.tensor(lp.table_from_counts(cnt.tolist(), occ.tolist()), dtype=torch.int32, device=dev)
            states, words, _ = ops.occ_rans_encode(p, gt[:nb].contiguous(), f1, G)
            nwords = torch.tensor([w.numel() for w in words], dtype=torch.int32, device=dev)
            span[G] = (nb, p, gt[:nb].contiguous(), f1, states, torch.cat(words), nwords)
            times[f"coder_encode_G{G}"], times[f"coder_decode_G{G}"] = [], []
            if a.lod:
                pyr = ops.occ_hier_pyramid(p, span[G][2])
                hf1, _ = llp.table_from_counts(*(t.tolist() for t in ops.occ_hier_hist(pyr)))
                hf1 = torch.tensor(hf1, dtype=torch.int32, device=dev)
                hs, hw = ops.occ_hier_encode(pyr, hf1, G)
                span[G] += (pyr, hf1, hs, torch.cat(hw), torch.tensor([w.numel() for w in hw], dtype=torch.int32, device=dev))
                for name in ("pyramid", "coder_encode", "coder_decode0", "coder_decode1", "coder_decode2"):
                    times[f"lod_{name}_G{G}"] = []
                if a.ctx in ("nbr", "inter"):
                    nf1, _ = nlp.table_from_counts(*(t.tolist() for t in ops.occ_nbr_hist(pyr)))
                    nf1 = torch.tensor(nf1, dtype=torch.int32, device=dev)
                    ns, nw = ops.occ_nbr_encode(pyr, nf1, G)
                    span[G] += (nf1, ns, torch.cat(nw), torch.tensor([w.numel() for w in nw], dtype=torch.int32, device=dev))
                    for name in ("coder_encode", "coder_decode0", "coder_decode1", "coder_decode2"):
                        times[f"nbr_{name}_G{G}"] = []
                if a.ctx == "inter":
                    rw = ref[0][:nb].contiguous()
                    if1, _ = ilp.table_from_counts(*(t.tolist() for t in ops.occ_inter_hist(pyr, rw)))
                    if1 = torch.tensor(if1, dtype=torch.int32, device=dev)
                    is_, iw = ops.occ_inter_encode(pyr, rw, if1, G)
                    span[G] += (rw, if1, is_, torch.cat(iw), torch.tensor([w.numel() for w in iw], dtype=torch.int32, device=dev))
                    for name in ("coder_encode", "coder_decode0", "coder_decode1", "coder_decode2"):
                        times[f"inter_{name}_G{G}"] = []
        for rep in range(a.warmup + a.reps):
            for G in groups:
                nb, p, gg, f1, states, flat, nwords = span[G][:7]
                timed = [(f"coder_encode_G{G}", lambda: ops.occ_rans_encode(p, gg, f1, G)),
                         (f"coder_decode_G{G}", lambda: ops.occ_rans_decode(p, f1, states, flat, nwords, G))]
                if a.lod:
                    pyr, hf1, hs, hflat, hn = span[G][7:12]
                    timed += [(f"lod_pyramid_G{G}", lambda: ops.occ_hier_pyramid(p, gg)),
                              (f"lod_coder_encode_G{G}", lambda: ops.occ_hier_encode(pyr, hf1, G))]
                    timed += [(f"lod_coder_decode{level}_G{G}", lambda level=level: ops.occ_hier_decode(pyr, hf1, hs, hflat, hn, G, level))
                              for level in (0, 1, 2)]
                if a.ctx in ("nbr", "inter"):
                    nf1, ns, nflat, nn = span[G][12:16]
                    timed += [(f"nbr_coder_encode_G{G}", lambda: ops.occ_nbr_encode(pyr, nf1, G))]
                    timed += [(f"nbr_coder_decode{level}_G{G}", lambda level=level: ops.occ_nbr_decode(pyr, nf1, ns, nflat, nn, G, level))
                              for level in (0, 1, 2)]
                if a.ctx == "inter":
                    rw, if1, is_, iflat, inn = span[G][16:]
                    timed += [(f"inter_coder_encode_G{G}", lambda: ops.occ_inter_encode(pyr, rw, if1, G))]
                    timed += [(f"inter_coder_decode{level}_G{G}", lambda level=level: ops.occ_inter_decode(pyr, rw, if1, is_, iflat, inn, G, level))
                              for level in (0, 1, 2)]
                for name, fn in timed:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= a.warmup:
                        times[name].append(e0.elapsed_time(e1))
    out = {"tool": "lossless_bench", "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "batch": a.batch,
           "chanstr": a.chanstr, "reps": a.reps, "warmup": a.warmup, "points": n_points,
           "span_blocks": {str(G): span[G][0] for G in groups}, "packs": {str(G): v for G, v in info.items()},
           "lod_packs": {str(G): v for G, v in lod_info.items()}, "nbr_packs": {str(G): v for G, v in nbr_info.items()},
           "inter_packs": {str(G): v for G, v in inter_info.items()},
           "inter_mv_packs": {str(G): v for G, v in mv_info.items()}, "motion": motion,
           "reference": {"points": 0 if ref_pts is None else int(ref_pts.shape[0]), "dropped": ref_dropped},
           "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                  for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
