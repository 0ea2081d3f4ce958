#!/usr/bin/env python3
"""One frozen fit step against the latent step it is made of, on the same resident blocks (917: the flagship cloud), and
one block_costs evaluation.

    frozen   one step of TrainEngine.fit_latents: no weight preparation or packing, main-head-only forward and backward,
             Adam on emb
    latent   TrainEngine.latent_step(2): prepare_weights + pack, the three heads, Adam on emb
    costs    TrainEngine.block_costs(): prepare_weights + eval forward + nvf_block_costs

The three alternate inside one run (frozen, latent, costs, frozen, ...), each call timed as a whole by a host clock
around work that ends in a device synchronise; reported: the median and the quartiles over --rounds calls each.

    python tools/pframe_bench.py --blocks 917 --rounds 30
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import bench
    from nvfpcc_amd.engine import LATENT_CHUNK
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=917)
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--chanstr", default="8,16,8,8")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pframe_bench needs a HIP device: a timing taken elsewhere says nothing")
    a.force_collective = False
    eng = bench.build_engine(a, torch.device("cuda"), 1)
    lo, hi = 0, eng.N_leaf
    assert hi <= LATENT_CHUNK

    def frozen():       # the body of fit_latents' loop
        eng.noise_step += 1
        de = eng._latent_grad(lo, hi, main_only=True)[1]
        eng._latent_update(lo, hi, de)

    calls = {"frozen": frozen, "latent": lambda: eng.latent_step(2), "costs": lambda: eng.block_costs()}
    eng.prepare_weights(2)
    times = {k: [] for k in calls}
    for r in range(a.warmup + a.rounds):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append(1e3 * (time.perf_counter() - t0))
    res = {"blocks": eng.N_leaf, "decoder": eng.decoder_class, "rounds": a.rounds, "unit": "ms per whole call"}
    for name, t in times.items():
        q = np.percentile(t, [25, 50, 75])
        res[name] = {"median": round(float(q[1]), 3), "q25": round(float(q[0]), 3), "q75": round(float(q[2]), 3)}
    res["frozen_over_latent"] = round(res["frozen"]["median"] / res["latent"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
