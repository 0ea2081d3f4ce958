"""BASELINE.json configs[3] on what a one-GPU test box allows: the data-parallel engine step through a REAL
collective between separate processes.  Two fresh child processes share GPU 0 (gloo on the host side stands in for
RCCL, which refuses two ranks on one device; the engine, the hooks, the sharding and the idle-rank path are the
production code) and must reproduce the single-process run: same all-reduced gradients, same parameters after
Adam, same latent table after the sharded latent step + all-gather, same epoch log sums."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist_worker.py")


def launch(world, out, n, batch, epochs, extra_env=None, backend="gloo"):
    """One child process per rank (the parent never joins the group).  backend "gloo": every rank on GPU 0, the host
    side reduces; "nccl" = RCCL, rank r on GPU r.  A rank that hangs (a collective that never completes) is killed by the
    watchdog below -- a child process, never a re-exec of a process that touched the GPU -- and the test fails."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, PYTHONPATH=ROOT, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NVF_DIST_BACKEND=backend,
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        if backend == "gloo":
            env["NVF_DEVICE_OVERRIDE"] = "0"
        else:
            env.pop("NVF_DEVICE_OVERRIDE", None)
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, WORKER, out, str(n), str(batch), str(epochs)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for p, o in zip(procs, logs):
        assert p.returncode == 0, o[-3000:]
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(900)
def test_two_ranks_through_a_real_collective_equal_one_rank(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    # 17 blocks, global mini-batch 8: two full mini-batches (4 blocks per rank, graph replay; the all-reduce runs from
    # the host between the step graph and the optimiser node) and a last one of ONE block -- rank 1 idles there and
    # must still add its share of the weight-rate gradient.  Epoch 0 at q = 1 (weight noise identical on both ranks),
    # epoch 1 at q = 2.
    N, B, E = 17, 8, 2
    one = launch(1, str(tmp_path / "w1.pt"), N, B, E)
    two = launch(2, str(tmp_path / "w2.pt"), N, B, E)
    assert two["world"] == 2 and one["world"] == 1
    # (one GPU: the one-block last mini-batch replays a single-step graph of its own; data parallel: host-launched)
    assert one["graphs"] == [(1, 1), (1, 2), (8, 1), (8, 2)] and two["graphs"] == [(4, 1), (4, 2)]
    assert one["noise_step"] == two["noise_step"] == E * 4 and one["opt_step"] == two["opt_step"] == E * 3
    # the all-reduced gradient of each epoch's LAST mini-batch (one block on rank 0, nothing on rank 1)
    for g1, g2 in zip(one["grads"], two["grads"]):
        scale = g1.abs().max().item()
        assert (g1 - g2).abs().max().item() < 2e-5 * scale
    # parameters after 6 Adam steps and the latent table after 2 sharded latent steps: Adam divides by sqrt(v), so an
    # entry whose gradient is pure rounding noise may move differently; everything else agrees to 1e-6
    dp = (one["flat_p"] - two["flat_p"]).abs()
    de = (one["emb"] - two["emb"]).abs()
    assert (dp > 1e-6).float().mean().item() < 1e-3 and dp.max().item() < 6 * 2e-3, (dp.max().item(), (dp > 1e-6).sum())
    # (latent table: lr_emb = 5e-3, two sharded latent steps; the two worlds sum their gradients in different orders, and an
    # entry's first Adam steps are lr * g / |g| (1 + O(rounding of g / g)): measured 0.4e-5 .. 1.1e-5 over this round's
    # kernels = 0.2 % of one step; the bound is 3 x that, not a sign flip's 5e-3)
    assert de.max().item() < 3e-5, de.max().item()
    # the epoch's log sums (engine.read_epoch_stats): focal terms, b_latent, b_net; the per-step accuracy RATIOS are
    # those of the whole mini-batch on both worlds, because the counts ride in the all-reduce of the gradients
    np.testing.assert_allclose(one["stats"][:, 0:5], two["stats"][:, 0:5], rtol=2e-4)
    np.testing.assert_allclose(one["stats"][:, 8:14], two["stats"][:, 8:14], atol=2e-3)   # a few voxels at p = 0.5
    np.testing.assert_allclose(one["stats"][:, 14:16], two["stats"][:, 14:16], rtol=2e-3, atol=2.0)
    assert (two["stats"][:, 7] == 3).all() and (two["stats"][:, 5:7] == 0).all()


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("collective", ["host", "graph"])
def test_two_ranks_rccl(tmp_path, collective):
    """BASELINE.json configs[3] on real hardware, the moment a box has two devices: two ranks over RCCL (backend "nccl",
    rank r on GPU r, the production engine and EpochDriver) against the one-rank run -- with the all-reduce launched from
    the host behind the step graph ("host", the default) and captured as a node of the step graph
    (NVF_GRAPH_COLLECTIVE=graph: 4-step and 1-step graphs replayed with peers).  Skips itself on one-GPU boxes: nothing in
    this repo has run RCCL with more than one rank yet (SCALE_r01-r04 were skipped), and this is the test that will."""
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices (RCCL refuses two ranks on one)")
    N, B, E = 17, 8, 2
    one = launch(1, str(tmp_path / "w1.pt"), N, B, E)
    two = launch(2, str(tmp_path / "w2.pt"), N, B, E, backend="nccl", extra_env={"NVF_GRAPH_COLLECTIVE": collective})
    assert two["world"] == 2 and two["graphs"] == [(4, 1), (4, 2)]
    assert one["noise_step"] == two["noise_step"] == E * 4 and one["opt_step"] == two["opt_step"] == E * 3
    for g1, g2 in zip(one["grads"], two["grads"]):
        assert (g1 - g2).abs().max().item() < 2e-5 * g1.abs().max().item()
    dp = (one["flat_p"] - two["flat_p"]).abs()
    de = (one["emb"] - two["emb"]).abs()
    assert (dp > 1e-6).float().mean().item() < 1e-3 and dp.max().item() < 6 * 2e-3, (dp.max().item(), (dp > 1e-6).sum())
    assert de.max().item() < 1e-5, de.max().item()
    np.testing.assert_allclose(one["stats"][:, 0:5], two["stats"][:, 0:5], rtol=2e-4)
    assert (two["stats"][:, 7] == 3).all() and (two["stats"][:, 5:7] == 0).all()


@pytest.mark.timeout(600)
def test_bench_gpus_2_launches_two_ranks_and_reports_the_live_world_size(tmp_path):
    """`python bench.py --gpus 2` with no torchrun environment: the script starts its two ranks itself (here over gloo,
    both on GPU 0 -- the numbers mean nothing, the path is the driver's N > 1 path: barriers, MAX over ranks, the
    sharded epoch), and rank 0's JSON line reports the size of the LIVE process group."""
    import json
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    env = dict(os.environ, PYTHONPATH=ROOT, NVF_DIST_BACKEND="gloo", NVF_DEVICE_OVERRIDE="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "12", "--warmup", "3",
                        "--epochs", "1", "--blocks", "61", "--distinct", "61", "--no-pmc", "--no-cpu-baseline",
                        "--sweep-blocks", "300", "--sustained-s", "0.2"],
                       env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 32 and d["config"]["parallelism"] == "dp2"
    assert d["scaling"] == "weak" and d["steps"] == 12 and d["value"] > 0 and np.isfinite(d["loss_last_step"])
    assert d["config"]["collective"] == "all-reduce launched from the host"
    # 61 blocks at a global mini-batch of 32: one full mini-batch and a short one of 29 (15 + 14 blocks)
    assert d["epoch"]["minibatches_per_epoch"] == 2 and d["epoch"]["blocks_per_s"] > 0
    # SURVEY 8(e) "report both": beside the latency-bound B = 16 / GPU line, the lines that keep every GPU busy --
    # batch 256 per GPU (weak), the full-batch latent step and a big latent step + eval sharded over the ranks (strong)
    sw = d["sweep"]
    assert sw["train_step_B256_per_gpu"]["global_batch"] == 512 and sw["train_step_B256_per_gpu"]["blocks_per_s"] > 0
    # ... and the strong-scaling line: the reference's own mini-batch of 16 split over the two ranks
    st = sw["train_step_B16_global_strong"]
    assert st["global_batch"] == 16 and st["blocks_per_gpu"] == 8 and st["blocks_per_s"] > 0
    assert "direct_form" in d and d["direct_form"]["blocks_per_s"] > 0 and d["sustained"]["steps"] > 0
    assert sw["latent_step_N61"]["blocks_per_s"] > 0
    assert sw["latent_step_N300"]["blocks_per_gpu"] == 150 and sw["eval_forward_N300"]["blocks_per_s"] > 0
    assert all(0 < v["frac_of_fp32_peak"] < 1 for v in sw.values())
