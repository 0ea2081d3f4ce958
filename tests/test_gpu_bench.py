"""A plain `bench.py --gpus 1 --steps K --warmup W` run: exactly K timed steps, the headline line without the --full
objects, and --dump-outputs files that two runs with the same arguments write identically."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "sustained", "direct_form", "epoch", "sweep", "cpu_baseline")


def plain_run(tmp_path, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3",
                        "--blocks", "61", "--distinct", "61", "--dump-outputs", str(out)],
                       env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_bench_run_times_k_steps_and_dumps_the_same_outputs_twice(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    d = plain_run(tmp_path, tmp_path / "o1")
    assert d["steps"] == 12 and d["warmup"] == 3 and d["unit"] == "blocks/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["metric"].startswith("leaf-blocks/sec NVF train step")
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(16 * 1e3 / d["ms_per_step"], rel=1e-3)
    assert len(d["repeats"]["ms_per_step"]) == 1 and np.isfinite(d["loss_last_step"])
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    names = {"p0", "p1", "p2", "loss_terms", "latent_bits", "net_bits", "loss", "params", "grads", "adam_m", "adam_v",
             "latents"}
    assert {f[:-4] for f in os.listdir(tmp_path / "o1")} == names
    one = {n: np.load(tmp_path / "o1" / (n + ".npy")) for n in names}
    assert sum(x.nbytes for x in one.values()) <= 64 * 2 ** 20
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in one.values())
    assert one["p2"].shape == (16, 1, 32, 32, 32) and one["p1"].shape == (16, 1, 16, 16, 16)
    assert one["latents"].shape == (61, 3, 2, 2, 2) and one["loss"][0] == pytest.approx(d["loss_last_step"], abs=1e-3)
    # the same arguments: the same inputs, the same kernels -- the same outputs
    plain_run(tmp_path, tmp_path / "o2")
    for n in names:
        assert np.array_equal(np.load(tmp_path / "o2" / (n + ".npy")), one[n]), n
