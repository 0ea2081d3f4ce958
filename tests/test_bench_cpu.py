"""bench.py without a GPU: what a plain run is asked to do, and how --dump-outputs writes what the timed path computed."""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_measures_the_headline_only():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.repeats is None                      # one timed region unless --full (three) or --repeats says otherwise
    f = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert f.full and f.dump_outputs == "out"


def test_outputs_are_written_as_float32_or_float64(tmp_path):
    arrays = {"p2": torch.rand(4, 1, 8, 8, 8), "loss": np.array([1.5], np.float64),
              "bits": np.arange(7, dtype=np.int32), "h": np.ones((3, 2), np.float16)}
    n = bench.write_outputs(str(tmp_path / "d"), arrays)
    got = {k: np.load(os.path.join(tmp_path, "d", k + ".npy")) for k in arrays}
    assert got["p2"].dtype == np.float32 and np.array_equal(got["p2"], arrays["p2"].numpy())
    assert got["loss"].dtype == np.float64 and got["loss"][0] == 1.5
    assert got["bits"].dtype == np.float32 and np.array_equal(got["bits"], np.arange(7))
    assert got["h"].dtype == np.float32
    assert n == sum(v.nbytes for v in got.values())


def test_large_per_block_outputs_keep_the_same_sample_of_blocks(tmp_path):
    x = np.arange(300 * 5, dtype=np.float32).reshape(300, 5)
    flat = np.arange(1000, dtype=np.float32)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"x": x, "flat": flat}, max_blocks=16)
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (16, 5) and np.array_equal(a, b)
    rows = a[:, 0] / 5                                  # rows of x, sorted, without repeats
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, x[rows.astype(int)])
    assert np.array_equal(np.load(tmp_path / "a" / "flat.npy"), flat)      # one-dimensional: never sampled


def test_outputs_over_the_limit_are_refused(tmp_path):
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "d"), {"x": np.zeros(1000, np.float32)}, limit=1000)
    assert not os.path.exists(tmp_path / "d" / "x.npy")
