"""D1 / D2 geometry metrics on the GPU (nvfpcc_amd.pc_metrics) against the cKDTree + numpy oracle of
tests/pc_metrics_ref.py: exact 1-NN (index and squared distance, ties to the lowest input index), exact k-NN sets,
PCA normals, the error sums, and the `[PCError]` line of `NVFPCC.py decode --ref_ply`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pc_metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def ellipsoid(seed, n_dir, radius=300.0, centre=(512.0, 512.0, 512.0)):
    """Bumpy ellipsoid shell, 10-bit coordinates (tools/rd_sweep.make_cloud's surface, any centre)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_dir, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    bump = 1.0 + 0.08 * np.sin(5 * d[:, 0]) * np.cos(4 * d[:, 1]) + 0.05 * np.sin(9 * d[:, 2])
    p = np.asarray(centre) + d * bump[:, None] * np.array([radius, 0.85 * radius, 1.2 * radius])
    return np.unique(np.clip(np.round(p), 0, 1023).astype(np.int64), axis=0)


def thinned_jittered(p, seed, keep=0.7, jitter=2):
    rng = np.random.default_rng(seed)
    q = p[rng.random(p.shape[0]) < keep] + rng.integers(-jitter, jitter + 1, size=(1, 3))
    q = q + rng.integers(-jitter, jitter + 1, size=q.shape) * (rng.random((q.shape[0], 1)) < 0.3)
    return rng.permutation(np.clip(q, 0, 1023))


def check_nearest(query, target):
    from nvfpcc_amd import pc_metrics
    idx, d2 = pc_metrics.nearest(query, target)
    want_i, want_d = R.nearest(query, target)
    assert np.array_equal(d2, want_d)
    assert np.array_equal(idx, want_i)
    return idx, d2


@pytest.mark.timeout(300)
def test_nearest_on_ellipsoid_surfaces():
    a = ellipsoid(1, 110_000)
    b = thinned_jittered(a, 2)
    assert a.shape[0] > 90_000
    check_nearest(a, b)
    check_nearest(b, a)


@pytest.mark.timeout(300)
def test_nearest_of_a_cloud_in_itself_is_itself():
    a = np.random.default_rng(3).permutation(ellipsoid(3, 30_000))
    idx, d2 = check_nearest(a, a)
    assert not d2.any() and np.array_equal(idx, np.arange(a.shape[0]))


@pytest.mark.timeout(300)
def test_duplicate_targets_tie_to_the_lowest_index():
    rng = np.random.default_rng(4)
    base = rng.integers(100, 140, size=(3000, 3))
    target = np.concatenate([base, base[::-1], base[:500]])          # every point at least twice, in shuffled order
    query = rng.integers(90, 150, size=(20_000, 3))
    idx, _ = check_nearest(query, target)
    assert (idx < base.shape[0]).all()                               # every distance is first reached in `base`
    # an equidistant pair: query between two targets, the lower index wins whichever sits first in the cells
    idx, d2 = check_nearest(np.array([[10, 10, 10]]), np.array([[10, 10, 20], [10, 10, 0]]))
    assert idx[0] == 0 and d2[0] == 100


@pytest.mark.timeout(300)
def test_single_point_target_and_the_domain_corners():
    rng = np.random.default_rng(5)
    corners = np.array([[x, y, z] for x in (0, 1023) for y in (0, 1023) for z in (0, 1023)])
    query = np.concatenate([corners, rng.integers(0, 1024, size=(5000, 3))])
    idx, d2 = check_nearest(query, np.array([[1023, 0, 1023]]))
    assert not idx.any() and d2.max() == 3 * 1023 ** 2                # the largest distance the domain holds
    check_nearest(query, corners)
    check_nearest(corners, query)


@pytest.mark.timeout(300)
def test_far_clusters_resolve_exactly():
    a = ellipsoid(6, 20_000, radius=40.0, centre=(60.0, 60.0, 70.0))
    b = ellipsoid(7, 20_000, radius=40.0, centre=(960.0, 900.0, 950.0))
    both = np.concatenate([a, b[: b.shape[0] // 10]])
    check_nearest(a, b)                                              # every query ~ 900 voxels from any target
    check_nearest(both, b)
    check_nearest(b, a)


@pytest.mark.timeout(300)
def test_target_with_empty_blocks():
    a = ellipsoid(8, 60_000)
    blk = a // 32
    drop = (blk[:, 0] + 3 * blk[:, 1] + 7 * blk[:, 2]) % 5 == 0     # whole 32^3 blocks removed, as a decoder may
    assert 0.1 < drop.mean() < 0.4
    check_nearest(a, a[~drop])
    check_nearest(a[~drop], a)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [3, 12, 32])
def test_knn_sets_and_normals(k):
    from nvfpcc_amd import pc_metrics
    a = np.random.default_rng(9).permutation(ellipsoid(9, 25_000))
    normals, knn = pc_metrics.estimate_normals(a, k=k, return_knn=True)
    want, _ = R.ordered_neighbours(a, a, k)
    assert np.array_equal(knn, want)
    ref, gap = R.pca_normals(a, want)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)
    ok = gap > 1e-3
    dot = np.abs((normals.astype(np.float64) * ref).sum(1))
    print(f"k = {k}: {np.count_nonzero(~ok)} of {a.shape[0]} points excluded (relative eigen-gap <= 1e-3)")
    assert ok.mean() > 0.5
    assert dot[ok].min() >= 1 - 1e-6


def _oracle_with(a, b, normals):
    return R.geometry_psnr(a, b, normals.astype(np.float32).astype(np.float64))


@pytest.mark.timeout(600)
def test_geometry_psnr_against_the_oracle():
    from nvfpcc_amd import pc_metrics
    a = ellipsoid(10, 60_000)
    b = thinned_jittered(a, 11)
    r = pc_metrics.geometry_psnr(a, b)
    normals = pc_metrics.estimate_normals(a)
    want = _oracle_with(a, b, normals)
    for key in ("ref_to_test", "test_to_ref"):
        assert r[key]["d1_mse"] == want[key]["d1_mse"]                 # sums of integers: exact
        assert r[key]["hausdorff_d2"] == want[key]["hausdorff_d2"]
        assert abs(r[key]["d2_mse"] - want[key]["d2_mse"]) <= 1e-9 * want[key]["d2_mse"]
    assert r["d1_mse"] == want["d1_mse"] and r["d1_psnr"] == want["d1_psnr"]
    assert abs(r["d2_psnr"] - want["d2_psnr"]) < 1e-8
    assert (r["n_ref"], r["n_test"]) == (a.shape[0], b.shape[0])
    assert r == pc_metrics.geometry_psnr(a, b)                         # bit-identical on a second call
    d1 = pc_metrics.geometry_psnr(a, b, d2=False)
    assert d1["d1_mse"] == r["d1_mse"] and d1["d2_mse"] is None
    same = pc_metrics.geometry_psnr(a, a)
    assert same["d1_mse"] == 0 and same["d1_psnr"] == float("inf") and same["d2_psnr"] == float("inf")


@pytest.mark.timeout(600)
def test_normals_from_the_ply_are_honoured(tmp_path):
    from nvfpcc_amd import pc_error, pc_metrics
    a = ellipsoid(12, 20_000)
    b = thinned_jittered(a, 13)
    rng = np.random.default_rng(14)
    n = rng.normal(size=a.shape)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    ref_ply = tmp_path / "ref.ply"
    with open(ref_ply, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {a.shape[0]}\nproperty float nx\nproperty float ny\n"
                "property float nz\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for p, v in zip(a, n):
            f.write(f"{v[0]:.7f} {v[1]:.7f} {v[2]:.7f} {p[0]} {p[1]} {p[2]}\n")
    xyz, normals = pc_metrics.read_ply_points(str(ref_ply))
    assert np.array_equal(xyz, a)
    r = pc_metrics.geometry_psnr(xyz, b, ref_normals=normals)
    want = _oracle_with(a, b, normals)
    assert abs(r["d2_mse"] - want["d2_mse"]) <= 1e-9 * want["d2_mse"]
    assert r["d2_mse"] != pc_metrics.geometry_psnr(a, b)["d2_mse"]    # not the estimated normals
    test_ply = tmp_path / "test.ply"
    from nvfpcc_amd.recon import write_ply_ascii
    write_ply_ascii(str(test_ply), b)
    out = subprocess.run([sys.executable, "-m", "nvfpcc_amd.pc_error", str(ref_ply), str(test_ply)], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert f"mseF,PSNR (p2point): {r['d1_psnr']:.6g}" in out.stdout
    assert f"mseF,PSNR (p2plane): {r['d2_psnr']:.6g}" in out.stdout
    assert pc_error.main([str(ref_ply), str(test_ply), "--no-d2"]) == 0


@pytest.mark.timeout(900)
def test_cli_decode_prints_pc_error_only_with_ref_ply(tmp_path, golden_dir):
    import shutil
    from tests.test_gpu_trained import golden_points
    from tests.test_trained_golden import CFG, load_pack
    from nvfpcc_amd import pc_metrics
    from nvfpcc_amd.recon import write_ply_ascii
    _, G = load_pack(golden_dir, "S")
    ref, test = golden_points(G, 0.64), golden_points(G, 0.6)
    cwd = str(tmp_path)
    write_ply_ascii(os.path.join(cwd, "ref.ply"), ref)
    shutil.copy(os.path.join(golden_dir, "trained_S_pack.pk"), os.path.join(cwd, "pack.pk"))
    ch, channels = CFG["S"]
    cmd = [sys.executable, os.path.join(ROOT, "NVFPCC.py"), "decode", "pack.pk", "--batchsize", "1", "--thh", "0.6",
           "--N", str(G["latents"].shape[0]), "--chanstr", ",".join(map(str, channels)), "--ch", str(ch)]
    run = lambda extra: subprocess.run(cmd + extra, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT),
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    r = run(["--ref_ply", "ref.ply"])
    assert r.returncode == 0, r.stdout[-3000:]
    want = _oracle_with(ref, test, pc_metrics.estimate_normals(ref))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[PCError]")]
    assert lines == ["[PCError] D1 PSNR: %.4f D2 PSNR: %.4f" % (want["d1_psnr"], want["d2_psnr"])]
    plain = run([])
    assert plain.returncode == 0, plain.stdout[-3000:]
    assert "[PCError]" not in plain.stdout
