"""D1 / D2 geometry metrics on the sparse cell index (csrc/pc_sparse.hip, nvfpcc_amd.pc_metrics with `bits` / `index`):
bit for bit the dense 10-bit results, unchanged under translation into the 11- and 12-bit domains, exact against the
cKDTree oracle of tests/pc_metrics_ref.py at 12 bits (hyper-cell planes, the domain's corners, far clusters, ties),
and the built index itself against a numpy restatement of its layout."""
import argparse

import numpy as np
import pytest
import torch

from tests import pc_metrics_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def ellipsoid(seed, n_dir, radius=300.0, centre=(512.0, 512.0, 512.0), bits=10):
    """Bumpy ellipsoid shell (the surface of test_gpu_pc_metrics.ellipsoid) clipped to [0, 2^bits)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_dir, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    bump = 1.0 + 0.08 * np.sin(5 * d[:, 0]) * np.cos(4 * d[:, 1]) + 0.05 * np.sin(9 * d[:, 2])
    p = np.asarray(centre) + d * bump[:, None] * np.array([radius, 0.85 * radius, 1.2 * radius])
    return np.unique(np.clip(np.round(p), 0, (1 << bits) - 1).astype(np.int64), axis=0)


def thinned_jittered(p, seed, keep=0.7, jitter=2, bits=10):
    rng = np.random.default_rng(seed)
    q = p[rng.random(p.shape[0]) < keep] + rng.integers(-jitter, jitter + 1, size=(1, 3))
    q = q + rng.integers(-jitter, jitter + 1, size=q.shape) * (rng.random((q.shape[0], 1)) < 0.3)
    return rng.permutation(np.clip(q, 0, (1 << bits) - 1))


def check_nearest(query, target, bits=12):
    from nvfpcc_amd import pc_metrics
    idx, d2 = pc_metrics.nearest(query, target, bits=bits)
    want_i, want_d = R.nearest(query, target)
    assert np.array_equal(d2, want_d)
    assert np.array_equal(idx, want_i)
    return idx, d2


KS = (3, 12, 32)


def results(a, b, **kw):
    """Everything the metrics give for the pair (a, b), as numpy arrays and one dictionary."""
    from nvfpcc_amd import pc_metrics
    out = {"ab": pc_metrics.nearest(a, b, **kw), "ba": pc_metrics.nearest(b, a, **kw)}
    for k in KS:
        out[k] = pc_metrics.estimate_normals(a, k=k, return_knn=True, **kw)
    return out


def assert_same(got, want):
    for key in ("ab", "ba"):
        assert np.array_equal(got[key][1], want[key][1]), f"{key}: squared distances"
        assert np.array_equal(got[key][0], want[key][0]), f"{key}: indices"
    for k in KS:
        assert np.array_equal(got[k][1], want[k][1]), f"k = {k}: k-NN sets"
        assert np.array_equal(got[k][0].view(np.uint32), want[k][0].view(np.uint32)), f"k = {k}: normal bits"


@pytest.fixture(scope="module")
def pair10():
    """(a, b, the dense 10-bit results): computed once, read by the tests below."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    a = ellipsoid(1, 33_000)
    b = thinned_jittered(a, 2)
    assert 28_000 < a.shape[0] < 33_000
    return a, b, results(a, b, index="dense")


@pytest.mark.timeout(300)
def test_sparse_equals_dense_at_ten_bits(pair10):
    from nvfpcc_amd import pc_metrics
    a, b, dense = pair10
    assert_same(results(a, b, index="sparse"), dense)
    assert pc_metrics.geometry_psnr(a, b, index="sparse") == pc_metrics.geometry_psnr(a, b, index="dense")
    assert pc_metrics.geometry_psnr(a, b, bits=10, index="sparse") == pc_metrics.geometry_psnr(a, b)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("offset,bits", [((1032, 2056, 3000), 12), ((1024, 0, 8), 11)])
def test_translation_into_a_deeper_domain_changes_nothing(pair10, offset, bits):
    # whole cells, but not whole super- or hyper-cells: the hierarchy meets the cloud differently, the cells do not
    a, b, dense = pair10
    off = np.asarray(offset)
    assert (a + off).max() < 1 << bits and (off % 8 == 0).all()
    assert_same(results(a + off, b + off, bits=bits), dense)


@pytest.mark.timeout(300)
def test_nearest_across_every_hyper_cell_plane():
    a = ellipsoid(3, 46_000, radius=1200.0, centre=(2048.0, 2048.0, 2048.0), bits=12)
    b = thinned_jittered(a, 4, bits=12)
    assert 38_000 < a.shape[0] and a[:, 2].min() < 1024 and a[:, 2].max() >= 3584   # z: planes 1024 .. 3584 crossed
    check_nearest(a, b)
    check_nearest(b, a)


@pytest.mark.timeout(300)
def test_single_point_target_and_the_corners_of_the_twelve_bit_domain():
    rng = np.random.default_rng(5)
    corners = np.array([[x, y, z] for x in (0, 4095) for y in (0, 4095) for z in (0, 4095)])
    uniform = rng.integers(0, 4096, size=(5000, 3))
    query = np.concatenate([corners, uniform])
    idx, d2 = check_nearest(query, np.array([[4095, 0, 4095]]))
    assert not idx.any() and d2.max() == 3 * 4095 ** 2                  # the largest distance the domain holds
    check_nearest(corners, uniform)
    check_nearest(uniform, corners)


@pytest.mark.timeout(300)
def test_far_clusters_resolve_exactly():
    a = ellipsoid(6, 5_500, radius=40.0, centre=(200.0, 200.0, 260.0), bits=12)
    b = ellipsoid(7, 5_500, radius=40.0, centre=(3900.0, 3800.0, 3850.0), bits=12)
    assert 4_000 < a.shape[0] < 5_500
    both = np.concatenate([a, b[: b.shape[0] // 10]])
    check_nearest(a, b)                                              # every query ~ 6 000 voxels from any target
    check_nearest(both, b)
    check_nearest(b, a)
    check_nearest(both, a)


@pytest.mark.timeout(300)
def test_target_with_empty_blocks():
    a = ellipsoid(8, 40_000, radius=700.0, centre=(2048.0, 2040.0, 2100.0), bits=12)
    blk = a // 32
    drop = (blk[:, 0] + 3 * blk[:, 1] + 7 * blk[:, 2]) % 5 == 0     # whole 32^3 blocks removed, as a decoder may
    assert 0.1 < drop.mean() < 0.4
    check_nearest(a, a[~drop])
    check_nearest(a[~drop], a)


@pytest.mark.timeout(300)
def test_duplicate_targets_tie_to_the_lowest_index():
    rng = np.random.default_rng(4)
    base = rng.integers(3000, 3040, size=(3000, 3))
    target = np.concatenate([base, base[::-1], base[:500]])          # every point at least twice, in shuffled order
    query = rng.integers(2990, 3050, size=(20_000, 3))
    idx, _ = check_nearest(query, target)
    assert (idx < base.shape[0]).all()                               # every distance is first reached in `base`
    idx, d2 = check_nearest(np.array([[10, 10, 3010]]), np.array([[10, 10, 3020], [10, 10, 3000]]))
    assert idx[0] == 0 and d2[0] == 100


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", [3, 32])
def test_knn_sets_and_normals_at_twelve_bits(k):
    from nvfpcc_amd import pc_metrics
    a = np.random.default_rng(9).permutation(
        ellipsoid(9, 15_500, radius=600.0, centre=(2048.0, 2050.0, 2040.0), bits=12))
    assert 14_000 < a.shape[0]
    normals, knn = pc_metrics.estimate_normals(a, k=k, return_knn=True, bits=12)
    want, _ = R.ordered_neighbours(a, a, k)
    assert np.array_equal(knn, want)
    ref, gap = R.pca_normals(a, want)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)
    ok = gap > 1e-3
    dot = np.abs((normals.astype(np.float64) * ref).sum(1))
    print(f"k = {k}: {np.count_nonzero(~ok)} of {a.shape[0]} points excluded (relative eigen-gap <= 1e-3)")
    assert ok.mean() > 0.5
    assert dot[ok].min() >= 1 - 1e-6


@pytest.mark.timeout(300)
def test_knn_of_twelve_points_spread_over_the_domain_is_the_whole_cloud():
    from nvfpcc_amd import pc_metrics
    rng = np.random.default_rng(10)
    a = np.concatenate([np.array([[0, 0, 0], [4095, 4095, 4095], [4095, 0, 17], [5, 4090, 2048]]),
                        rng.integers(0, 4096, size=(8, 3))])
    assert a.shape[0] == 12
    _, knn = pc_metrics.estimate_normals(a, k=12, return_knn=True, bits=12)
    want, _ = R.ordered_neighbours(a, a, 12)
    assert np.array_equal(np.sort(want, 1), np.tile(np.arange(12), (12, 1)))
    assert np.array_equal(knn, want)                                 # in (d2, index) order


@pytest.mark.timeout(300)
def test_geometry_psnr_at_twelve_bits_against_the_oracle():
    from nvfpcc_amd import pc_metrics
    a = ellipsoid(11, 40_000, radius=900.0, centre=(2048.0, 2048.0, 2048.0), bits=12)
    b = thinned_jittered(a, 12, bits=12)
    r = pc_metrics.geometry_psnr(a, b, bits=12)
    normals = pc_metrics.estimate_normals(a, bits=12)
    want = R.geometry_psnr(a, b, normals.astype(np.float32).astype(np.float64), peak=4095)
    for key in ("ref_to_test", "test_to_ref"):
        assert r[key]["d1_mse"] == want[key]["d1_mse"]                 # sums of integers: exact
        assert r[key]["hausdorff_d2"] == want[key]["hausdorff_d2"]
        assert abs(r[key]["d2_mse"] - want[key]["d2_mse"]) <= 1e-9 * want[key]["d2_mse"]
    assert r["d1_mse"] == want["d1_mse"] and r["d1_psnr"] == want["d1_psnr"]    # peak defaults to 4095
    assert (r["n_ref"], r["n_test"]) == (a.shape[0], b.shape[0])
    assert r == pc_metrics.geometry_psnr(a, b, bits=12)                # bit-identical on a second call
    assert r == pc_metrics.geometry_psnr(a, b, bits=12, peak=4095)


def numpy_index(p, bits):
    """The layout of NvfPcSparseIndex (include/nvf_hip.h), restated."""
    hb = bits - 9
    key9 = lambda v: ((v[:, 0] & 7) << 6) | ((v[:, 1] & 7) << 3) | (v[:, 2] & 7)
    h = p >> 9
    key = (((h[:, 0] << (2 * hb)) | (h[:, 1] << hb) | h[:, 2]) << 18) | (key9(p >> 6) << 9) | key9(p >> 3)
    order = np.argsort(key, kind="stable")
    cell_key, counts = np.unique(key, return_counts=True)
    supers, first = np.unique(cell_key >> 9, return_index=True)
    mask = np.zeros((supers.size, 8), np.uint64)
    for ck in cell_key:
        c = int(ck) & 511
        mask[np.searchsorted(supers, ck >> 9), c >> 6] |= np.uint64(1 << (c & 63))
    super_table = np.full(1 << (3 * (bits - 6)), -1, np.int64)
    super_table[supers] = np.arange(supers.size)
    hyper_table = np.zeros(1 << (3 * hb), np.int64)
    hyper_table[np.unique(cell_key >> 18)] = 1
    return {"sorted": np.concatenate([p, np.arange(p.shape[0])[:, None]], 1)[order],
            "start": np.concatenate([[0], np.cumsum(counts)]), "mask": mask, "first": first,
            "super_table": super_table, "hyper_table": hyper_table}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("bits", [10, 12])
def test_the_built_index_is_the_documented_layout(bits):
    from nvfpcc_amd import pc_metrics
    top = (1 << bits) - 1
    rng = np.random.default_rng(13)
    p = np.concatenate([ellipsoid(13, 1_600, radius=30.0, centre=(100.0, 120.0, 90.0), bits=bits),
                        ellipsoid(14, 1_600, radius=45.0, centre=(top - 500.0, top - 60.0, 530.0), bits=bits),
                        np.array([[0, 0, 0], [top, top, top], [top, 0, 511], [512, 511, 0]])])
    p = rng.permutation(p)
    assert 2_500 < p.shape[0] < 3_500
    want = numpy_index(p, bits)
    if bits == 12:
        assert want["hyper_table"].sum() < 0.05 * want["hyper_table"].size
    c = pc_metrics._SparseCloud(pc_metrics._points(p, "p", bits), torch.device("cuda"), bits)
    got = {"sorted": c.sorted, "start": c.start, "first": c.first, "super_table": c.super_table,
           "hyper_table": c.hyper_table}
    for name, t in got.items():
        assert np.array_equal(t.cpu().numpy().astype(np.int64), want[name]), name
    assert np.array_equal(c.mask.cpu().numpy().view(np.uint64), want["mask"])
    again = pc_metrics._SparseCloud(pc_metrics._points(p[::-1].copy(), "p", bits), torch.device("cuda"), bits)
    assert torch.equal(again.mask, c.mask) and torch.equal(again.first, c.first)      # any input order
    assert torch.equal(again.super_table, c.super_table) and torch.equal(again.start, c.start)


@pytest.mark.timeout(300)
def test_print_pc_error_and_the_pc_error_tool_at_deeper_domains(tmp_path, capsys):
    import NVFPCC
    from nvfpcc_amd import pc_error, pc_metrics
    from nvfpcc_amd.recon import write_ply_ascii
    a = ellipsoid(15, 12_000, radius=500.0, centre=(1024.0, 1000.0, 1030.0), bits=11)
    b = thinned_jittered(a, 16, bits=11)
    assert a.max() >= 1024
    ref_ply, test_ply = str(tmp_path / "ref.ply"), str(tmp_path / "test.ply")
    write_ply_ascii(ref_ply, a)
    write_ply_ascii(test_ply, b)
    capsys.readouterr()
    NVFPCC._print_pc_error(argparse.Namespace(ref_ply=ref_ply), b, "cuda", bits=11)
    want = pc_metrics.geometry_psnr(a, b, bits=11)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[PCError]")]
    assert lines == ["[PCError] D1 PSNR: %.4f D2 PSNR: %.4f" % (want["d1_psnr"], want["d2_psnr"])]
    assert want["d1_psnr"] == R.psnr(want["d1_mse"], 2047.0)
    assert pc_error.main([ref_ply, test_ply, "--bits", "12"]) == 0
    out = capsys.readouterr().out
    assert "peak: 4095 " in out
    r12 = pc_metrics.geometry_psnr(a, b, bits=12)
    assert f"mseF,PSNR (p2point): {r12['d1_psnr']:.6g}" in out
    assert pc_error.main([ref_ply, test_ply]) == 1                    # 10 bits by default: out of range
