"""The voxeliser on the device (nvfpcc_amd/voxelize.py, csrc/voxelize.hip) against its numpy restatement
(tests/voxelize_ref.py).  points, counts, M and max_err2 are compared exactly.  sum_err2 is compared within P * 2^-52
relative: every term is non-negative, so any order of summing P of them lands within (P - 1) roundings of 2^-53 each of
the exact sum, and so do two orders within P * 2^-52 of each other; the order is the device's own, not numpy's."""
import numpy as np
import pytest
import torch

from nvfpcc_amd import voxelize as vx
from tests import voxelize_ref as R

pytestmark = pytest.mark.gpu

O_NEG = (-3.2, 1e3, 7.5)
STEP = 0.0137


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def cloud(n, bits, origin=O_NEG, step=STEP, seed=0, cells=None, dtype=np.float64):
    """n points o + q s + j s, |j| <= 0.25, on `cells` distinct random cells (n // 2 + 1 when None: duplicates)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << bits, size=(cells or n // 2 + 1, 3))
    q = pool[rng.integers(0, len(pool), size=n)]
    x = np.asarray(origin) + (q + rng.uniform(-0.25, 0.25, size=(n, 3))) * step
    return x.astype(dtype).astype(np.float64), q


def check(points, bits=10, lattice=None):
    """voxelize on the device against the reference; -> (device result, reference result)."""
    ref = R.voxelize(points, bits, lattice)
    got = vx.voxelize(points, "cuda", bits=bits, lattice=None if lattice is None else vx.Lattice(*lattice))
    assert got.points.dtype == torch.int32 and got.counts.dtype == torch.int32 and got.points.is_cuda
    assert got.points.shape == (len(ref.points), 3) and got.counts.shape == (len(ref.points),)      # M
    assert np.array_equal(got.points.cpu().numpy(), ref.points)
    assert np.array_equal(got.counts.cpu().numpy(), ref.counts)
    assert got.n_in == ref.n_in == len(points) == int(got.counts.sum().item())
    assert got.max_err2 == ref.max_err2
    print("sum_err2", got.sum_err2, ref.sum_err2)
    assert abs(got.sum_err2 - ref.sum_err2) <= len(points) * 2.0 ** -52 * ref.sum_err2
    assert got.lattice.bits == ref.lattice.bits
    assert got.lattice.origin == tuple(ref.lattice.origin) and got.lattice.step == ref.lattice.step      # by value
    return got, ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 100003])
def test_explicit_lattice_at_every_size(n):
    need_gpu()
    x, _ = cloud(n, 10, seed=n)
    got, ref = check(x, lattice=(10, O_NEG, STEP))
    assert len(ref.points) < n or n == 1          # the cloud holds duplicates


@pytest.mark.parametrize("n", [1, 65, 1025, 100003])
def test_fitted_lattice_equals_the_references_fit(n):
    need_gpu()
    x, _ = cloud(n, 10, seed=100 + n)
    got, ref = check(x, bits=10)
    assert got.points.min().item() >= 0 and got.points.max().item() <= 1023


def test_all_points_equal_is_one_voxel_with_step_one():
    need_gpu()
    x = np.tile(np.array([[-0.0, 12.5, -7.25]]), (300, 1))
    got, _ = check(x, bits=11)
    assert got.points.cpu().tolist() == [[0, 0, 0]] and got.counts.cpu().tolist() == [300]
    assert got.lattice.step == 1.0 and got.max_err2 == 0.0
    assert got.lattice.origin == (0.0, 12.5, -7.25) and np.signbit(got.lattice.origin[0]) == False   # noqa: E712


@pytest.mark.parametrize("copies", [700, 3000])
def test_a_run_of_duplicates_between_two_other_points(copies):
    """700 copies: longer than a 256-thread workgroup; 3000: longer than the 1024 keys one workgroup of the unique pass
    spans, so the run's head and tail lie two workgroups apart with a whole one in between."""
    need_gpu()
    lat = (10, (0.0, 0.0, 0.0), 1.0)
    x = np.concatenate([[[1.0, 2.0, 3.0]], np.tile([[500.2, 17.0, 900.9]], (copies, 1)), [[1023.0, 1023.0, 1023.0]]])
    x = x[np.random.default_rng(3).permutation(len(x))]
    got, _ = check(x, lattice=lat)
    assert got.points.cpu().tolist() == [[1, 2, 3], [500, 17, 901], [1023, 1023, 1023]]
    assert got.counts.cpu().tolist() == [1, copies, 1]


@pytest.mark.parametrize("before, run", [(1000, 100), (1023, 2), (1024, 5), (2040, 1100)])
def test_a_run_that_straddles_a_workgroup_boundary_of_the_unique_pass(before, run):
    """`before` distinct points with smaller keys, then `run` copies of one: the run covers the sorted positions
    before .. before + run - 1, across position 1024 (and 2048, 3072), where one workgroup's keys end."""
    need_gpu()
    lat = (10, (0.0, 0.0, 0.0), 1.0)
    low = np.stack([np.zeros(before), np.arange(before) // 1024, np.arange(before) % 1024], 1)
    x = np.concatenate([low, np.tile([[7.0, 7.0, 7.0]], (run, 1)), [[9.0, 0.0, 0.0], [9.0, 0.0, 1.0]]])
    x = x[np.random.default_rng(before).permutation(len(x))]
    got, _ = check(x, lattice=lat)
    assert got.counts.cpu().tolist() == [1] * before + [run, 1, 1]


@pytest.mark.parametrize("bits", [10, 11, 12])
@pytest.mark.parametrize("origin, step", [(O_NEG, STEP), ((1e3, -1e3, 999.999), 1.0 / 3), ((-512.0, 0.0, 77.0), 2.0 ** -4),
                                          ((0.1, 0.2, 0.3), 1e-3)])
def test_every_bit_depth_reaches_both_ends_of_every_axis(bits, origin, step):
    need_gpu()
    top = (1 << bits) - 1
    x, _ = cloud(3000, bits, origin, step, seed=bits)
    ends = np.array([[0, 0, 0], [top, top, top], [top, 0, 0], [0, top, 0], [0, 0, top], [top, top, 0]], np.float64)
    x = np.concatenate([x, np.asarray(origin) + ends * step])
    got, ref = check(x, lattice=(bits, origin, step))
    p = got.points.cpu().numpy()
    assert p.min(0).tolist() == [0, 0, 0] and p.max(0).tolist() == [top, top, top]
    key = (p[:, 0].astype(np.int64) << (2 * bits)) | (p[:, 1].astype(np.int64) << bits) | p[:, 2]
    assert np.all(np.diff(key) > 0) and (bits == 10 or key.max() >= 1 << 32)


def test_float32_inputs_are_widened_exactly():
    need_gpu()
    x, q = cloud(5000, 10, dtype=np.float32)
    got = vx.voxelize(x.astype(np.float32), "cuda", lattice=vx.Lattice(10, O_NEG, STEP))
    ref = R.voxelize(x, 10, (10, O_NEG, STEP))
    assert np.array_equal(got.points.cpu().numpy(), ref.points) and np.array_equal(ref.points, np.unique(q, axis=0))
    assert got.max_err2 == ref.max_err2


def test_non_finite_points_raise_with_count_and_first_index():
    need_gpu()
    x, _ = cloud(2000, 10)
    for lattice in (None, vx.Lattice(10, O_NEG, STEP)):
        bad = x.copy()
        bad[0, 1] = np.nan
        bad[-1, 2] = np.inf
        bad[777, 0] = -np.inf
        with pytest.raises(ValueError, match=r"3 of 2000 points are not finite \(the first is point 0\)"):
            vx.voxelize(bad, "cuda", lattice=lattice)
        bad = x.copy()
        bad[-1, 2] = np.inf
        with pytest.raises(ValueError, match=r"1 of 2000 points are not finite \(the first is point 1999\)"):
            vx.voxelize(bad, "cuda", lattice=lattice)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("side", [-1, 1])
def test_points_outside_a_given_lattice_raise_with_count_and_first_index(axis, side):
    need_gpu()
    lat = vx.Lattice(11, O_NEG, STEP)
    x, _ = cloud(1500, 11)
    for at, q in ((1234, -0.5000001 if side < 0 else 2047.5000001), (40, -3.0 if side < 0 else 5000.0)):
        x[at, axis] = O_NEG[axis] + q * STEP
    nonfinite, outside, _ = R.classify(x, R.RefLattice(*lat))
    assert not nonfinite.any() and np.flatnonzero(outside).tolist() == [40, 1234]
    with pytest.raises(ValueError, match=r"2 of 1500 points lie outside the lattice of 11 bits.*\(the first is point 40\)"):
        vx.voxelize(x, "cuda", lattice=lat)
    # the last values still inside on that side
    x[40, axis] = O_NEG[axis] + (0.0 if side < 0 else 2047.0) * STEP
    x[1234, axis] = O_NEG[axis] + (-0.25 if side < 0 else 2047.25) * STEP
    check(x, lattice=lat)


def test_to_source_is_the_references_and_voxelize_inverts_it():
    need_gpu()
    for bits, origin, step in ((10, O_NEG, STEP), (11, (1e3, -1e3, 999.999), 1.0 / 3), (12, (0.1, 0.2, 0.3), 1e-3)):
        lat = vx.Lattice(bits, origin, step)
        q = np.unique(np.random.default_rng(bits).integers(0, 1 << bits, size=(20000, 3)), axis=0)
        src = vx.to_source(q, lat, "cuda")
        assert src.dtype == torch.float64 and src.is_cuda
        assert np.array_equal(src.cpu().numpy().view(np.int64), R.to_source(q, lat).view(np.int64))      # bit for bit
        coarse = vx.to_source(q >> 1, lat, "cuda", level=1)
        assert np.array_equal(coarse.cpu().numpy(), R.to_source(q >> 1, R.RefLattice(bits, origin, 2 * step)))
        back = vx.voxelize(src, "cuda", lattice=lat)
        key = (q[:, 0] << (2 * bits)) | (q[:, 1] << bits) | q[:, 2]
        assert np.array_equal(back.points.cpu().numpy(), q[np.argsort(key)])
        assert back.counts.cpu().unique().tolist() == [1]


def test_voxelize_then_preprocess_equals_preprocess_of_the_references_voxels():
    need_gpu()
    from nvfpcc_amd import preprocess as pp
    rng = np.random.default_rng(5)
    q = np.concatenate([c + rng.integers(0, 40, size=(600, 3)) for c in ((100, 200, 300), (600, 40, 900), (1000, 1000, 0))])
    q = q.clip(0, 1023)
    x = np.asarray(O_NEG) + (q + rng.uniform(-0.25, 0.25, size=q.shape)) * STEP
    x = np.concatenate([x, x[::10]])[rng.permutation(len(x) + len(x[::10]))]
    lat = (10, O_NEG, STEP)
    got = vx.voxelize(x, "cuda", lattice=vx.Lattice(*lat))
    ref = R.voxelize(x, 10, lat)
    assert np.array_equal(ref.points, np.unique(q, axis=0))
    a, b = pp.preprocess_device(got.points, "cuda"), pp.preprocess_device(ref.points, "cuda")
    assert len(a.origins) > 3 and a.n_points == b.n_points == len(ref.points)
    for name in ("origins", "blk_off", "points", "gt", "dist"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_every_entry_point_refuses_bad_arguments():
    need_gpu()
    from nvfpcc_amd._lib import lib, CONSTANTS
    from nvfpcc_amd import ops
    L, EINVAL = lib(), CONSTANTS["NVF_EINVAL"]
    dev = torch.device("cuda")
    n = 16
    xyz = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    q = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(ops.VOX_STATUS_WORDS, dtype=torch.int64, device=dev)
    bounds = torch.zeros(ops.VOX_BOUNDS_WORDS, dtype=torch.int64, device=dev)
    bwork = torch.zeros(ops.VOX_BOUNDS_WORK_WORDS, dtype=torch.int64, device=dev)
    uwork = torch.zeros(ops.VOX_MAX_GROUPS, dtype=torch.int32, device=dev)
    P = lambda t: t.data_ptr()
    bad_n = (0, -1, 1 << 30)
    bad_bits = (9, 13, 0)
    bad_step = (0.0, -1.0, float("inf"), float("nan"))

    def variants(good, bad):
        """Every argument list that differs from `good` in one place, by one of the bad values of that place."""
        for i, values in bad.items():
            for v in values:
                yield good[:i] + (v,) + good[i + 1:]

    good = (P(xyz), n, P(bounds), P(bwork), None)
    assert L.nvf_vox_bounds(*good) == 0
    for args in variants(good, {0: (None,), 1: bad_n, 2: (None,), 3: (None,)}):
        assert L.nvf_vox_bounds(*args) == EINVAL, args
    good = (P(xyz), n, 10, 0.0, 0.0, 0.0, 1.0, 1.0, P(q), P(keys), P(status), None)
    assert L.nvf_vox_quantize(*good) == 0
    for args in variants(good, {0: (None,), 1: bad_n, 2: bad_bits, 3: (float("nan"),), 6: bad_step, 7: bad_step,
                                8: (None,), 9: (None,), 10: (None,)}):
        assert L.nvf_vox_quantize(*args) == EINVAL, args
    good = (P(keys), n, 10, P(q), P(counts), P(status), P(uwork), None)
    assert L.nvf_vox_unique(*good) == 0
    for args in variants(good, {0: (None,), 1: bad_n, 2: bad_bits, 3: (None,), 4: (None,), 5: (None,), 6: (None,)}):
        assert L.nvf_vox_unique(*args) == EINVAL, args
    good = (P(q), n, 0.0, 0.0, 0.0, 1.0, P(xyz), None)
    assert L.nvf_vox_dequantize(*good) == 0
    for args in variants(good, {0: (None,), 1: bad_n, 5: bad_step, 6: (None,)}):
        assert L.nvf_vox_dequantize(*args) == EINVAL, args
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [n] + [0] * (n - 1)      # the good unique call: sixteen equal keys, one voxel
