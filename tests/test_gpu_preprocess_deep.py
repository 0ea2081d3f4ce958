"""Pre-processing of clouds with 11 and 12 bits per axis on the device (preprocess.preprocess_device(bits=...),
csrc/pp_device.hip at D = 6 and 7) against three yardsticks: the CPU restatement (preprocess.octree_partition / octree_level_bytes /
_neighbour_lists), the KD-tree grid oracle, and the 10-bit device path -- which is pinned to the reference's executable
-- under translation by whole octants.  Then the command line at 11 bits.  Every comparison is exact."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from nvfpcc_amd import preprocess as pp
from tests.golden_inputs import synthetic_cloud, write_cloud_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENSORS = ("origins", "blk_off", "points", "nb_off", "nb_idx", "gt", "dist")
LONELY = (992, 320, 352)                # the block [992, 1024) x [320, 352) x [352, 384) holds this point alone


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def shell_patch(center, radius, n_dir, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_dir, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.round(np.asarray(center, np.float64) + radius * d * np.array([1.0, 0.8, 1.2])).astype(np.int64)


def deep_cloud(bits):
    """Fifteen blocks at 11 bits, twenty-three at 12 (the KD-tree oracle takes a quarter of a second per block): a thin
    shell around the point where the planes x, y, z = 1024 meet (at 12 bits a second one around 2048), three stray
    points in other octants, the two far corners of the volume, duplicated rows, and a block with a single point in
    the corner farthest from the plane x = 1023 | 1024 whose neighbour across that plane is full next to the shared
    face, so most of the block's distances are decided by the neighbour's points."""
    top = (1 << bits) - 1
    parts = [shell_patch((1024, 1024, 1024), 13.0, 2500, 1), [[top - 40, 77, 1500], [5, top - 3, 900], [1100, 60, top]]]
    if bits == 12:
        parts.append(shell_patch((2048, 2048, 2048), 13.0, 2500, 2))
    ax = np.arange(32)
    slab = np.stack(np.meshgrid(1024 + np.arange(3), 320 + ax, 352 + ax, indexing="ij"), -1).reshape(-1, 3)
    parts += [slab, [LONELY], [[0, 0, 0], [top, top, top]]]
    pts = np.concatenate(parts)
    return np.concatenate([pts, pts[::7], pts[:50]])                # duplicates, not in the order of the originals


@pytest.fixture(scope="module", params=(11, 12))
def deep(request):
    """(bits, the cloud, its DevicePreprocess, the CPU partition): computed once per depth."""
    need_gpu()
    bits = request.param
    pts = deep_cloud(bits)
    return bits, pts, pp.preprocess_device(pts, "cuda", bits=bits), pp.octree_partition(pts, bits)


def test_deep_route_equals_the_cpu_restatement(deep):
    bits, pts, pre, (origins, subtree) = deep
    n, uniq = len(origins), np.unique(pts, axis=0)
    assert n == {11: 15, 12: 23}[bits]
    for plane in (1024,) if bits == 11 else (1024, 2048):       # the cloud does cross the octant planes, on every axis
        assert ((origins == plane - 32).any(0) & (origins == plane).any(0)).all()
    assert pre.bits == bits
    assert pre.origins.dtype == torch.int32 and np.array_equal(pre.origins.cpu().numpy(), origins)
    levels = pp.octree_level_bytes(pts, bits)
    assert len(pre.octree_bytes) == bits - 4
    for lv, (a, b) in enumerate(zip(pre.octree_bytes, levels)):
        assert a == b, f"level {lv}"
    assert pre.subtree == subtree
    pack = pre.octree_pack()
    assert pack[0] == bits - 5 and pack == pp.write_octree_pack(levels)
    assert np.array_equal(pp.read_octree_pack(pack), origins)
    assert pre.n_points == len(uniq)
    # the sorted points: blk_off from a host count, every block's range the points of its cube as sorted rows
    cell_of = {tuple(c): i for i, c in enumerate((origins // 32).tolist())}
    blk = np.array([cell_of[tuple(c)] for c in (pts // 32).tolist()])
    blk_off = np.concatenate([[0], np.cumsum(np.bincount(blk, minlength=n))])
    sp, off = pre.points.cpu().numpy(), pre.blk_off.cpu().numpy()
    assert np.array_equal(off, blk_off) and sp.shape == (len(pts), 3)
    for b in range(n):
        want = pts[blk == b]
        assert np.array_equal(sp[off[b]:off[b + 1]], want[np.lexsort(want.T[::-1])]), f"block {b}"
    nb_off, nb_idx = pp._neighbour_lists(origins)
    assert np.array_equal(pre.nb_off.cpu().numpy(), nb_off) and np.array_equal(pre.nb_idx.cpu().numpy(), nb_idx)
    # neighbours across an octant plane are ordinary neighbours
    lonely, slab = cell_of[(31, 10, 11)], cell_of[(32, 10, 11)]
    assert off[lonely + 1] - off[lonely] == 1
    assert nb_idx[nb_off[lonely]:nb_off[lonely + 1]].tolist() == [lonely, slab]
    corner = cell_of[((1 << bits) // 32 - 1,) * 3]
    assert nb_idx[nb_off[corner]:nb_off[corner + 1]].tolist() == [corner]


def test_deep_grids_equal_the_kdtree_oracle(deep):
    from oracle import preprocess_oracle as PO
    bits, pts, pre, (origins, _) = deep
    n = len(origins)
    for t in (pre.gt, pre.dist):
        assert t.shape == (n, 1, 32, 32, 32) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    gt_o, dist_o = PO.grids(pts, origins)
    assert torch.equal(pre.gt.cpu(), torch.from_numpy(gt_o).float())
    assert torch.equal(pre.dist.cpu(), torch.from_numpy(dist_o).float())
    assert int(pre.gt.sum().item()) == pre.n_points
    # the lonely block: one occupied voxel, and most of its voxels are nearer to the slab across x = 1023 | 1024
    b = (origins // 32).tolist().index([31, 10, 11])
    assert int(gt_o[b].sum()) == 1
    own = np.sqrt(((np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1)) ** 2).sum(-1))
    assert (dist_o[b, 0] < own).mean() > 0.5


@pytest.fixture(scope="module")
def ten_bit():
    need_gpu()
    pts = synthetic_cloud(n_dir=6000, radius=40.0)           # a small shell: a few dozen leaf cubes
    return pts, pp.preprocess_device(pts, "cuda")


@pytest.mark.parametrize("octant", ((1, 0, 0), (1, 1, 1)))
@pytest.mark.parametrize("bits", (11, 12))
def test_deep_route_equals_the_ten_bit_route_under_translation(ten_bit, bits, octant):
    pts, ref = ten_bit
    o = np.array(octant)
    shift = 1024 * o if bits == 11 else 3072 * o
    extra = bits - 10
    pre = pp.preprocess_device(pts + shift, "cuda", bits=bits)
    back = torch.from_numpy(shift).to(device="cuda", dtype=torch.int32)
    assert torch.equal(pre.origins - back, ref.origins) and torch.equal(pre.points - back, ref.points)
    for name in ("blk_off", "nb_off", "nb_idx", "gt", "dist"):
        assert torch.equal(getattr(pre, name), getattr(ref, name)), name
    assert pre.n_points == ref.n_points
    child = bytes([1 << (octant[0] + 2 * octant[1] + 4 * octant[2])])
    assert pre.octree_bytes[:extra] == (child,) * extra and pre.octree_bytes[extra:] == ref.octree_bytes
    assert pre.octree_pack()[1 + extra:] == ref.octree_pack()[1:]


def test_row_order_and_duplicates_do_not_matter_and_calls_repeat_bit_for_bit(deep):
    bits, pts, a, _ = deep
    b = pp.preprocess_device(pts, "cuda", bits=bits)
    for name in TENSORS:                                    # the same input: the same bits everywhere
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    uniq = np.unique(pts, axis=0)
    u = pp.preprocess_device(uniq, "cuda", bits=bits)
    rng = np.random.default_rng(3)
    shuffled = np.repeat(uniq, 2, axis=0)[rng.permutation(2 * len(uniq))]
    c = pp.preprocess_device(torch.from_numpy(shuffled).to("cuda"), "cuda", bits=bits)     # int64, already on the device
    for other in (b, u, c):
        for name in ("origins", "nb_off", "nb_idx", "gt", "dist"):
            assert torch.equal(getattr(a, name), getattr(other, name)), name
        assert other.octree_bytes == a.octree_bytes and other.subtree == a.subtree and other.n_points == a.n_points
    assert c.points.shape[0] == 2 * len(uniq) and torch.equal(c.blk_off, 2 * u.blk_off)
    assert torch.equal(c.points[::2], u.points) and torch.equal(c.points[1::2], u.points)


@pytest.mark.parametrize("bits", (11, 12))
def test_blocks_scattered_over_the_whole_volume(bits):
    """A few thousand blocks all over the volume: every workgroup of the grid-wide scans holds set bits, so block ids
    and neighbour offsets depend on the partial sums carried between workgroups."""
    need_gpu()
    rng = np.random.default_rng(40 + bits)
    top = 1 << bits
    seeds = rng.integers(0, top, size=(1500, 3))
    pts = np.concatenate([seeds, (seeds[:700] + rng.integers(-40, 41, size=(700, 3))).clip(0, top - 1)])
    pre = pp.preprocess_device(pts, "cuda", bits=bits)
    origins, subtree = pp.octree_partition(pts, bits)
    assert len(origins) > 2000 and np.array_equal(pre.origins.cpu().numpy(), origins)
    assert pre.octree_bytes == tuple(pp.octree_level_bytes(pts, bits)) and pre.subtree == subtree
    nb_off, nb_idx = pp._neighbour_lists(origins)
    assert nb_off[-1] > len(origins)                                       # some blocks do have neighbours
    assert np.array_equal(pre.nb_off.cpu().numpy(), nb_off) and np.array_equal(pre.nb_idx.cpu().numpy(), nb_idx)
    key = pp._child_path_key(pts // 32, bits - 5) * 32768 + (pts[:, 0] % 32) * 1024 + (pts[:, 1] % 32) * 32 + pts[:, 2] % 32
    order = np.argsort(key, kind="stable")
    assert np.array_equal(pre.points.cpu().numpy(), pts[order])
    first = np.flatnonzero(np.diff(key[order] // 32768, prepend=-1))
    assert np.array_equal(pre.blk_off.cpu().numpy(), np.concatenate([first, [len(pts)]]))
    assert pre.n_points == len(np.unique(pts, axis=0)) == int(pre.gt.sum().item())
    assert pre.gt.shape == (len(origins), 1, 32, 32, 32) and float(pre.dist.max()) <= np.float32(np.sqrt(3 * 31.0 ** 2))


def test_more_than_a_million_rows_at_twelve_bits():
    """Past 2^20 rows at 12 bits the neighbour-offset scan gives each thread two entries instead of one (the buffers
    are sized from min(8^D, rows), and 8^6 is below that count); the rows are the small cloud's, repeated."""
    need_gpu()
    bits = 12
    uniq = np.unique(deep_cloud(bits), axis=0)
    a = pp.preprocess_device(uniq, "cuda", bits=bits)
    k = (1 << 20) // len(uniq) + 1
    big = pp.preprocess_device(torch.from_numpy(uniq).to("cuda").repeat(k, 1), "cuda", bits=bits)
    assert big.points.shape[0] == k * len(uniq) > 1 << 20
    for name in ("origins", "nb_off", "nb_idx", "gt", "dist"):
        assert torch.equal(getattr(a, name), getattr(big, name)), name
    assert big.octree_bytes == a.octree_bytes and big.n_points == a.n_points
    assert torch.equal(big.points[::k], torch.from_numpy(uniq[np.argsort(
        pp._child_path_key(uniq // 32, 7) * 32768 + (uniq % 32) @ np.array([1024, 32, 1]), kind="stable")]).to("cuda", torch.int32))


def test_bad_input_raises_value_error_and_the_next_call_works():
    need_gpu()
    good = deep_cloud(11)[:200]
    for bits, bound in ((11, 2048), (12, 4096), (10, 1024)):
        base = good if bits > 10 else good % 1024
        for bad_row in ([5, bound, 5], [-1, 0, 0], [0, 0, 2 ** 40 + 7], [-2 ** 35, 1, 1]):
            with pytest.raises(ValueError, match=r"\[0, %d\)" % bound):
                pp.preprocess_device(np.concatenate([base, [bad_row]]), "cuda", bits=bits)
        with pytest.raises(ValueError, match=r"\[0, %d\)" % bound):            # int32 on the device: no host clamp
            pp.preprocess_device(torch.tensor([[1, 2, 3], [bound, 0, 0]], dtype=torch.int32, device="cuda"), "cuda", bits=bits)
        pre = pp.preprocess_device(base, "cuda", bits=bits)                     # the device is as usable as before
        assert np.array_equal(pre.origins.cpu().numpy(), pp.octree_partition(base, bits)[0])
    for bits in (13, 9):
        with pytest.raises(ValueError, match="bits"):
            pp.preprocess_device(good, "cuda", bits=bits)
    with pytest.raises(ValueError):
        pp.preprocess_device(np.zeros((0, 3), np.int64), "cuda", bits=12)
    with pytest.raises(ValueError):
        pp.preprocess_device(np.zeros((4, 3), np.float32), "cuda", bits=11)
    single = pp.preprocess_device(np.array([[2047, 0, 1030]]), "cuda", bits=11)
    assert single.origins.tolist() == [[2016, 0, 1024]] and single.nb_idx.tolist() == [0] and single.n_points == 1
    assert single.octree_bytes == tuple(pp.octree_level_bytes(np.array([[2047, 0, 1030]]), 11))


# ---------------------------------------------------------------- command line
def run(cmd, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert (r.returncode == 0) == ok, r.stdout[-3000:]
    return r.stdout


@pytest.mark.timeout(600)
def test_cli_trains_encodes_and_decodes_an_eleven_bit_cloud(tmp_path):
    need_gpu()
    from nvfpcc_amd.recon import read_ply_ascii
    pts = np.unique(shell_patch((1024, 1024, 1024), 12.0, 3000, 5), axis=0)     # the eight blocks around one corner
    assert len(pp.octree_partition(pts, 11)[0]) == 8 and pts.min() < 1024 <= pts.max()
    cwd = str(tmp_path)
    write_cloud_ply(os.path.join(cwd, "cloud.ply"), pts)
    cli = os.path.join(ROOT, "NVFPCC.py")
    common = ["--chanstr", "8,16,8,8", "--ch", "3"]
    # what the deeper partition does not reach exits with its reason before the device is opened or the cloud is read
    out = run([cli, "encode", "absent.ply", "--bits", "11", "--load_weights", "q4.ckpt"] + common, cwd, ok=False)
    assert "10-bit only" in out and "Traceback" not in out
    for command in ("train", "encode"):
        out = run([cli, command, "absent.ply", "--from_ply", "--bits", "11", "--ref_ply", "cloud.ply"] + common, cwd, ok=False)
        assert "--ref_ply with --bits 11 is not supported" in out and "Traceback" not in out
    assert sorted(os.listdir(cwd)) == ["cloud.ply"]
    out = run([cli, "train", "cloud.ply", "--from_ply", "--bits", "11", "--checkpoint_dir", "ckpts", "--batchsize", "4",
               "--lambda", "200", "--lr", "1e-3", "--w1", "10", "--w2", "57", "--wemb", "5", "--shuffle", "True",
               "--epochs", "2", "--phase_change", "1"] + common, cwd)
    assert "[data] 8 leaf blocks, %d points" % len(pts) in out and "[Epoch 0001 TRAIN" in out
    run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0000.ckpt", "q4.ckpt", "16"], cwd)
    out = run([cli, "encode", "cloud.ply", "--from_ply", "--pack_octree", "--bits", "11", "--thh_mode", "block-count",
               "--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0000_emb.ckpt"] + common, cwd)
    assert "[Recon]" in out
    run([cli, "decode", "pack.pk", "--batchsize", "1"] + common, cwd)              # no --N, no --thh, no --bits
    with open(os.path.join(cwd, "pack.pk"), "rb") as f:
        pack = pickle.load(f)
    assert list(pack) == ['net_weight_pack', 'latent_pack', 'octree_pack', 'thh_pack']
    assert pack['octree_pack'][0] == 6
    assert np.array_equal(pp.read_octree_pack(pack['octree_pack']), pp.octree_partition(pts, 11)[0])
    enc, dec = read_ply_ascii(os.path.join(cwd, "rc_enc.ply")), read_ply_ascii(os.path.join(cwd, "rc_dec.ply"))
    assert np.array_equal(np.unique(enc, axis=0), np.unique(dec, axis=0)) and len(enc) == len(dec)
    assert dec.min() >= 0 and dec.max() < 2048 and dec.max() >= 1024
