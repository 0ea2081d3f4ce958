"""Pre-processing on the device (preprocess.preprocess_device, csrc/pp_device.hip) against the host route it replaces
(octree_level5 + build_grids -> float32, same process), the KD-tree oracle and the reference executable's golden
partition; the `--from_ply` / `--pack_octree` command lines against the file-based ones.  Every comparison is exact."""
import hashlib
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from nvfpcc_amd import preprocess as pp
from tests.golden_inputs import synthetic_cloud, write_cloud_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def scattered_cloud():
    rng = np.random.default_rng(6)                      # as test_distance_grids_equal_the_kdtree_oracle
    return np.unique(rng.integers(300, 460, size=(400, 3)), axis=0)


def corner_cloud():
    ends = np.array([0, 1023])
    corners = np.stack(np.meshgrid(ends, ends, ends, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    near = np.concatenate([c + rng.integers(-20, 21, size=(30, 3)) for c in corners]).clip(0, 1023)
    return np.unique(np.concatenate([corners, near]), axis=0)


CLOUDS = {
    "synthetic": synthetic_cloud,
    "scattered": scattered_cloud,
    "corners": corner_cloud,
    "single": lambda: np.array([[1023, 0, 517]], np.int64),
}
TENSORS = ("origins", "blk_off", "points", "nb_off", "nb_idx", "gt", "dist")


def host_route(pts):
    """The existing path: (origins, subtree, gt float32, dist float32 as LoadedVoxelDataset.to_device gives them,
    blk_off, (nb_off, nb_idx))."""
    origins, subtree = pp.octree_level5(pts)
    gt, dist = pp.build_grids(pts, origins)
    cell_of = {tuple(c): i for i, c in enumerate((origins // 32).tolist())}
    blk = np.array([cell_of[tuple(c)] for c in (np.asarray(pts) // 32).tolist()])
    blk_off = np.concatenate([[0], np.cumsum(np.bincount(blk, minlength=len(origins)))])
    return (origins, subtree, torch.from_numpy(gt).float(), torch.from_numpy(dist).float(), blk_off,
            pp._neighbour_lists(origins))


@pytest.mark.parametrize("name", list(CLOUDS))
def test_device_route_equals_the_host_route_and_the_oracle(name, golden_dir):
    need_gpu()
    from oracle import preprocess_oracle as PO
    pts = CLOUDS[name]()
    pre = pp.preprocess_device(pts, "cuda")
    origins, subtree, gt, dist, blk_off, (nb_off, nb_idx) = host_route(pts)
    n = len(origins)
    assert pre.origins.dtype == torch.int32 and np.array_equal(pre.origins.cpu().numpy(), origins)
    assert pre.subtree == subtree
    assert pre.octree_bytes == tuple(pp.octree_level_bytes(pts))
    assert pp.read_octree_pack(pre.octree_pack()).tolist() == origins.tolist()
    assert pre.n_points == len(pts)
    assert np.array_equal(pre.blk_off.cpu().numpy(), blk_off)
    assert np.array_equal(pre.nb_off.cpu().numpy(), nb_off) and np.array_equal(pre.nb_idx.cpu().numpy(), nb_idx)
    for t in (pre.gt, pre.dist):
        assert t.shape == (n, 1, 32, 32, 32) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    assert torch.equal(pre.gt.cpu(), gt) and torch.equal(pre.dist.cpu(), dist)
    gt_o, dist_o = PO.grids(pts, origins)
    assert torch.equal(pre.gt.cpu(), torch.from_numpy(gt_o).float())
    assert torch.equal(pre.dist.cpu(), torch.from_numpy(dist_o).float())
    assert int(pre.gt.sum().item()) == len(pts)
    # the sorted points: every block's range holds exactly the points of its cube
    sp, off = pre.points.cpu().numpy(), pre.blk_off.cpu().numpy()
    assert np.array_equal(np.unique(sp, axis=0), np.unique(pts, axis=0))
    assert np.array_equal(sp // 32 * 32, np.repeat(origins, np.diff(off), axis=0))
    if name == "synthetic":
        G = np.load(os.path.join(golden_dir, "octree.npz"))
        assert np.array_equal(pre.origins.cpu().numpy(), G["origins"])
        assert len(pre.subtree) == int(G["subtree_len"])
        assert hashlib.sha256(pre.subtree.encode()).digest() == G["subtree_sha"].tobytes()


def test_row_order_and_duplicates_do_not_matter_and_calls_repeat_bit_for_bit():
    need_gpu()
    pts = synthetic_cloud()
    a = pp.preprocess_device(pts, "cuda")
    b = pp.preprocess_device(pts, "cuda")
    rng = np.random.default_rng(3)
    shuffled = np.repeat(pts, 2, axis=0)[rng.permutation(2 * len(pts))]
    c = pp.preprocess_device(torch.from_numpy(shuffled).to("cuda"), "cuda")        # int64 tensor already on the device
    for other in (b, c):
        for name in ("origins", "nb_off", "nb_idx", "gt", "dist"):
            assert torch.equal(getattr(a, name), getattr(other, name)), name
        assert other.octree_bytes == a.octree_bytes and other.subtree == a.subtree and other.n_points == a.n_points
    for name in TENSORS:                                    # the same input: the same bits everywhere
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert c.n_points == len(pts) and c.points.shape[0] == 2 * len(pts)
    assert torch.equal(c.blk_off, 2 * a.blk_off)
    assert torch.equal(c.points[::2], a.points) and torch.equal(c.points[1::2], a.points)


def test_bad_input_raises_value_error():
    need_gpu()
    with pytest.raises(ValueError):
        pp.preprocess_device(np.zeros((0, 3), np.int64), "cuda")
    good = synthetic_cloud()[:100]
    for bad_row in ([5, 1024, 5], [-1, 0, 0], [0, 0, 2 ** 40 + 7], [-2 ** 35, 1, 1]):
        with pytest.raises(ValueError, match=r"\[0, 1024\)"):
            pp.preprocess_device(np.concatenate([good, [bad_row]]), "cuda")
    with pytest.raises(ValueError):
        pp.preprocess_device(np.zeros((4, 2), np.int64), "cuda")
    with pytest.raises(ValueError):
        pp.preprocess_device(np.zeros((4, 3), np.float32), "cuda")


def exact_against_the_cpu_restatement(pts, bits, pre):
    """Every integer output of `pre` against octree_partition / octree_level_bytes / _neighbour_lists and a host sort;
    returns the origins."""
    pts = np.asarray(pts, np.int64)
    origins, subtree = pp.octree_partition(pts, bits)
    assert pre.bits == bits and pre.origins.dtype == torch.int32 and np.array_equal(pre.origins.cpu().numpy(), origins)
    assert pre.octree_bytes == tuple(pp.octree_level_bytes(pts, bits)) and pre.subtree == subtree
    assert pre.octree_pack() == pp.octree_pack_from_origins(origins, bits)
    assert np.array_equal(pp.read_octree_pack(pre.octree_pack()), origins)
    nb_off, nb_idx = pp._neighbour_lists(origins)
    assert np.array_equal(pre.nb_off.cpu().numpy(), nb_off) and np.array_equal(pre.nb_idx.cpu().numpy(), nb_idx)
    key = pp._child_path_key(pts // 32, bits - 5) * 32768 + (pts % 32) @ np.array([1024, 32, 1])
    order = np.argsort(key, kind="stable")
    assert np.array_equal(pre.points.cpu().numpy(), pts[order])
    first = np.flatnonzero(np.diff(key[order] // 32768, prepend=-1))
    assert np.array_equal(pre.blk_off.cpu().numpy(), np.concatenate([first, [len(pts)]]))
    assert pre.n_points == len(np.unique(pts, axis=0)) == int(pre.gt.sum().item())
    return origins


@pytest.mark.parametrize("bits", (10, 11, 12))
def test_one_point_at_the_last_voxel_of_the_volume(bits):
    """Every level holds one node (min(8^L, 1) = 1 byte of room) and every scan meets its only non-empty word at the
    very end of its bitmap."""
    need_gpu()
    from oracle import preprocess_oracle as PO
    top = (1 << bits) - 1
    pts = np.array([[top, top, top]], np.int64)
    pre = pp.preprocess_device(pts, "cuda", bits=bits)
    origins = exact_against_the_cpu_restatement(pts, bits, pre)
    assert origins.tolist() == [[top - 31] * 3] and pre.octree_bytes == (b"\x80",) * (bits - 4)
    assert pre.nb_off.tolist() == [0, 1] and pre.nb_idx.tolist() == [0] and pre.blk_off.tolist() == [0, 1]
    gt_o, dist_o = PO.grids(pts, origins)
    assert pre.gt.shape == (1, 1, 32, 32, 32)
    assert torch.equal(pre.gt.cpu(), torch.from_numpy(gt_o).float())
    assert torch.equal(pre.dist.cpu(), torch.from_numpy(dist_o).float())


def test_seven_points_in_seven_leaves():
    """Fewer points than a node has children: every level below the root has room for 7 nodes, not 8^L, and the
    levels of the octree bytes start where those rooms add up to."""
    need_gpu()
    from oracle import preprocess_oracle as PO
    pts = np.array([[0, 0, 0], [1023, 1023, 1023], [40, 0, 0], [0, 40, 0], [511, 512, 500], [512, 511, 500],
                    [700, 33, 991]], np.int64)
    pre = pp.preprocess_device(pts, "cuda")
    origins = exact_against_the_cpu_restatement(pts, 10, pre)
    assert len(origins) == 7 and [len(b) for b in pre.octree_bytes] == [1, 5, 5, 5, 5, 7]
    assert pre.octree_pack() == pp.octree_pack_from_origins(origins)
    host = host_route(pts)
    assert pre.subtree == host[1] and torch.equal(pre.gt.cpu(), host[2]) and torch.equal(pre.dist.cpu(), host[3])
    gt_o, dist_o = PO.grids(pts, origins)
    assert torch.equal(pre.gt.cpu(), torch.from_numpy(gt_o).float())
    assert torch.equal(pre.dist.cpu(), torch.from_numpy(dist_o).float())


@pytest.mark.parametrize("where", ("corner", "centre"))
@pytest.mark.parametrize("bits", (10, 12))
def test_a_solid_cube_of_125_leaves(bits, where):
    """5 x 5 x 5 leaves, one point each, at the origin corner of the volume and straddling its centre planes: the
    middle block's list holds all 125 blocks in _neighbour_lists' order, the blocks at the rim are clipped."""
    need_gpu()
    side = 1 << (bits - 5)
    first = 0 if where == "corner" else side // 2 - 2
    cells = np.stack(np.meshgrid(*[first + np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = cells * 32 + np.random.default_rng(bits).integers(0, 32, size=cells.shape)
    pre = pp.preprocess_device(pts, "cuda", bits=bits)
    origins = exact_against_the_cpu_restatement(pts, bits, pre)
    assert len(origins) == 125
    nb_off, nb_idx = pre.nb_off.cpu().numpy(), pre.nb_idx.cpu().numpy()
    cell_of = {tuple(c): i for i, c in enumerate((origins // 32).tolist())}
    steps = sorted(((dx, dy, dz) for dx in range(-2, 3) for dy in range(-2, 3) for dz in range(-2, 3)),
                   key=lambda s: s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    mid = cell_of[(first + 2,) * 3]
    assert nb_idx[nb_off[mid]:nb_off[mid + 1]].tolist() == [cell_of[tuple(first + 2 + d for d in s)] for s in steps]
    low = cell_of[(first,) * 3]
    assert nb_off[low + 1] - nb_off[low] == 27 and nb_idx[nb_off[low]] == low
    gt, dist = pp.build_grids(pts, origins)                    # the same distance kernel under the host's lists
    assert pre.gt.shape == (125, 1, 32, 32, 32)
    assert torch.equal(pre.gt.cpu(), torch.from_numpy(gt).float())
    assert torch.equal(pre.dist.cpu(), torch.from_numpy(dist).float())


def test_out_of_range_at_ten_bits_raises_and_the_next_call_works():
    need_gpu()
    good = scattered_cloud()
    for bad_row in ([5, 1024, 5], [-1, 0, 0]):
        with pytest.raises(ValueError, match=r"coordinates must lie in \[0, 1024\)"):
            pp.preprocess_device(np.concatenate([good, [bad_row]]), "cuda", bits=10)
    with pytest.raises(ValueError, match=r"coordinates must lie in \[0, 1024\)"):          # int32 on the device: no host clamp
        pp.preprocess_device(torch.tensor([[1, 2, 3], [1024, 0, 0]], dtype=torch.int32, device="cuda"), "cuda", bits=10)
    exact_against_the_cpu_restatement(good, 10, pp.preprocess_device(good, "cuda", bits=10))


def test_sqrt_epilogue_is_exact_for_every_squared_distance():
    """dist = sqrtf(d2) on the device equals float32(sqrt(float64(d2))) for every integer below 2^22, the bound
    thh_select.d2_from_dist documents; gt = (d2 == 0)."""
    need_gpu()
    from nvfpcc_amd.thh_select import D2_EXACT_BOUND
    assert D2_EXACT_BOUND == 1 << 22
    d2 = torch.arange(D2_EXACT_BOUND, dtype=torch.int32, device="cuda")
    gt, dist = pp.grids_from_d2(d2)
    want = np.sqrt(np.arange(D2_EXACT_BOUND, dtype=np.float64)).astype(np.float32)
    assert np.array_equal(dist.cpu().numpy(), want)
    assert int(gt.sum().item()) == 1 and float(gt[0]) == 1.0
    odd = d2[:1027].clone()                                 # a length that is no multiple of four
    gt2, dist2 = pp.grids_from_d2(odd, in_place=True)
    assert dist2.data_ptr() == odd.data_ptr() and np.array_equal(dist2.cpu().numpy(), want[:1027])
    assert torch.equal(gt2, gt[:1027])


def test_dataset_from_device_matches_the_file_dataset(tmp_path):
    need_gpu()
    from nvfpcc_amd.dataloader import LoadedVoxelDataset
    from nvfpcc_amd.thh_select import d2_from_dist
    pts = scattered_cloud()
    origins, _ = pp.octree_level5(pts)
    gt, dist = pp.build_grids(pts, origins)
    fid = str(tmp_path / "c")
    np.save(f"{fid}_l5_origins", origins.astype(np.float64))
    np.save(f"{fid}_l5_gt_grid", gt)
    np.save(f"{fid}_l5_dist", dist)
    files = LoadedVoxelDataset(f"{fid}_l5_origins.npy", f"{fid}_l5_gt_grid.npy", f"{fid}_l5_dist.npy")
    pre = pp.preprocess_device(pts, "cuda")
    data = LoadedVoxelDataset.from_device(pre)
    assert "gt_grid" not in data.__dict__ and "dist" not in data.__dict__          # nothing materialised yet
    assert (data.N_leaf, int(data.N), len(data)) == (files.N_leaf, int(files.N), len(files))
    assert data.origins.dtype == files.origins.dtype and np.array_equal(data.origins, files.origins)
    assert [data.permute(i) for i in range(len(data))] == [files.permute(i) for i in range(len(files))]
    assert np.array_equal(data.epoch_order(3, True, seed=1), files.epoch_order(3, True, seed=1))
    g_dev, d_dev = data.to_device("cuda")
    assert g_dev.data_ptr() == pre.gt.data_ptr() and d_dev.data_ptr() == pre.dist.data_ptr()      # no copy
    g_file, d_file = files.to_device("cuda")
    assert torch.equal(g_dev, g_file) and torch.equal(d_dev, d_file)
    assert "gt_grid" not in data.__dict__
    assert data.gt_grid.dtype == np.uint8 and np.array_equal(data.gt_grid, files.gt_grid)
    assert torch.equal(d2_from_dist(data.dist), d2_from_dist(files.dist))
    for a, b in zip(data[5], files[5]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- command line
def run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def gross_bpp(out):
    return re.search(r"Gross bpp: ([0-9.]+)", out).group(1)


def ply_rows(path):
    from nvfpcc_amd.recon import read_ply_ascii
    return read_ply_ascii(path)


@pytest.mark.timeout(900)
def test_cli_from_ply_equals_the_file_based_cli(tmp_path):
    need_gpu()
    pts = synthetic_cloud(n_dir=6000, radius=40.0)           # a small shell: a few dozen leaf cubes
    n_leaf = len(pp.octree_level5(pts)[0])
    cli = os.path.join(ROOT, "NVFPCC.py")
    common = ["--chanstr", "8,16,8,8", "--ch", "3"]
    train = ["--checkpoint_dir", "ckpts", "--batchsize", "8", "--lambda", "200", "--lr", "1e-3", "--w1", "10", "--w2",
             "57", "--wemb", "5", "--shuffle", "True", "--epochs", "11", "--phase_change", "5"] + common
    enc = ["--batchsize", "5", "--load_weights", "q4.ckpt", "--load_emb", "ckpts/0010_emb.ckpt", "--thh", "0.5"] + common
    dirs = {k: str(tmp_path / k) for k in ("files", "ply", "ply_count")}
    for d in dirs.values():
        os.makedirs(d)
        write_cloud_ply(os.path.join(d, "cloud.ply"), pts)
    # the file-based route: get_octree.py + util_get_grids.py + train / encode / decode
    run([os.path.join(ROOT, "get_octree.py"), "cloud.ply", "cloud_l5_origins.txt", "cloud_l5_subtree.txt"], dirs["files"])
    run([os.path.join(ROOT, "util_get_grids.py"), "cloud.ply", "5"], dirs["files"])
    run([cli, "train", "cloud.ply"] + train, dirs["files"])
    run([cli, "train", "cloud.ply", "--from_ply"] + train, dirs["ply"])
    assert not [f for f in os.listdir(dirs["ply"]) if f.endswith(".npy") or f.endswith(".txt")]
    for fn in ("0000.ckpt", "0010.ckpt"):
        a = torch.load(os.path.join(dirs["files"], "ckpts", fn), map_location="cpu")
        b = torch.load(os.path.join(dirs["ply"], "ckpts", fn), map_location="cpu")
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (fn, k)
    for fn in ("0000_emb.ckpt", "0010_emb.ckpt"):
        assert torch.equal(torch.load(os.path.join(dirs["files"], "ckpts", fn), map_location="cpu"),
                           torch.load(os.path.join(dirs["ply"], "ckpts", fn), map_location="cpu")), fn
    for d in (dirs["files"], dirs["ply"]):
        run([os.path.join(ROOT, "manipulate_weights.py"), "ckpts/0010.ckpt", "q4.ckpt", "16"], d)
    out_f = run([cli, "encode", "cloud.ply"] + enc, dirs["files"])
    run([cli, "decode", "pack.pk", "--batchsize", "1", "--thh", "0.5", "--N", str(n_leaf)] + common, dirs["files"])
    out_p = run([cli, "encode", "cloud.ply", "--from_ply", "--pack_octree"] + enc, dirs["ply"])
    run([cli, "decode", "pack.pk", "--batchsize", "1", "--thh", "0.5"] + common, dirs["ply"])          # no --N
    with open(os.path.join(dirs["ply"], "pack.pk"), "rb") as f:
        pack = pickle.load(f)
    with open(os.path.join(dirs["files"], "pack.pk"), "rb") as f:
        pack_f = pickle.load(f)
    assert list(pack_f) == ['net_weight_pack', 'origins', 'latent_pack']                  # unchanged without the flag
    assert list(pack) == ['net_weight_pack', 'latent_pack', 'octree_pack']
    assert np.array_equal(pp.read_octree_pack(pack['octree_pack']), pack_f['origins'].astype(np.int64))
    assert pack['latent_pack']['latent_byte_stream'] == pack_f['latent_pack']['latent_byte_stream']
    # eleven epochs need not lift any probability over a fixed 0.5: that the decoded cloud is not empty is asserted
    # below, where the threshold is chosen to keep at least as many voxels as the input has points
    ref = ply_rows(os.path.join(dirs["files"], "rc_enc.ply"))
    assert np.array_equal(ref, ply_rows(os.path.join(dirs["files"], "rc_dec.ply")))
    assert np.array_equal(ref, ply_rows(os.path.join(dirs["ply"], "rc_enc.ply")))
    assert np.array_equal(ref, ply_rows(os.path.join(dirs["ply"], "rc_dec.ply")))
    # Gross bpp counts the octree bytes: the file-based figure + 8 len(octree_pack) / N, as printed
    bits = 8 * (len(pack_f['latent_pack']['latent_byte_stream']) + len(pack_f['net_weight_pack']['bit_stream']))
    assert gross_bpp(out_f) == '%.4f' % (bits / len(pts))
    assert gross_bpp(out_p) == '%.4f' % ((bits + 8 * len(pack['octree_pack'])) / len(pts))
    ln = lambda out: [l for l in out.splitlines() if l.startswith("[Recon]")]
    assert ln(out_p) == ln(out_f) and ln(out_p)
    # with a threshold chosen at encode time the pack carries both side entries; the file-based encoder takes
    # --pack_octree too and writes the same octree bytes
    for f in ("q4.ckpt", "ckpts"):
        os.symlink(os.path.join(dirs["ply"], f), os.path.join(dirs["ply_count"], f))
    out_c = run([cli, "encode", "cloud.ply", "--from_ply", "--pack_octree", "--thh_mode", "count"] + enc, dirs["ply_count"])
    run([cli, "decode", "pack.pk", "--batchsize", "2"] + common, dirs["ply_count"])
    with open(os.path.join(dirs["ply_count"], "pack.pk"), "rb") as f:
        pack_c = pickle.load(f)
    assert list(pack_c) == ['net_weight_pack', 'latent_pack', 'octree_pack', 'thh_pack']
    assert pack_c['octree_pack'] == pack['octree_pack']
    ref_c = ply_rows(os.path.join(dirs["ply_count"], "rc_enc.ply"))
    assert ref_c.shape[0] >= len(pts) and np.array_equal(ref_c, ply_rows(os.path.join(dirs["ply_count"], "rc_dec.ply")))
    out_fc = run([cli, "encode", "cloud.ply", "--thh_mode", "count"] + enc, dirs["files"])
    assert np.array_equal(ref_c, ply_rows(os.path.join(dirs["files"], "rc_enc.ply")))
    run([cli, "decode", "pack.pk", "--batchsize", "1", "--N", str(n_leaf)] + common, dirs["files"])
    assert np.array_equal(ref_c, ply_rows(os.path.join(dirs["files"], "rc_dec.ply")))
    bits_c = bits + 8 * len(pack_c['thh_pack'])
    assert gross_bpp(out_fc) == '%.4f' % (bits_c / len(pts))
    assert gross_bpp(out_c) == '%.4f' % ((bits_c + 8 * len(pack['octree_pack'])) / len(pts))
    pick = lambda out: [l for l in out.splitlines() if l.startswith("[Threshold]")]
    assert pick(out_c) == pick(out_fc) and pick(out_c)
    run([cli, "encode", "cloud.ply", "--pack_octree", "--pack_fn", "pack_o.pk"] + enc, dirs["files"])
    with open(os.path.join(dirs["files"], "pack_o.pk"), "rb") as f:
        assert pickle.load(f)['octree_pack'] == pack['octree_pack']
