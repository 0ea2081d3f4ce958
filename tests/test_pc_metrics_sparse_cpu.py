"""Host-side parts of the geometry metrics beyond 10 bits per axis: the range rules of `bits` / `index`, the flags of
`python -m nvfpcc_amd.pc_error`, the bits `NVFPCC.py decode --ref_ply` reads from a pack, and the refusals of the
sparse-index entry points of the C ABI, none of which needs a device."""
import ctypes

import numpy as np
import pytest

from nvfpcc_amd import _lib, pc_error, pc_metrics

GOOD = np.array([[0, 0, 0], [1023, 1023, 1023], [5, 6, 7]])


def test_the_range_follows_bits():
    assert np.array_equal(pc_metrics._points(np.array([[0, 0, 1024]]), "x", 11), [[0, 0, 1024]])
    assert np.array_equal(pc_metrics._points(np.array([[4095, 0, 2048.0]]), "x", 12), [[4095, 0, 2048]])
    with pytest.raises(ValueError, match=r"\[0, 1024\)"):
        pc_metrics.nearest(np.array([[0, 0, 1024]]), GOOD)                        # the default stays 10 bits
    with pytest.raises(ValueError, match=r"\[0, 2048\)"):
        pc_metrics.nearest(GOOD, np.array([[2048, 0, 0]]), bits=11)
    with pytest.raises(ValueError, match=r"\[0, 4096\)"):
        pc_metrics.geometry_psnr(GOOD, np.array([[0, 4096, 0]]), bits=12)
    with pytest.raises(ValueError, match=r"\[0, 4096\)"):
        pc_metrics.estimate_normals(np.array([[0, 4096, 0]] * 12), bits=12)


def test_a_cloud_in_range_passes_the_host_checks():
    # 1024 is accepted at 11 bits: the call gets as far as asking for a device (or runs, where there is one)
    import torch
    if torch.cuda.is_available():
        idx, d2 = pc_metrics.nearest(np.array([[0, 0, 1024]]), GOOD, bits=11)
        assert idx[0] == 2 and d2[0] == 25 + 36 + 1017 ** 2
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pc_metrics.nearest(np.array([[0, 0, 1024]]), GOOD, bits=11)


@pytest.mark.parametrize("bits", [9, 13])
def test_bits_outside_ten_to_twelve_are_refused(bits):
    for call in (lambda: pc_metrics.nearest(GOOD, GOOD, bits=bits),
                 lambda: pc_metrics.estimate_normals(GOOD, k=3, bits=bits),
                 lambda: pc_metrics.geometry_psnr(GOOD, GOOD, bits=bits)):
        with pytest.raises(ValueError, match="bits"):
            call()


def test_the_dense_index_is_ten_bit_only():
    for bits in (11, 12):
        with pytest.raises(ValueError, match="dense"):
            pc_metrics.geometry_psnr(GOOD, GOOD, bits=bits, index="dense")
        with pytest.raises(ValueError, match="dense"):
            pc_metrics.nearest(GOOD, GOOD, bits=bits, index="dense")
    with pytest.raises(ValueError, match="index"):
        pc_metrics.nearest(GOOD, GOOD, index="hashed")
    assert pc_metrics._check_index(10, None) is False and pc_metrics._check_index(10, "dense") is False
    assert pc_metrics._check_index(10, "sparse") is True
    assert pc_metrics._check_index(11, None) is True and pc_metrics._check_index(12, "sparse") is True


def test_pc_error_parser_has_bits_and_index():
    p = pc_error.build_parser()
    d = p.parse_args(["a.ply", "b.ply"])
    assert (d.bits, d.index, d.peak) == (10, None, None)
    a = p.parse_args(["a.ply", "b.ply", "--bits", "12", "--index", "sparse", "--peak", "1023"])
    assert (a.bits, a.index, a.peak) == (12, "sparse", 1023.0)
    for bad in (["--bits", "13"], ["--index", "hashed"]):
        with pytest.raises(SystemExit):
            p.parse_args(["a.ply", "b.ply"] + bad)


def test_pack_bits():
    import NVFPCC
    for header, bits in ((5, 10), (6, 11), (7, 12)):
        assert NVFPCC._pack_bits({"octree_pack": bytes([header, 0xff, 0x01])}, None) == bits
    raw = lambda top: np.array([[0, 32, 64], [top, 0, 0]], np.int16)
    assert NVFPCC._pack_bits({"origins": raw(992)}, raw(992)) == 10
    assert NVFPCC._pack_bits({"origins": raw(1024)}, raw(1024)) == 11
    assert NVFPCC._pack_bits({"origins": raw(2016)}, raw(2016)) == 11
    assert NVFPCC._pack_bits({"origins": raw(2048)}, raw(2048)) == 12
    assert NVFPCC._pack_bits({"origins": raw(4064)}, raw(4064)) == 12
    with pytest.raises(SystemExit):
        NVFPCC._pack_bits({"origins": raw(4096)}, raw(4096))


def test_pack_bits_reads_what_the_encoder_writes():
    import NVFPCC
    from nvfpcc_amd import preprocess as pp
    origins = np.array([[0, 0, 0], [2016, 32, 1024]])
    assert NVFPCC._pack_bits({"octree_pack": pp.octree_pack_from_origins(origins, bits=11)}, None) == 11
    assert NVFPCC._pack_bits({"octree_pack": pp.octree_pack_from_origins(origins // 2 // 32 * 32)}, None) == 10


def _index(bits=12, n=100, n_cells=10, n_supers=2, **null):
    f = {name: 8 for name in ("sorted", "cell_start", "super_mask", "super_first", "super_table", "hyper_table")}
    f.update(null)
    return _lib.NvfPcSparseIndex(f["sorted"], f["cell_start"], f["super_mask"], f["super_first"], f["super_table"],
                                 f["hyper_table"], n, n_cells, n_supers, bits)


def test_sparse_entry_points_refuse_bad_arguments_without_a_launch():
    h = _lib.lib()
    ref = ctypes.byref
    bad = [_index(bits=9), _index(bits=13), _index(n=0), _index(n_cells=0), _index(n_cells=101), _index(n_supers=0),
           _index(n_supers=11), _index(bits=10, n=10 ** 6, n_cells=10 ** 5, n_supers=4097)]
    bad += [_index(**{name: None}) for name in ("sorted", "cell_start", "super_mask", "super_first", "super_table",
                                                "hyper_table")]
    for ix in bad:
        assert h.nvf_pc_sparse_build(ref(ix), 8, 8, None) == -1
        assert h.nvf_pc_nearest_sparse(8, 10, ref(ix), 8, 8, None) == -1
        assert h.nvf_pc_knn_normals_sparse(ref(ix), 8, 12, 8, None, None) == -1
    ok = _index()
    assert h.nvf_pc_sparse_build(None, 8, 8, None) == -1
    assert h.nvf_pc_sparse_build(ref(ok), None, 8, None) == -1
    assert h.nvf_pc_sparse_build(ref(ok), 8, None, None) == -1
    assert h.nvf_pc_nearest_sparse(None, 10, ref(ok), 8, 8, None) == -1
    assert h.nvf_pc_nearest_sparse(8, 0, ref(ok), 8, 8, None) == -1
    assert h.nvf_pc_nearest_sparse(8, 10, None, 8, 8, None) == -1
    assert h.nvf_pc_nearest_sparse(8, 10, ref(ok), None, 8, None) == -1
    assert h.nvf_pc_nearest_sparse(8, 10, ref(ok), 8, None, None) == -1
    assert h.nvf_pc_knn_normals_sparse(None, 8, 12, 8, None, None) == -1
    assert h.nvf_pc_knn_normals_sparse(ref(ok), None, 12, 8, None, None) == -1
    assert h.nvf_pc_knn_normals_sparse(ref(ok), 8, 12, None, None, None) == -1
    assert h.nvf_pc_knn_normals_sparse(ref(ok), 8, 2, 8, None, None) == -1           # k < 3
    assert h.nvf_pc_knn_normals_sparse(ref(ok), 8, 33, 8, None, None) == -1          # k > 32
    assert h.nvf_pc_knn_normals_sparse(ref(_index(n=10, n_cells=5)), 8, 12, 8, None, None) == -1     # n < k
