"""Host-side parts of the D1 / D2 geometry metrics (nvfpcc_amd.pc_metrics): the PLY reader, input checks that run
before any device work, the workspace query of the C ABI and the CLI flag."""
import numpy as np
import pytest

from nvfpcc_amd import _lib, pc_metrics
from nvfpcc_amd.pc_error import main as pc_error_main


def _write(path, header_props, rows, fmt="ascii 1.0", extra_elements=""):
    with open(path, "w") as f:
        f.write(f"ply\nformat {fmt}\n{extra_elements}element vertex {len(rows)}\n")
        for p in header_props:
            f.write(f"property float {p}\n")
        f.write("end_header\n")
        for r in rows:
            f.write(" ".join(str(v) for v in r) + "\n")
    return str(path)


def test_read_ply_points_by_property_name(tmp_path):
    rows = [(0.5, 3, 2, 1), (0.25, 6, 5, 4)]
    xyz, normals = pc_metrics.read_ply_points(_write(tmp_path / "a.ply", ["red", "z", "y", "x"], rows))
    assert xyz.dtype == np.int64
    assert np.array_equal(xyz, [[1, 2, 3], [4, 5, 6]])
    assert normals is None


def test_read_ply_points_returns_normals(tmp_path):
    rows = [(1, 2, 3, 0, 0, 1), (4, 5, 6, 0.6, 0.8, 0)]
    xyz, normals = pc_metrics.read_ply_points(_write(tmp_path / "n.ply", ["x", "y", "z", "nx", "ny", "nz"], rows))
    assert np.array_equal(xyz, [[1, 2, 3], [4, 5, 6]])
    assert np.allclose(normals, [[0, 0, 1], [0.6, 0.8, 0]])


def test_read_ply_points_skips_elements_before_the_vertices(tmp_path):
    path = tmp_path / "c.ply"
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement camera 1\nproperty float view\n"
                "element vertex 1\nproperty double x\nproperty double y\nproperty double z\nend_header\n9\n7 8 9\n")
    xyz, _ = pc_metrics.read_ply_points(str(path))
    assert np.array_equal(xyz, [[7, 8, 9]])


def test_read_ply_points_reads_what_the_codec_writes(tmp_path):
    from nvfpcc_amd.recon import write_ply_ascii
    pts = np.array([[0, 1023, 5], [17, 3, 1000]])
    write_ply_ascii(str(tmp_path / "rc.ply"), pts)
    xyz, normals = pc_metrics.read_ply_points(str(tmp_path / "rc.ply"))
    assert np.array_equal(xyz, pts) and normals is None


@pytest.mark.parametrize("fmt", ["binary_little_endian 1.0", "binary_big_endian 1.0"])
def test_read_ply_points_refuses_binary(tmp_path, fmt):
    with pytest.raises(ValueError, match="ASCII"):
        pc_metrics.read_ply_points(_write(tmp_path / "b.ply", ["x", "y", "z"], [], fmt=fmt))


def test_read_ply_points_refuses_empty_and_broken_files(tmp_path):
    (tmp_path / "empty.ply").write_text("")
    with pytest.raises(ValueError):
        pc_metrics.read_ply_points(str(tmp_path / "empty.ply"))
    (tmp_path / "short.ply").write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\n"
                                        "property float z\nend_header\n1 2 3\n")
    with pytest.raises(ValueError, match="fewer"):
        pc_metrics.read_ply_points(str(tmp_path / "short.ply"))
    with pytest.raises(ValueError, match="integers"):
        pc_metrics.read_ply_points(_write(tmp_path / "f.ply", ["x", "y", "z"], [(1.5, 2, 3)]))


GOOD = np.array([[0, 0, 0], [1023, 1023, 1023], [5, 6, 7]])


@pytest.mark.parametrize("bad", [
    np.array([[0, 0, 1024]]),                   # outside [0, 1024)
    np.array([[-1, 0, 0]]),                     # negative
    np.array([[0.5, 1.0, 2.0]]),                # not an integer
    np.array([[np.nan, 1.0, 2.0]]),
    np.zeros((0, 3), np.int64),                 # empty cloud
    np.array([1, 2, 3]),                        # not [n, 3]
])
def test_geometry_psnr_rejects_bad_clouds_before_any_device_work(bad):
    with pytest.raises(ValueError):
        pc_metrics.geometry_psnr(GOOD, bad)
    with pytest.raises(ValueError):
        pc_metrics.geometry_psnr(bad, GOOD)
    with pytest.raises(ValueError):
        pc_metrics.nearest(bad, GOOD)


def test_integral_float_coordinates_are_accepted():
    assert np.array_equal(pc_metrics._points(np.array([[1.0, 2.0, 1023.0]]), "x"), [[1, 2, 1023]])


@pytest.mark.parametrize("k", [2, 33, 2.5])
def test_knn_out_of_range_is_refused(k):
    with pytest.raises(ValueError, match="knn"):
        pc_metrics.geometry_psnr(GOOD, GOOD, knn=k)


def test_too_few_points_for_the_normal_estimate():
    with pytest.raises(ValueError, match="at least"):
        pc_metrics.estimate_normals(GOOD, k=12)


def test_ref_normals_must_match_the_cloud():
    with pytest.raises(ValueError, match="ref_normals"):
        pc_metrics.geometry_psnr(GOOD, GOOD, ref_normals=np.zeros((2, 3)))


def test_psnr_convention():
    assert pc_metrics.psnr(0.0) == float("inf")
    assert pc_metrics.psnr(3 * 1023.0 ** 2) == 0.0
    assert abs(pc_metrics.psnr(1.0) - 10 * np.log10(3 * 1023.0 ** 2)) < 1e-12


def test_workspace_query_needs_no_gpu():
    h = _lib.lib()
    assert h.nvf_pc_workspace_bytes(0, 0) == 0
    small, large = h.nvf_pc_workspace_bytes(100, 10), h.nvf_pc_workspace_bytes(800_000, 10)
    assert 0 < small <= large
    assert h.nvf_pc_workspace_bytes(10, 800_000) == large        # covers both directions of a pair


def test_entry_points_refuse_bad_sizes_without_a_launch():
    h = _lib.lib()
    assert h.nvf_pc_nearest(None, 0, None, None, 0, None, None, None) == -1
    assert h.nvf_pc_knn_normals(1, 1, 1, 100, 2, 1, None, None) == -1        # k < 3
    assert h.nvf_pc_knn_normals(1, 1, 1, 100, 33, 1, None, None) == -1       # k > 32
    assert h.nvf_pc_knn_normals(1, 1, 1, 10, 12, 1, None, None) == -1        # n < k
    assert h.nvf_pc_error_sums(1, 100, 1, 1, None, 0, 1, 1, 1, 0, None) == -2   # workspace too small


def test_pc_error_cli_exits_nonzero_on_bad_input(tmp_path, capsys):
    a = _write(tmp_path / "a.ply", ["x", "y", "z"], [(1, 2, 3)])
    b = _write(tmp_path / "b.ply", ["x", "y", "z"], [(1, 2, 3)], fmt="binary_little_endian 1.0")
    assert pc_error_main([a, b]) == 1
    assert "ASCII" in capsys.readouterr().err
    assert pc_error_main([a, str(tmp_path / "missing.ply")]) == 1


def test_cli_parser_has_ref_ply():
    import NVFPCC
    p = NVFPCC.build_parser()
    assert p.parse_args(["decode", "pack.pk"]).ref_ply is None
    assert p.parse_args(["encode", "x.ply", "--ref_ply", "orig.ply"]).ref_ply == "orig.ply"
