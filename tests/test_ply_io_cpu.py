"""Host half of nvfpcc_amd.ply_io: the header parser, the binary reader and writer, the ASCII writer without a device,
and the refusals of the PLY entries of the C ABI that come before any HIP call."""
import ctypes
import struct

import numpy as np
import pytest

from nvfpcc_amd import _lib, ply_io, recon

SPELLINGS = [("char", "int8"), ("uchar", "uint8"), ("short", "int16"), ("ushort", "uint16"), ("int", "int32"),
             ("uint", "uint32"), ("float", "float32"), ("double", "float64")]
XYZ = "property float x\nproperty float y\nproperty float z\n"


def header(lines, eol="\n"):
    return (eol.join(["ply"] + lines + ["end_header"]) + eol).encode("ascii")


# ---- header ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eol", ["\n", "\r\n"])
@pytest.mark.parametrize("second", [0, 1])
def test_header_knows_every_type_under_both_names(eol, second):
    props = [f"property {names[second]} p{i}" for i, names in enumerate(SPELLINGS)]
    raw = header(["format binary_big_endian 1.0", "comment a comment with end_header in it", "element vertex 7"] + props +
                 ["property double x", "property float y", "property int z"], eol) + b"body"
    h = ply_io.parse_header(raw, "f.ply")
    assert h.format == "binary_big_endian" and raw[h.body:] == b"body"
    (v,) = h.elements
    assert (v.name, v.count) == ("vertex", 7)
    assert [p.type for p in v.props[:8]] == [canonical for _, canonical in SPELLINGS]
    assert [(p.type, p.name, p.is_list) for p in v.props[8:]] == [("float64", "x", False), ("float32", "y", False),
                                                                 ("int32", "z", False)]


def test_header_lists_elements_in_order_with_their_lists_marked():
    raw = header(["format ascii 1.0", "element camera 2", "property float view", "element vertex 3"] + XYZ.split("\n")[:3] +
                 ["element face 1", "property list uchar int vertex_indices"])
    h = ply_io.parse_header(raw)
    assert [(e.name, e.count) for e in h.elements] == [("camera", 2), ("vertex", 3), ("face", 1)]
    assert h.elements[2].props == [ply_io.Property("int32", "vertex_indices", True)]
    assert h.body == len(raw)
    assert h.format == "ascii"


@pytest.mark.parametrize("raw, fault", [
    (b"plx\nformat ascii 1.0\nelement vertex 0\n" + XYZ.encode() + b"end_header\n", "magic"),
    (b"ply\nformat ascii 1.0\nelement vertex 0\n" + XYZ.encode(), "no end_header"),
    (header(["format ascii 1.0", "element face 1", "property int a"]), "no vertex element"),
    (header(["format ascii 1.0", "element vertex 1", "property float x", "property float z"]), "no 'y' property"),
    (header(["format ascii 1.0", "element vertex 1", "property float y", "property float z"]), "no 'x' property"),
    (header(["format ascii 1.0", "element vertex 1", "property float x", "property float y"]), "no 'z' property"),
    (header(["format ascii 1.0", "element vertex 1"] + XYZ.split("\n")[:3] + ["property list uchar int n"]),
     "vertex element has a list property"),
    (header(["format binary_little_endian 1.0", "element face 1", "property list uchar int n", "element vertex 1"] +
            XYZ.split("\n")[:3]), "list property in element 'face' before the vertices"),
    (header(["format ascii 1.0", "element vertex 1", "property half x", "property float y", "property float z"]),
     "unknown PLY property type 'half'"),
    (header(["format ebcdic 1.0", "element vertex 1"] + XYZ.split("\n")[:3]), "format must be one of"),
])
def test_header_faults_name_the_file_and_the_fault(raw, fault):
    with pytest.raises(ValueError) as e:
        ply_io.parse_header(raw, "some/cloud.ply")
    assert "some/cloud.ply" in str(e.value) and fault in str(e.value)


def test_an_ascii_file_may_hold_a_list_before_the_vertices():
    raw = header(["format ascii 1.0", "element face 1", "property list uchar int n", "element vertex 1"] + XYZ.split("\n")[:3])
    assert ply_io.parse_header(raw).elements[0].props[0].is_list


# ---- binary reader -------------------------------------------------------------------------------------------------------
MIXED = ["property uchar red", "property uchar green", "property uchar blue", "property double z", "property float y",
         "property int x", "property float nx", "property float ny", "property float nz"]
ROWS = [(255, 0, 7, 3.0, 2.0, 1, 0.1, -0.25, 1e-3), (1, 2, 3, 4095.0, 0.0, 2047, 0.6, 0.8, 0.0)]


def mixed_file(path, order, camera=False, rows=ROWS, cut=0):
    name = {"<": "binary_little_endian", ">": "binary_big_endian"}[order]
    cam = ["element camera 2", "property float view", "property short id"] if camera else []
    body = b"".join(struct.pack(order + "fh", 1.5, k) for k in range(2)) if camera else b""
    body += b"".join(struct.pack(order + "BBBdfifff", *r) for r in rows)
    with open(path, "wb") as f:
        f.write(header([f"format {name} 1.0"] + cam + [f"element vertex {len(rows)}"] + MIXED) + body[:len(body) - cut])
    return str(path)


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("camera", [False, True])
def test_binary_reader_finds_xyz_and_normals_by_name(tmp_path, order, camera):
    path = mixed_file(tmp_path / "m.ply", order, camera)
    xyz, normals = ply_io.read_ply(path, normals=True)
    assert xyz.dtype == np.int64 and np.array_equal(xyz, [[1, 2, 3], [2047, 0, 4095]])
    want = np.array([[np.float32(v) for v in r[6:]] for r in ROWS], np.float64)      # the file's float32 values, exactly
    assert normals.dtype == np.float64 and np.array_equal(normals, want)
    assert ply_io.read_ply(path)[1] is None


@pytest.mark.parametrize("bad", [2.5, float("nan"), float("inf")])
def test_binary_reader_refuses_a_coordinate_that_is_no_integer(tmp_path, bad):
    rows = [ROWS[0], ROWS[1][:4] + (bad,) + ROWS[1][5:]]
    with pytest.raises(ValueError, match="coordinates must be integers"):
        ply_io.read_ply(mixed_file(tmp_path / "b.ply", "<", rows=rows))


def test_binary_reader_refuses_a_truncated_body_and_says_what_it_found(tmp_path):
    path = mixed_file(tmp_path / "t.ply", ">", camera=True, cut=5)
    with pytest.raises(ValueError) as e:
        ply_io.read_ply(path)
    assert str(e.value) == (f"{path}: binary PLY declares 62 bytes of vertex data, 57 follow "
                            f"(an ASCII body under a binary header?)")


# ---- writer --------------------------------------------------------------------------------------------------------------
CLOUD = np.array([[0, 1023, 5], [17, 3, 1000], [4095, 4095, 0], [-3, 10, 99]])


def test_ascii_writer_without_a_device_gives_the_bytes_of_write_ply_ascii(tmp_path):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    recon.write_ply_ascii(a, CLOUD)
    ply_io.write_ply(b, CLOUD)
    assert open(a, "rb").read() == open(b, "rb").read()
    ply_io.write_ply(b, CLOUD.astype(np.float64), fmt="ascii", device="cpu")
    assert open(a, "rb").read() == open(b, "rb").read()
    xyz, _ = ply_io.read_ply(b)
    assert np.array_equal(xyz, CLOUD)


def test_binary_writer_reads_back_to_the_same_points(tmp_path):
    import torch
    path = str(tmp_path / "c.ply")
    pts = np.concatenate([CLOUD, [[(1 << 24) - 1, -(1 << 24) + 1, 0]]])
    for given in (pts, pts.astype(np.float64), torch.from_numpy(pts)):
        ply_io.write_ply(path, given, fmt="binary")
        raw = open(path, "rb").read()
        assert raw.startswith(b"ply\nformat binary_little_endian 1.0\ncomment Created by nvfpcc_amd\nelement vertex 5\n"
                              b"property float x\nproperty float y\nproperty float z\nend_header\n")
        assert len(raw) == ply_io.parse_header(raw).body + 5 * 12
        xyz, normals = ply_io.read_ply(path, normals=True)
        assert np.array_equal(xyz, pts) and normals is None


@pytest.mark.parametrize("value", [1 << 24, -(1 << 24), 1 << 31])
def test_binary_writer_refuses_what_float32_cannot_hold(tmp_path, value):
    with pytest.raises(ValueError, match="2\\^24"):
        ply_io.write_ply(str(tmp_path / "c.ply"), np.array([[0, value, 0]]), fmt="binary")
    assert not (tmp_path / "c.ply").exists()


@pytest.mark.parametrize("points", [np.array([[0.5, 1, 2]]), np.array([[np.nan, 1, 2]]), np.zeros((3, 2), np.int64),
                                    np.zeros(3, np.int64), np.zeros((1, 3), bool)])
@pytest.mark.parametrize("fmt", ["ascii", "binary"])
def test_writer_refuses_what_is_no_integer_cloud(tmp_path, points, fmt):
    with pytest.raises(ValueError):
        ply_io.write_ply(str(tmp_path / "c.ply"), points, fmt=fmt)
    with pytest.raises(ValueError):
        ply_io.write_ply(str(tmp_path / "c.ply"), CLOUD, fmt="text")


def test_a_stub_of_write_ply_ascii_set_after_import_is_honoured(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(recon, "write_ply_ascii", lambda fn, pts: seen.append((fn, np.asarray(pts))))
    path = str(tmp_path / "never.ply")
    ply_io.write_ply(path, CLOUD, device="cpu")
    assert len(seen) == 1 and seen[0][0] == path and np.array_equal(seen[0][1], CLOUD)
    assert not (tmp_path / "never.ply").exists()


def test_host_reader_of_ascii_is_read_ply_points(tmp_path):
    path = str(tmp_path / "n.ply")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float nx\nproperty float ny\nproperty float nz\n"
                "property float z\nproperty float y\nproperty float x\nend_header\n0.1 0.2 0.3 3 2 1\n0 0 1e-3 6.0 5 4\n")
    xyz, normals = ply_io.read_ply(path, normals=True)
    assert np.array_equal(xyz, [[1, 2, 3], [4, 5, 6]])
    assert np.array_equal(normals, [[0.1, 0.2, 0.3], [0.0, 0.0, 1e-3]])
    assert ply_io.read_ply(path)[1] is None


# ---- the C entries, before any HIP call ----------------------------------------------------------------------------------
DUMMY = 0x1000      # a non-null address nobody dereferences


def test_ply_entries_refuse_null_and_negative_arguments_and_accept_empty_input():
    h, d = _lib.lib(), DUMMY
    calls = {
        "count_lines": (h.nvf_ply_count_lines, [d, 64, 64, d, None], {0: None, 1: -1, 2: 0, 3: None}, {1: 0}),
        "line_starts": (h.nvf_ply_line_starts, [d, 64, 64, d, d, 4, None], {0: None, 1: -1, 2: 0, 3: None, 4: None, 5: -1},
                        {1: 0, 5: 0}),
        "parse_xyz": (h.nvf_ply_parse_xyz, [d, 64, d, 0, 4, 3, 0, 1, 2, d, d, None],
                      {0: None, 1: -1, 2: None, 3: -1, 4: -1, 5: 2, 6: -1, 7: 3, 8: 1, 9: None, 10: None}, {4: 0}),
        "format_sizes": (h.nvf_ply_format_sizes, [d, 4, d, None], {0: None, 1: -1, 2: None}, {1: 0}),
        "format_xyz": (h.nvf_ply_format_xyz, [d, d, 4, d, 64, None], {0: None, 1: None, 2: -1, 3: None, 4: -1}, {2: 0, 4: 0}),
    }
    for name, (fn, good, refused, empty) in calls.items():
        for i, v in refused.items():
            args = list(good)
            args[i] = v
            assert fn(*args) == -1, (name, i, v)
        for i, v in empty.items():
            args = list(good)
            args[i] = v
            assert fn(*args) == 0, (name, i, v)


# ---- command line --------------------------------------------------------------------------------------------------------
def test_ply_format_parses_and_is_absent_when_not_given():
    import NVFPCC
    p = NVFPCC.build_parser()
    assert p.parse_args(["decode", "pack.pk", "--ply_format", "binary"]).ply_format == "binary"
    assert p.parse_args(["encode", "x.ply", "--ply_format", "ascii"]).ply_format == "ascii"
    assert not hasattr(p.parse_args(["decode", "pack.pk"]), "ply_format")
    with pytest.raises(SystemExit):
        p.parse_args(["decode", "pack.pk", "--ply_format", "text"])
