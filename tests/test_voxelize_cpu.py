"""What the voxeliser needs of the host (nvfpcc_amd/voxelize.py, nvfpcc_amd/ply_io.py, the command line): the vox_pack
bytes, the fit, the float PLY reader and writer, the refusals -- and the numpy reference itself (tests/voxelize_ref.py)
on the properties the GPU tests rely on.  Nothing here touches a GPU."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from nvfpcc_amd import ply_io, voxelize as vx
from tests import voxelize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, S = (-3.2, 1e3, 7.5), 0.0137


# ---- vox_pack ---------------------------------------------------------------------------------------------------------
def test_pack_is_34_bytes_and_round_trips():
    for lat in (vx.Lattice(10, O, S), vx.Lattice(12, (0.0, -0.5, 1e300), 5e-324 * 2 ** 60), vx.Lattice(11, (1, 2, 3), 1)):
        data = vx.pack(lat)
        assert isinstance(data, bytes) and len(data) == 34 == vx.PACK_BYTES
        assert data[0] == 1 and data[1] == lat.bits
        assert data[2:] == struct.pack("<4d", *lat.origin, lat.step)
        back = vx.unpack(data)
        assert back == lat and isinstance(back, vx.Lattice) and back.inv == 1.0 / lat.step


@pytest.mark.parametrize("data, message", [
    (b"", "0 bytes, not 34"),
    (struct.pack("<BB4d", 1, 10, 0, 0, 0, 1) + b"\0", "35 bytes, not 34"),
    (struct.pack("<BB4d", 2, 10, 0, 0, 0, 1), "version 2"),
    (struct.pack("<BB4d", 0, 10, 0, 0, 0, 1), "version 0"),
    (struct.pack("<BB4d", 1, 9, 0, 0, 0, 1), "bits must be one of"),
    (struct.pack("<BB4d", 1, 13, 0, 0, 0, 1), "bits must be one of"),
    (struct.pack("<BB4d", 1, 10, 0, 0, 0, 0.0), "step must be finite and above 0"),
    (struct.pack("<BB4d", 1, 10, 0, 0, 0, -1.0), "step must be finite and above 0"),
    (struct.pack("<BB4d", 1, 10, 0, 0, 0, float("inf")), "step must be finite and above 0"),
    (struct.pack("<BB4d", 1, 10, 0, 0, 0, float("nan")), "step must be finite and above 0"),
    (struct.pack("<BB4d", 1, 10, 0, float("nan"), 0, 1.0), "origin must be three finite numbers"),
])
def test_unpack_refuses(data, message):
    with pytest.raises(ValueError, match="vox_pack: .*" + message):
        vx.unpack(data)


def test_lattice_refuses_what_unpack_refuses():
    for args in ((9, O, S), (True, O, S), (10, (0, 0), S), (10, O, 0.0), (10, O, float("nan")), (10, O, 1e-320)):
        with pytest.raises(ValueError, match="lattice"):
            vx.Lattice(*args)


# ---- fit --------------------------------------------------------------------------------------------------------------
def test_fit():
    lat = vx.fit((-1.0, 2.0, 3.0), (1.0, 2.5, 13.23), 10)
    assert lat == vx.Lattice(10, (-1.0, 2.0, 3.0), (13.23 - 3.0) / 1023.0)           # the largest extent, not centred
    assert vx.fit((0, 0, 0), (4095, 1, 1), 12).step == 1.0
    zero = vx.fit((-0.0, 5.0, -0.0), (-0.0, 5.0, -0.0), 11)                           # no extent: step 1.0
    assert zero.step == 1.0 and zero.origin == (0.0, 5.0, 0.0)
    assert not any(np.signbit(v) for v in zero.origin)                                # -0.0 became +0.0
    with pytest.raises(ValueError, match="no finite point"):
        vx.fit((np.inf,) * 3, (-np.inf,) * 3, 10)
    x = np.random.default_rng(0).normal(size=(1000, 3)) * (3, 50, 7) + (1e3, -20, 0.1)
    ref = R.fit(x, 11)
    assert vx.fit(x.min(0), x.max(0), 11) == vx.Lattice(*ref)
    q = R.quantize(x, ref)
    assert q.min() == 0 and q.max() == 2047                                           # a fitted lattice holds its cloud


# ---- the reference meets what the GPU tests rely on -------------------------------------------------------------------
@pytest.mark.parametrize("bits", [10, 11, 12])
def test_reference_maps_a_jittered_integer_cloud_back(bits):
    rng = np.random.default_rng(bits)
    lat = R.RefLattice(bits, O, S)
    q = rng.integers(0, 1 << bits, size=(50000, 3))
    q[:4] = [[0, 0, 0], [(1 << bits) - 1] * 3, [0, (1 << bits) - 1, 0], [(1 << bits) - 1, 0, 0]]
    for jitter in (0.0, 0.25, -0.25, rng.uniform(-0.25, 0.25, size=q.shape)):
        x = np.asarray(O) + q * S + jitter * S
        assert np.array_equal(R.quantize(x, lat), q)
        assert np.array_equal(R.quantize(x.astype(np.float32).astype(np.float64), lat), q)      # float32-rounded inputs
    v = R.voxelize(np.asarray(O) + np.concatenate([q, q[:100]]) * S, bits, lat)
    uq, counts = np.unique(np.concatenate([q, q[:100]]), axis=0, return_counts=True)
    assert np.array_equal(v.points, uq) and np.array_equal(v.counts, counts) and v.n_in == len(q) + 100
    assert v.points.dtype == np.int32 and v.max_err2 < (1e-9 * S) ** 2 * 3


def test_reference_rounds_ties_up():
    lat = R.RefLattice(10, (1.0, -2.0, 0.0), 0.25)        # everything below is exact in float64
    k = np.arange(0, 1023)
    x = np.stack([1.0 + (k + 0.5) * 0.25, -2.0 + (k + 0.5) * 0.25, (k + 0.5) * 0.25], 1)
    assert np.array_equal(R.quantize(x, lat), np.stack([k + 1] * 3, 1))
    nonfinite, outside, _ = R.classify(np.array([[1.0 - 0.125, -2.0, 0.0], [1.0, -2.0, 1023.5 * 0.25],
                                                 [1.0 - 0.126, -2.0, 0.0], [np.nan, 0, 0], [0, np.inf, 2000.0]]), lat)
    assert outside.tolist() == [False, True, True, False, False] and nonfinite.tolist() == [False, False, False, True, True]


@pytest.mark.parametrize("bits, origin, step", [(10, O, S), (11, (1e3, -1e3, 999.999), 1.0 / 3), (12, (0.1, 0.2, 0.3), 1e-3),
                                                (12, (-512.0, 0.0, 77.0), 2.0 ** -4)])
def test_reference_is_idempotent(bits, origin, step):
    lat = R.RefLattice(bits, origin, step)
    q = np.random.default_rng(1).integers(0, 1 << bits, size=(200000, 3))
    assert np.array_equal(R.quantize(R.to_source(q, lat), lat), q)
    assert np.array_equal(R.to_source(q >> 2, lat, level=2), np.asarray(origin) + (q >> 2) * (4 * step))


# ---- PLY with float coordinates ---------------------------------------------------------------------------------------
XYZ = np.array([[1.5, 1e2, -0.0], [-3.25, 0.1, 7.0], [1e-3, -1e10, 2.5], [0.0, 1.0, 2.0]])


def _binary(path, order, kind):
    """x, y, z of XYZ as `kind`, between other properties, in the byte order `order`."""
    fmt = "binary_little_endian" if order == "<" else "binary_big_endian"
    name = {"f4": "float", "f8": "double"}[kind]
    props = [("red", "u1", "uchar"), ("y", kind, name), ("nx", "f4", "float"), ("x", kind, name), ("z", kind, name)]
    rec = np.zeros(len(XYZ), np.dtype([(n, order + t) for n, t, _ in props]))
    for a, axis in enumerate("xyz"):
        rec[axis] = XYZ[:, a]
    head = f"ply\nformat {fmt} 1.0\nelement vertex {len(XYZ)}\n" + "".join(f"property {w} {n}\n" for n, _, w in props)
    with open(path, "wb") as f:
        f.write((head + "end_header\n").encode() + rec.tobytes())


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("kind", ["f4", "f8"])
def test_read_float_binary(tmp_path, order, kind):
    path = str(tmp_path / "c.ply")
    _binary(path, order, kind)
    xyz, nrm = ply_io.read_ply(path, coords="float")
    want = XYZ.astype(kind).astype(np.float64)
    assert nrm is None and xyz.dtype == np.float64 and xyz.shape == (4, 3)
    assert np.array_equal(xyz.view(np.int64), want.view(np.int64))                    # -0.0 stays -0.0
    with pytest.raises(ValueError, match="coordinates must be integers"):
        ply_io.read_ply(path)                                                         # the default is what it was
    with pytest.raises(ValueError, match="coords must be"):
        ply_io.read_ply(path, coords="double")


def test_read_float_ascii_by_column_name(tmp_path):
    path = str(tmp_path / "a.ply")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment x y z are not the first columns\nelement vertex 4\nproperty uchar red\n"
                "property float z\nproperty float nx\nproperty float x\nproperty float y\nend_header\n"
                "255 -0.0 0.5 1.5 1e2\n0 7 0.5 -3.25 0.1\n\n7 2.5 0 1e-3 -1e10\n9 2 1 0 1\n")
    xyz, _ = ply_io.read_ply(path, coords="float")
    assert xyz.dtype == np.float64 and np.array_equal(xyz.view(np.int64), XYZ.view(np.int64))
    bad = str(tmp_path / "nan.ply")
    ply_io.write_ply_float(bad, [[np.nan, np.inf, -np.inf], [1, 2, 3]])
    xyz, _ = ply_io.read_ply(bad, coords="float")                                     # passed through for the voxeliser
    assert np.isnan(xyz[0, 0]) and xyz[0, 1] == np.inf and xyz[0, 2] == -np.inf and xyz[1].tolist() == [1, 2, 3]
    short = str(tmp_path / "short.ply")
    with open(short, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                "1 2 3\n4 5 6\n")
    with pytest.raises(ValueError, match="fewer vertex values"):
        ply_io.read_ply(short, coords="float")


@pytest.mark.parametrize("fmt", ["ascii", "binary"])
def test_integer_file_reads_as_before_and_widens_exactly(tmp_path, fmt):
    path = str(tmp_path / "i.ply")
    pts = np.random.default_rng(2).integers(0, 4096, size=(500, 3))
    ply_io.write_ply(path, pts, fmt=fmt)
    xyz, nrm = ply_io.read_ply(path)
    assert xyz.dtype == np.int64 and np.array_equal(xyz, pts) and nrm is None
    xf, _ = ply_io.read_ply(path, coords="float")
    assert xf.dtype == np.float64 and np.array_equal(xf, pts.astype(np.float64))


@pytest.mark.parametrize("fmt", ["ascii", "binary"])
def test_write_float_then_read_is_bit_exact(tmp_path, fmt):
    rng = np.random.default_rng(3)
    x = np.concatenate([XYZ, rng.normal(size=(2000, 3)) * 10.0 ** rng.integers(-8, 9, size=(2000, 3)),
                        [[5e-324, 1.7976931348623157e308, -2.2250738585072014e-308], [0.1, 1 / 3, 2 / 3]]])
    path = str(tmp_path / "f.ply")
    ply_io.write_ply_float(path, x, fmt)
    with open(path, "rb") as f:
        head = f.read(200)
    assert (b"format ascii 1.0" if fmt == "ascii" else b"format binary_little_endian 1.0") in head
    assert b"property double x\nproperty double y\nproperty double z\nend_header\n" in head
    back, _ = ply_io.read_ply(path, coords="float")
    assert back.dtype == np.float64 and np.array_equal(back.view(np.int64), x.view(np.int64))
    with pytest.raises(ValueError, match="fmt must be"):
        ply_io.write_ply_float(path, x, "text")


# ---- the command line refuses, before anything is loaded ---------------------------------------------------------------
REFUSALS = [
    (["train", "c.ply", "--voxelize"], "--voxelize needs --from_ply"),
    (["encode", "c.ply", "--voxelize"], "--voxelize needs --from_ply"),
    (["encode", "c.ply", "--from_ply", "--vox_step", "0.5"], "is the lattice step of --voxelize; give --voxelize too"),
    (["train", "c.ply", "--from_ply", "--voxelize", "--vox_origin", "1", "2", "3"], "give --vox_step too"),
    (["encode", "c.ply", "--from_ply", "--vox_origin", "1", "2", "3"], "give both too"),
    (["encode", "c.ply", "--from_ply", "--voxelize", "--vox_step", "0"], "is not a finite step above 0"),
    (["encode", "c.ply", "--from_ply", "--voxelize", "--vox_step", "-0.5"], "is not a finite step above 0"),
    (["train", "c.ply", "--from_ply", "--voxelize", "--vox_step", "inf"], "is not a finite step above 0"),
    (["train", "c.ply", "--from_ply", "--voxelize", "--vox_step", "nan"], "is not a finite step above 0"),
    (["train", "c_%04d.ply", "--from_ply", "--voxelize", "--gof", "2"], "give --vox_step / --vox_origin"),
    (["encode", "c_%04d.ply", "--from_ply", "--voxelize", "--gof", "2"], "give --vox_step / --vox_origin"),
    (["decode", "p.pk", "--voxelize"], "decode reads the lattice from the pack's vox_pack"),
    (["encode", "c.ply", "--source_frame"], "--source_frame is a switch of decode"),
]


@pytest.mark.parametrize("argv, message", REFUSALS)
def test_command_line_refuses(argv, message, tmp_path, monkeypatch):
    """The files named do not exist and there may be no device: a refusal that came after either would not be this one."""
    import NVFPCC
    monkeypatch.chdir(tmp_path)
    args = NVFPCC.build_parser().parse_args(argv)
    with pytest.raises(SystemExit) as e:
        {"train": NVFPCC.train, "encode": NVFPCC.encode, "decode": NVFPCC.decode}[args.command](args)
    assert isinstance(e.value.code, str) and message in e.value.code and e.value.code.startswith(argv[0] + ":")


def test_an_origin_as_the_voxelize_line_prints_it_can_be_typed_back():
    import NVFPCC
    origin = (-1.2e-05, -3.2, -1.5e+20)
    argv = ["encode", "c.ply", "--from_ply", "--voxelize", "--vox_step", repr(1e-3), "--vox_origin"] + [repr(v) for v in origin]
    args = NVFPCC.build_parser().parse_args(argv + ["--pack_octree"])
    assert tuple(args.vox_origin) == origin and args.vox_step == 1e-3 and args.pack_octree is True
    NVFPCC._voxelize_refusals(args)
    assert args.vox_lattice == vx.Lattice(10, origin, 1e-3)
    plain = NVFPCC.build_parser().parse_args(["encode", "c.ply"])
    assert not any(hasattr(plain, k) for k in ("voxelize", "vox_step", "vox_origin", "source_frame", "vox_lattice"))


def test_a_refusal_through_the_real_command_line_and_the_module(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "NVFPCC.py"), "encode", "c.ply", "--voxelize"], cwd=tmp_path, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "--voxelize needs --from_ply" in r.stderr and "Traceback" not in r.stderr
    r = subprocess.run([sys.executable, "-m", "nvfpcc_amd.voxelize", "in.ply", "out.ply", "--vox_origin", "0", "0", "1"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "give --vox_step too" in r.stderr and "Traceback" not in r.stderr
    assert not os.path.exists(tmp_path / "out.ply")
