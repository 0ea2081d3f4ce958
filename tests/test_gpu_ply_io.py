"""PLY text on the device (csrc/ply_io.hip through ops.ply_parse_xyz / ops.ply_format_xyz and nvfpcc_amd.ply_io): the
parser against the two host readers, exactly; what it hands back to the host reader; its read and write bounds; the
formatter against recon.write_ply_ascii, byte for byte; and the command line through both."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

from nvfpcc_amd import ops, pc_metrics, ply_io, preprocess, recon

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SIZES = [1, 2, 255, 256, 257, 70_001]
CHUNKS = [64, ops.PLY_CHUNK]                  # 64: lines straddle chunks even in tiny files
DIGITS = [0, 9, 10, 99, 100, 999, 1000, 1023, 4095, 2_147_483_647]      # every digit count


@functools.lru_cache(maxsize=None)
def cloud(n):
    """n points whose coordinates cover every digit count, then random 12-bit ones (read-only)."""
    rng = np.random.default_rng(n)
    pts = rng.integers(0, 4096, size=(n, 3))
    k = min(n, len(DIGITS))
    pts[:k, 0], pts[:k, 1], pts[:k, 2] = DIGITS[:k], DIGITS[::-1][:k], np.roll(DIGITS, 3)[:k]
    pts.setflags(write=False)
    return pts


@pytest.fixture(scope="module")
def cloud_file(tmp_path_factory):
    """n -> (path of the file recon.write_ply_ascii writes for cloud(n), its bytes): written once, shared."""
    folder = tmp_path_factory.mktemp("clouds")

    @functools.lru_cache(maxsize=None)
    def get(n):
        path = str(folder / f"cloud{n}.ply")
        recon.write_ply_ascii(path, cloud(n))
        return path, open(path, "rb").read()
    return get


def device_parse(raw, chunk, tail=b""):
    """ops.ply_parse_xyz on the body of the PLY `raw` -> (xyz numpy, status list).  `tail`: bytes that follow the text
    in the device buffer it is a slice of."""
    h = ply_io.parse_header(raw)
    vi, v, col = ply_io._vertex(h)
    buf = torch.from_numpy(np.frombuffer(raw + tail, np.uint8).copy()).to(DEV)
    text = buf[h.body:len(raw)]
    xyz, status = ops.ply_parse_xyz(text, sum(e.count for e in h.elements[:vi]), v.count, len(v.props),
                                    (col["x"], col["y"], col["z"]), chunk=chunk)
    return xyz.cpu().numpy(), status.cpu().tolist()


def write(tmp_path, raw, name="f.ply"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(raw)
    return path


def ply(props, body, n, before="", eol="\n"):
    head = ["ply", "format ascii 1.0"] + ([before] if before else []) + [f"element vertex {n}"] + \
        [f"property float {p}" for p in props] + ["end_header"]
    return (eol.join(head) + eol).encode("ascii") + body.encode("ascii")


# ---- parse against the host readers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("n", SIZES)
def test_parse_equals_both_host_readers(cloud_file, n, chunk):
    path, raw = cloud_file(n)
    xyz, status = device_parse(raw, chunk)
    assert status == [0, 0, -1, -1]
    assert np.array_equal(xyz, cloud(n))
    if chunk == CHUNKS[0]:          # the host readers once per size
        assert np.array_equal(pc_metrics.read_ply_points(path)[0], cloud(n))
        assert np.array_equal(preprocess.read_ply_xyz(path), cloud(n))
        got, normals = ply_io.read_ply(path, device=DEV, normals=True)
        assert got.dtype == torch.int32 and got.is_cuda and normals is None
        assert np.array_equal(got.cpu().numpy(), cloud(n))


LAYOUTS = {
    "columns red z y x": ply(["red", "z", "y", "x"], "0.5 3 2 1\n0.25 6 5 4\n", 2),
    "elements before the vertices": ply(["x", "y", "z"], "9\n\n8\n7 8 9\n10 11 12\n", 2,
                                        before="element camera 3\nproperty float view"),
    "crlf": ply(["x", "y", "z"], "1 2 3\r\n4 5 6\r\n", 2, eol="\r\n"),
    "tabs, runs of spaces, leading spaces": ply(["x", "y", "z"], "  1\t\t2   3 \n\t4 5\t 6\t\n", 2),
    "signs, zeros after the point": ply(["x", "y", "z"], "12.000 +7 -3\n-0 5. 007\n0.0 -12.0 +0\n", 3),
    "no trailing newline": ply(["x", "y", "z"], "1 2 3\n4 5 1023", 2),
    "trailing blank lines": ply(["x", "y", "z"], "1 2 3\n4 5 6\n\n\n  \n", 2),
    "elements after the vertices": ply(["x", "y", "z"], "1 2 3\n4 5 6\n3 0 1 2\n", 2) .replace(
        b"end_header", b"element face 1\nproperty list uchar int vertex_indices\nend_header"),
    "colour and normal columns": ply(["nx", "x", "red", "y", "ny", "z", "nz"],
                                     "0.5 1 255 2 1e-3 3 -0.25\n-1e-3 4 0 5 nan 6 .5\n", 2),
    "more tokens than properties": ply(["x", "y", "z"], "1 2 3 4.5 abc\n4 5 6 7\n", 2),
    "a long line across many chunks": ply(["x", "red", "y", "z"], "1 " + " " * 300 + "0.125 2 3" + " " * 200 + "\n4 1 5 6\n", 2),
}


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_parse_layouts_equal_the_host_reader(tmp_path, name, chunk):
    raw = LAYOUTS[name]
    want, _ = pc_metrics.read_ply_points(write(tmp_path, raw))
    xyz, status = device_parse(raw, chunk)
    assert status == [0, 0, -1, -1]
    assert np.array_equal(xyz, want)


def test_ascii_normals_equal_the_host_readers(tmp_path):
    """xyz from the device, nx ny nz from np.loadtxt: the very float64 values read_ply_points (Python's float()) gives."""
    rng = np.random.default_rng(3)
    rows = "".join("%d %r %d %r %d %r\n" % (p[0], float(v[0]), p[1], float(np.float32(v[1])), p[2], float(v[2]) * 1e-5)
                   for p, v in zip(rng.integers(0, 1024, (300, 3)), rng.normal(size=(300, 3))))
    path = write(tmp_path, ply(["x", "nx", "y", "ny", "z", "nz"], "7\n" + rows, 300,
                               before="element camera 1\nproperty float view"))
    want_xyz, want_n = pc_metrics.read_ply_points(path)
    xyz, normals = ply_io.read_ply(path, device=DEV, normals=True, fallback=False)
    assert np.array_equal(xyz.cpu().numpy(), want_xyz)
    assert normals.dtype == np.float64 and np.array_equal(normals, want_n)


# ---- what goes back to the host ------------------------------------------------------------------------------------------
def outcome(fn):
    try:
        xyz, normals = fn()
    except ValueError as e:
        return type(e), str(e)
    return (xyz.cpu().numpy() if isinstance(xyz, torch.Tensor) else xyz), normals


@pytest.mark.parametrize("token", ["1.5", "1e2", "nan", "12345678901", "2147483648", "0x10", "1,5", "--1", "+", "1.0.0", "."])
def test_a_token_outside_the_grammar_goes_to_the_host_reader(tmp_path, token):
    lines = ["%d %d %d" % (i, i + 1, i + 2) for i in range(300)]
    lines[17] = lines[17] + " "
    lines[260] = f"3 {token} 4"
    lines[281] = f"{token} 1 2"
    raw = ply(["x", "y", "z"], "\n".join(lines) + "\n", 300)
    path = write(tmp_path, raw)
    for chunk in CHUNKS:
        _, status = device_parse(raw, chunk)
        assert status == [0, 2, -1, 260]
    want = outcome(lambda: pc_metrics.read_ply_points(path))
    got = outcome(lambda: ply_io.read_ply(path, device=DEV))
    if isinstance(want[0], type):
        assert got == want
    else:
        assert np.array_equal(got[0], want[0]) and got[1] is None
    with pytest.raises(ValueError, match="vertex 260 .*grammar"):
        ply_io.read_ply(path, device=DEV, fallback=False)


def test_a_token_outside_the_grammar_in_a_skipped_column_is_not_looked_at(tmp_path):
    raw = ply(["x", "red", "y", "z"], "1 1.5 2 3\n4 1e2 5 6\n7 12345678901 8 9\n", 3)
    xyz, status = device_parse(raw, 64)
    assert status == [0, 0, -1, -1] and np.array_equal(xyz, [[1, 2, 3], [4, 5, 6], [7, 8, 9]])


@pytest.mark.parametrize("body, n, vertex", [("1 2 3\n4 5\n7 8 9\n", 3, 1), ("1 2 3\n\n7 8 9\n", 3, 1),
                                             ("1 2 3\n4 5 6\n", 3, 2), ("1 2 3\n4 5 6", 4, 2), ("", 2, 0)])
def test_missing_values_raise_with_the_vertex(tmp_path, body, n, vertex):
    raw = ply(["x", "y", "z"], body, n)
    path = write(tmp_path, raw)
    _, status = device_parse(raw, 64)
    assert status[0] >= 1 and status[2] == vertex and status[1] == 0
    with pytest.raises(ValueError, match="fewer vertex values than its header declares"):
        pc_metrics.read_ply_points(path)
    with pytest.raises(ValueError) as e:
        ply_io.read_ply(path, device=DEV)
    assert str(e.value) == f"{path}: PLY holds fewer vertex values than its header declares (vertex {vertex})"


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_parser_does_not_read_past_its_text(chunk):
    """The text is a slice of a larger device buffer that goes on with digits; the last line has no newline."""
    raw = ply(["x", "y", "z"], "1 2 3\n4 5 67", 2)
    xyz, status = device_parse(raw, chunk, tail=b"89012 5 5\n6 6 6\n" * 8)
    assert status == [0, 0, -1, -1] and np.array_equal(xyz, [[1, 2, 3], [4, 5, 67]])
    xyz, status = device_parse(ply(["x", "y", "z"], "1 2 3\n4 5 6\n", 3), chunk, tail=b"7 8 9\n" * 8)
    assert status[0] == 1 and status[2] == 2          # the third line is not in the text, whatever follows it


# ---- format --------------------------------------------------------------------------------------------------------------
def body_of(raw):
    return raw[ply_io.parse_header(raw).body:]


@pytest.mark.parametrize("n", SIZES)
def test_format_equals_write_ply_ascii_and_keeps_its_guard_bytes(cloud_file, n):
    _, raw = cloud_file(n)
    buf, nbytes = ops.ply_format_xyz(torch.from_numpy(cloud(n).astype(np.int32)).to(DEV), guard=64)
    buf = buf.cpu().numpy()
    assert nbytes == len(body_of(raw)) and buf.size == nbytes + 64
    assert buf[:nbytes].tobytes() == body_of(raw)
    assert np.all(buf[nbytes:] == 0xAA)


def test_format_negative_values_and_int32_min(tmp_path):
    lo = -2 ** 31
    pts = np.array([[lo, lo, lo], [-1, 0, 1], [-9, -10, -99], [-100, -999, -1000], [2 ** 31 - 1, lo, -1023],
                    [lo + 1, -4095, 7]] * 50 + [[0, 0, 0]], np.int64)
    path = str(tmp_path / "want.ply")
    recon.write_ply_ascii(path, pts)
    want = open(path, "rb").read()
    buf, nbytes = ops.ply_format_xyz(torch.from_numpy(pts.astype(np.int32)).to(DEV), guard=64)
    buf = buf.cpu().numpy()
    assert buf[:nbytes].tobytes() == body_of(want) and np.all(buf[nbytes:] == 0xAA)
    ply_io.write_ply(str(tmp_path / "got.ply"), pts, device=DEV)
    assert open(tmp_path / "got.ply", "rb").read() == want


def test_write_ply_on_the_device_gives_the_host_file(tmp_path):
    for n in (0, 1, 257):
        pts = cloud(n) if n else np.zeros((0, 3), np.int64)
        a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        recon.write_ply_ascii(a, pts)
        for given in (pts, pts.astype(np.float64), torch.from_numpy(pts.astype(np.int32)).to(DEV)):
            ply_io.write_ply(b, given, fmt="ascii", device=DEV)
            assert open(a, "rb").read() == open(b, "rb").read()


def test_round_trip_of_100_000_points(tmp_path):
    pts = np.random.default_rng(5).integers(0, 4096, size=(100_000, 3)).astype(np.int32)
    path = str(tmp_path / "rt.ply")
    ply_io.write_ply(path, torch.from_numpy(pts).to(DEV), device=DEV)
    xyz, _ = ply_io.read_ply(path, device=DEV, fallback=False)
    assert xyz.dtype == torch.int32 and np.array_equal(xyz.cpu().numpy(), pts)


# ---- through preprocess_device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [10, 12])
def test_preprocess_device_of_a_binary_file_equals_the_ascii_route(tmp_path, bits):
    rng = np.random.default_rng(bits)
    centre = rng.integers(100, (1 << bits) - 100, size=(6, 3))
    pts = np.clip(centre[rng.integers(0, 6, 400)] + rng.integers(-20, 21, size=(400, 3)), 0, (1 << bits) - 1)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    recon.write_ply_ascii(a, pts)
    ply_io.write_ply(b, pts, fmt="binary")
    want = preprocess.preprocess_device(preprocess.read_ply_xyz(a), DEV, bits=bits)
    got = preprocess.preprocess_device(ply_io.read_ply(b, device=DEV)[0], DEV, bits=bits)
    for name in ("origins", "gt", "dist"):
        assert torch.equal(torch.as_tensor(getattr(got, name)), torch.as_tensor(getattr(want, name))), name
    assert got.n_points == want.n_points


# ---- command line --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoded(tmp_path_factory, golden_dir):
    """tests/golden/trained_S_pack.pk decoded by NVFPCC.decode, once without --ply_format and once with binary ->
    {"ascii": bytes of rc_dec.ply, "binary": path of rc_dec.ply, "want": the points}."""
    import NVFPCC
    from nvfpcc_amd import network
    from tests.test_gpu_trained import golden_points
    from tests.test_trained_golden import CFG, load_pack
    _, G = load_pack(golden_dir, "S")
    ch, channels = CFG["S"]
    out, old = {"want": golden_points(G, 0.6)}, os.getcwd()
    noise = network.NoiseState
    state = (network.SEED2, network.seed_ptr, noise.seed, noise.step, noise.latent_step)     # decode() rewinds these
    for fmt in ("ascii", "binary"):
        cwd = str(tmp_path_factory.mktemp(fmt))
        shutil.copy(os.path.join(golden_dir, "trained_S_pack.pk"), os.path.join(cwd, "pack.pk"))
        argv = ["decode", "pack.pk", "--batchsize", "1", "--thh", "0.6", "--N", str(G["latents"].shape[0]), "--chanstr",
                ",".join(map(str, channels)), "--ch", str(ch)] + (["--ply_format", "binary"] if fmt == "binary" else [])
        os.chdir(cwd)
        try:
            NVFPCC.decode(NVFPCC.build_parser().parse_args(argv))
        finally:
            os.chdir(old)
        path = os.path.join(cwd, "rc_dec.ply")
        out[fmt] = open(path, "rb").read() if fmt == "ascii" else path
    network.SEED2, network.seed_ptr, noise.seed, noise.step, noise.latent_step = state
    return out


def test_the_default_rc_dec_ply_keeps_its_bytes(decoded, tmp_path):
    path = str(tmp_path / "want.ply")
    recon.write_ply_ascii(path, decoded["want"])
    assert decoded["ascii"] == open(path, "rb").read()


def test_ply_format_binary_writes_the_same_points_in_the_same_order(decoded):
    assert open(decoded["binary"], "rb").read(40).startswith(b"ply\nformat binary_little_endian 1.0\n")
    for dev in (None, DEV):
        xyz, _ = ply_io.read_ply(decoded["binary"], device=dev)
        xyz = xyz.cpu().numpy() if dev else xyz
        assert np.array_equal(xyz, decoded["want"])


def test_pc_error_reads_a_binary_ref_and_an_ascii_test(decoded, tmp_path, capsys):
    from nvfpcc_amd import pc_error
    ref = decoded["want"][::3] + np.array([0, 1, 0])
    files = {}
    for name, pts, fmt in (("ref_a", ref, "ascii"), ("ref_b", ref, "binary"), ("test_a", decoded["want"], "ascii")):
        files[name] = str(tmp_path / (name + ".ply"))
        ply_io.write_ply(files[name], pts, fmt=fmt)
    outs = []
    for r in ("ref_a", "ref_b"):
        capsys.readouterr()
        assert pc_error.main([files[r], files["test_a"]]) == 0
        outs.append([ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("infile1")])
    assert outs[0] == outs[1] and any("mseF,PSNR (p2point)" in ln for ln in outs[0])
