"""PLY files in and out: ASCII bodies parsed and formatted on the device, binary PLY on the host.

    read_ply(path, device=None, normals=False, fallback=True, coords="int" | "float") -> (xyz, normals or None)
    write_ply(path, points, fmt="ascii" | "binary", device=None)
    write_ply_float(path, xyz, fmt="ascii" | "binary")
    parse_header(raw, path) -> Header

Formats: ascii, binary_little_endian, binary_big_endian; x, y, z are found by property name in the `vertex` element and
need not come first or in that order; elements before and after `vertex` are skipped (before it, in a binary file, they
must not hold list properties: their size is unknown without walking them).  Coordinates are integers, unless
read_ply is asked for coords="float": then they come back as float64 on the host, whatever they are (NaN and infinities
included: nvfpcc_amd.voxelize refuses them), and write_ply_float writes such a cloud; both on the host.

With a HIP device the body of an ASCII file goes up as bytes and the kernels of csrc/ply_io.hip (ops.ply_parse_xyz) turn
it into an int32 tensor [n, 3] there; write_ply formats an int32 tensor into the text of the file there
(ops.ply_format_xyz) and fetches it in one copy.  The device parser is a fast path with a narrow grammar: a coordinate
token is [+-]?[0-9]{1,10}(\\.0*)? with a magnitude of at most 2^31 - 1, tokens of other columns are skipped without a look.
On every file the host reader (pc_metrics.read_ply_points) accepts, it returns the host reader's coordinates or hands
the file to the host reader: a coordinate token outside the grammar (1.5, 1e2, nan, eleven digits), a control byte
other than tab / LF / CR-before-LF and a byte >= 0x7f anywhere in a vertex line all do the latter, and the host reader
then accepts or refuses the file as it always did.  The one difference: the host reader converts every column to a
float and so refuses a file with a non-numeric token in a column nobody asked for; the device parser does not read it.

Without a device everything runs on the host: pc_metrics.read_ply_points for ASCII, numpy for binary, and
recon.write_ply_ascii (looked up on the module at call time) for ASCII output.  The bytes of an ASCII file are the same
on both routes.
"""
import io
import re
import warnings
from collections import namedtuple

import numpy as np
import torch

Property = namedtuple("Property", "type name is_list")      # type: int8 .. float64 (of the items, for a list)
Element = namedtuple("Element", "name count props")
Header = namedtuple("Header", "format elements body")       # body: byte offset of the first byte after the header

FORMATS = ("ascii", "binary_little_endian", "binary_big_endian")
TYPES = {"char": "int8", "uchar": "uint8", "short": "int16", "ushort": "uint16", "int": "int32", "uint": "uint32",
         "float": "float32", "double": "float64"}
TYPES.update({v: v for v in list(TYPES.values())})
_NP = {"int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "float32": "f4",
       "float64": "f8"}
_END = re.compile(rb"\nend_header[ \t]*\r?(\n|$)")
_HEAD_BYTES = 1 << 16       # where a header is looked for first; the whole file when it does not end there


def _type(word, path):
    if word not in TYPES:
        raise ValueError(f"{path}: unknown PLY property type '{word}'")
    return TYPES[word]


def parse_header(raw, path="<bytes>"):
    """The header of a PLY file from its first bytes (everything up to and including the end_header line must be in
    `raw`) -> Header(format, elements, body).  ValueError names the file and the fault."""
    raw = bytes(raw)
    if not re.match(rb"ply[ \t]*\r?\n", raw):
        raise ValueError(f"{path}: not a PLY file (no 'ply' magic)")
    m = _END.search(raw)
    if m is None:
        raise ValueError(f"{path}: PLY header has no end_header")
    fmt, elements = None, []
    for line in raw[:m.start()].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format" and len(w) >= 2:
            fmt = w[1]
        elif w[0] == "element" and len(w) == 3 and w[2].isdigit():
            elements.append(Element(w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) == 5 and w[1] == "list":
            _type(w[2], path)
            elements[-1].props.append(Property(_type(w[3], path), w[4], True))
        elif w[0] == "property" and elements and len(w) == 3:
            elements[-1].props.append(Property(_type(w[1], path), w[2], False))
        else:
            raise ValueError(f"{path}: PLY header line not understood: '{line.strip()}'")
    if fmt not in FORMATS:
        raise ValueError(f"{path}: PLY format must be one of {', '.join(FORMATS)}, not {fmt}")
    names = [e.name for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: PLY has no vertex element")
    vi = names.index("vertex")
    vprops = [p.name for p in elements[vi].props]
    for axis in ("x", "y", "z"):
        if axis not in vprops:
            raise ValueError(f"{path}: vertex element has no '{axis}' property")
    if any(p.is_list for p in elements[vi].props):
        raise ValueError(f"{path}: the vertex element has a list property")
    if fmt != "ascii":
        for e in elements[:vi]:
            if any(p.is_list for p in e.props):
                raise ValueError(f"{path}: binary PLY with a list property in element '{e.name}' before the vertices: "
                                 f"its size is unknown without walking it")
    return Header(fmt, elements, m.end())


def _vertex(header):
    """-> (index of the vertex element, the element, column of each property name)."""
    vi = [e.name for e in header.elements].index("vertex")
    v = header.elements[vi]
    return vi, v, {p.name: i for i, p in enumerate(v.props)}


def _record(element, order):
    return np.dtype([(f"p{i}", order + _NP[p.type]) for i, p in enumerate(element.props)])


def _read_binary(arr, header, path, normals, coords="int"):
    """xyz int64 [n, 3] (float64, as stored, with coords="float"; and nx ny nz float64 [n, 3], when asked for and present)
    of a binary PLY held in `arr`."""
    order = "<" if header.format == "binary_little_endian" else ">"
    vi, v, col = _vertex(header)
    offset = header.body + sum(e.count * _record(e, order).itemsize for e in header.elements[:vi])
    rec = _record(v, order)
    want, have = v.count * rec.itemsize, max(0, arr.size - offset)
    if have < want:
        raise ValueError(f"{path}: binary PLY declares {want} bytes of vertex data, {have} follow "
                         f"(an ASCII body under a binary header?)")
    rows = np.frombuffer(arr, dtype=rec, count=v.count, offset=offset)
    xyz = np.stack([rows[f"p{col[a]}"].astype(np.float64) for a in ("x", "y", "z")], 1) if v.count else \
        np.zeros((0, 3), np.float64)
    if coords == "int" and (not np.all(np.isfinite(xyz)) or np.any(xyz != np.round(xyz))):
        raise ValueError(f"{path}: coordinates must be integers")
    nrm = None
    if normals and all(a in col for a in ("nx", "ny", "nz")):
        nrm = np.stack([rows[f"p{col[a]}"].astype(np.float64) for a in ("nx", "ny", "nz")], 1).reshape(-1, 3)
    return (xyz.reshape(-1, 3) if coords == "float" else xyz.astype(np.int64)), nrm


def _gpu(device):
    """-> torch.device of a HIP device, or None for the host (device None or a CPU device)."""
    if device is None:
        return None
    dev = torch.device(device)
    if dev.type == "cpu":
        return None
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"nvfpcc_amd.ply_io: {dev} is no HIP device (pass device=None for the host route)")
    return dev


def _on_device(xyz, dev):
    """Host int64 coordinates as a tensor on dev: int32, or int64 when a value does not fit (nothing downstream takes
    such a cloud, and its own range check says why)."""
    fits = xyz.size == 0 or (xyz.min() >= -2 ** 31 and xyz.max() < 2 ** 31)
    return torch.from_numpy(xyz.astype(np.int32) if fits else xyz).to(dev)


def _ascii_normals(arr, header, path, names=("nx", "ny", "nz")):
    """nx ny nz (or the columns `names`) float64 [n, 3] of an ASCII body by np.loadtxt, for a file whose vertex lines
    the device parser has already found complete (so no vertex line is blank, and loadtxt's rows are the vertex lines)."""
    vi, v, col = _vertex(header)
    body = arr[header.body:].tobytes()
    pos = 0
    for _ in range(sum(e.count for e in header.elements[:vi])):
        pos = body.find(b"\n", pos) + 1
    return np.loadtxt(io.BytesIO(body[pos:]), dtype=np.float64, comments=None, max_rows=v.count,
                      usecols=tuple(col[a] for a in names), ndmin=2).reshape(-1, 3)


def _read_float(arr, header, path, normals):
    """coords="float": (xyz float64 [n, 3], normals or None) on the host.  Binary files through the record path; ASCII
    bodies through np.loadtxt on the x, y, z columns by name (it skips blank lines, as the host reader of the integer
    route does)."""
    if header.format != "ascii":
        return _read_binary(arr, header, path, normals, coords="float")
    vi, v, col = _vertex(header)
    if v.count == 0:
        return np.zeros((0, 3), np.float64), None
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)        # loadtxt announces every blank line it skips
            xyz = _ascii_normals(arr, header, path, ("x", "y", "z"))
            nrm = _ascii_normals(arr, header, path) if normals and all(a in col for a in ("nx", "ny", "nz")) else None
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    if xyz.shape[0] != v.count:
        raise ValueError(f"{path}: PLY holds fewer vertex values than its header declares ({xyz.shape[0]} of {v.count})")
    return xyz, nrm


def read_ply(path, device=None, normals=False, fallback=True, coords="int"):
    """(xyz, normals or None) of an ASCII or binary PLY.  With a HIP `device`, xyz is an int32 tensor [n, 3] on it (int64
    in the one case of _on_device); without, int64 numpy.  normals=True: float64 numpy [n, 3] when the file has nx ny nz.
    fallback=False: an ASCII file outside the device parser's grammar raises ValueError instead of going to the host
    reader.  coords="float": the coordinates as the file holds them, widened to float64 numpy [n, 3] on the host
    (`device` and `fallback` are not read; NaN and infinities pass through)."""
    if coords not in ("int", "float"):
        raise ValueError(f"coords must be 'int' or 'float', got {coords!r}")
    dev = _gpu(device)
    arr = np.fromfile(path, dtype=np.uint8)
    try:
        header = parse_header(arr[:_HEAD_BYTES].tobytes(), path)
    except ValueError:
        if arr.size <= _HEAD_BYTES:
            raise
        header = parse_header(arr.tobytes(), path)
    if coords == "float":
        return _read_float(arr, header, path, normals)
    if header.format != "ascii":
        xyz, nrm = _read_binary(arr, header, path, normals)
        return (xyz if dev is None else _on_device(xyz, dev)), nrm
    from .pc_metrics import read_ply_points
    if dev is None:
        xyz, nrm = read_ply_points(path)
        return xyz, (nrm if normals else None)
    from . import ops
    vi, v, col = _vertex(header)
    first_line = sum(e.count for e in header.elements[:vi])
    with torch.cuda.device(dev):
        text = torch.from_numpy(arr).to(dev)[header.body:]
        xyz, status = ops.ply_parse_xyz(text, first_line, v.count, len(v.props), (col["x"], col["y"], col["z"]))
        short, foreign, first_short, first_foreign = status.cpu().tolist()
    if foreign:
        if not fallback:
            raise ValueError(f"{path}: vertex {first_foreign} (body line {first_line + first_foreign}) is outside the "
                             f"device parser's grammar")
        xyz, nrm = read_ply_points(path)
        return _on_device(xyz, dev), (nrm if normals else None)
    if short:
        raise ValueError(f"{path}: PLY holds fewer vertex values than its header declares (vertex {first_short})")
    nrm = None
    if normals and v.count and all(a in col for a in ("nx", "ny", "nz")):
        nrm = _ascii_normals(arr, header, path)
    return xyz, nrm


def _header_bytes(n, fmt):
    form, kind = ("ascii", "double") if fmt == "ascii" else ("binary_little_endian", "float")
    return (f"ply\nformat {form} 1.0\ncomment Created by nvfpcc_amd\nelement vertex {n}\n"
            f"property {kind} x\nproperty {kind} y\nproperty {kind} z\nend_header\n").encode("ascii")


def write_ply(path, points, fmt="ascii", device=None):
    """Writes integer points [n, 3] (numpy or tensor, host or device; integral floats are taken) as a PLY.
    fmt="ascii": the very bytes recon.write_ply_ascii writes (double x y z, "%d %d %d" per point); with a HIP `device`
    the text is formatted there.  fmt="binary": binary_little_endian, float x y z; coordinates of 2^24 and more in
    magnitude have no exact float32 and raise ValueError."""
    if fmt not in ("ascii", "binary"):
        raise ValueError(f"fmt must be 'ascii' or 'binary', got {fmt!r}")
    dev = _gpu(device)
    if isinstance(points, torch.Tensor):
        t = points.detach()
    else:
        a = np.ascontiguousarray(points)
        t = torch.from_numpy(a if a.flags.writeable else a.copy())      # (torch takes no read-only array)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype == torch.bool or t.dtype.is_complex:
        raise ValueError(f"write_ply: expected integer points of shape [n, 3], got {t.dtype} {tuple(t.shape)}")
    n = t.shape[0]
    minus_zero = False
    if t.dtype.is_floating_point and n:
        if not bool((torch.isfinite(t) & (t == torch.round(t))).all()):
            raise ValueError("write_ply: coordinates must be integers")
        minus_zero = bool(((t == 0) & torch.signbit(t)).any())      # the host writer prints it as "-0"
    lo, hi = (int(v) for v in torch.stack([t.amin(), t.amax()]).tolist()) if n else (0, 0)
    if fmt == "binary":
        if max(-lo, hi) >= 1 << 24:
            raise ValueError(f"write_ply: binary PLY holds float32 coordinates, exact below 2^24 only (got {lo} .. {hi})")
        with open(path, "wb") as f:
            f.write(_header_bytes(n, fmt))
            f.write(t.cpu().numpy().astype("<f4").tobytes())
        return
    if dev is None or minus_zero or lo < -2 ** 31 or hi >= 2 ** 31:
        from . import recon
        recon.write_ply_ascii(path, points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points)
        return
    from . import ops
    head = _header_bytes(n, fmt)
    with torch.cuda.device(dev):
        text = ops.ply_format_xyz(t.to(torch.int32).to(dev).contiguous())      # 12 bytes per point go up
        out = np.empty(len(head) + text.numel(), np.uint8)
        out[:len(head)] = np.frombuffer(head, np.uint8)
        if text.numel():
            torch.from_numpy(out[len(head):]).copy_(text)       # one device-to-host copy, into the file's buffer
    with open(path, "wb") as f:
        f.write(memoryview(out))                                # one write


def write_ply_float(path, xyz, fmt="ascii"):
    """Writes points [n, 3] (numpy or tensor) with float64 coordinates as a PLY, on the host.  fmt="binary":
    binary_little_endian, double x y z; fmt="ascii": "%.17g" per coordinate, which reads back to the same float64.
    read_ply(path, coords="float") returns the very bits, -0.0, NaN and infinities included."""
    if fmt not in ("ascii", "binary"):
        raise ValueError(f"fmt must be 'ascii' or 'binary', got {fmt!r}")
    a = xyz.detach().cpu().numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "fiu":
        raise ValueError(f"write_ply_float: expected points of shape [n, 3], got {a.dtype} {a.shape}")
    a = np.ascontiguousarray(a, np.float64)
    form = "ascii" if fmt == "ascii" else "binary_little_endian"
    head = (f"ply\nformat {form} 1.0\ncomment Created by nvfpcc_amd\nelement vertex {a.shape[0]}\n"
            f"property double x\nproperty double y\nproperty double z\nend_header\n").encode("ascii")
    with open(path, "wb") as f:
        f.write(head)
        if fmt == "binary":
            f.write(a.astype("<f8").tobytes())
        else:
            f.write("".join("%.17g %.17g %.17g\n" % tuple(r) for r in a.tolist()).encode("ascii"))
