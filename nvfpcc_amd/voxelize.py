"""Voxelisation of a float cloud on the device, and the lattice that travels in the pack.

    Lattice(bits, origin, step)                          bits 10 | 11 | 12, origin three float64, step a float64 > 0
    fit(lo, hi, bits) -> Lattice                         isotropic, not centred
    pack(lattice) -> 34 bytes, unpack(bytes) -> Lattice  the `vox_pack` entry of pack.pk
    voxelize(points, device, bits=10, lattice=None) -> Voxelized(points, counts, lattice, n_in, sum_err2, max_err2)
    to_source(q, lattice, device, level=0) -> float64 tensor [n, 3]
    python -m nvfpcc_amd.voxelize IN.ply OUT.ply [--bits B] [--vox_step S --vox_origin X Y Z] [--ply_format ascii|binary]

The definition is the format: both sides of a pack must agree to the bit.  With inv = 1.0 / step (one
float64 division, here on the host), per axis

    forward   t = x - o;  u = t * inv;  q = floor(u + 0.5)
    inverse   x = o + q * step

every operation rounded to float64 on its own.  A point is non-finite if a coordinate is a NaN or an infinity, outside
if some u + 0.5 is below 0 or at least 2^bits.  The result is the distinct lattice points in ascending order of
key = q0 << 2 bits | q1 << bits | q2, how many input points fell on each, and the maximum and the sum over the input
points of e2 = sum over axes of (x - (o + q step))^2.

Device only, like the rest of ops: the kernels are those of csrc/voxelize.hip (torch.sort between them is plumbing, as
in preprocess_device) and there is no CPU fallback; the numpy twin is tests/voxelize_ref.py.
"""
import collections
import math
import struct

import numpy as np
import torch

BITS = (10, 11, 12)
PACK_VERSION = 1
PACK_BYTES = 34
_PACK = struct.Struct("<BB4d")

Voxelized = collections.namedtuple("Voxelized", "points counts lattice n_in sum_err2 max_err2")


class Lattice(collections.namedtuple("Lattice", "bits origin step")):
    """(bits, origin, step): lattice point q stands for origin + q * step, 0 <= q < 2^bits on every axis."""
    __slots__ = ()

    def __new__(cls, bits, origin, step):
        if isinstance(bits, bool) or bits not in BITS:
            raise ValueError(f"lattice: bits must be one of {BITS}, not {bits!r}")
        origin = tuple(float(v) for v in np.asarray(origin, np.float64).reshape(-1))
        if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
            raise ValueError(f"lattice: the origin must be three finite numbers, not {origin!r}")
        step = float(step)
        if not (math.isfinite(step) and step > 0.0 and math.isfinite(1.0 / step)):
            raise ValueError(f"lattice: the step must be finite and above 0 (and so must 1 / step), not {step!r}")
        return super().__new__(cls, int(bits), origin, step)

    @property
    def inv(self):
        """1.0 / step: the one division of the definition."""
        return 1.0 / self.step


def fit(lo, hi, bits):
    """The lattice of a cloud whose finite points span lo .. hi per axis: step = (largest extent) / (2^bits - 1), or
    1.0 when the extent is 0; origin = lo + 0.0, so that -0.0 becomes +0.0.  Isotropic, not centred."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if isinstance(bits, bool) or bits not in BITS:
        raise ValueError(f"lattice: bits must be one of {BITS}, not {bits!r}")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("fit: the cloud has no finite point")
    extent = float(np.max(hi - lo))
    step = extent / float((1 << bits) - 1) if extent > 0.0 else 1.0
    return Lattice(bits, lo + 0.0, step)


def pack(lattice):
    """vox_pack: version byte 1, bits as uint8, the origin as three little-endian float64, the step as one."""
    return _PACK.pack(PACK_VERSION, lattice.bits, *lattice.origin, lattice.step)


def unpack(data):
    """vox_pack -> Lattice; ValueError on a wrong length, a wrong version, bad bits, a step that is not finite and
    above 0 or an origin that is not finite."""
    data = bytes(data)
    if len(data) != PACK_BYTES:
        raise ValueError(f"vox_pack: {len(data)} bytes, not {PACK_BYTES}")
    version, bits, ox, oy, oz, step = _PACK.unpack(data)
    if version != PACK_VERSION:
        raise ValueError(f"vox_pack: version {version}, not {PACK_VERSION}")
    try:
        return Lattice(bits, (ox, oy, oz), step)
    except ValueError as e:
        raise ValueError(f"vox_pack: {e}") from None


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("nvfpcc_amd.voxelize runs on the HIP device only; there is no CPU fallback")
    return dev


def voxelize(points, device, bits=10, lattice=None):
    """points [P, 3] (numpy or tensor; float32 and integers are widened exactly) -> Voxelized: points int32 [M, 3] and
    counts int32 [M] on the device, the lattice, n_in = P, and sum_err2 / max_err2 as Python floats.  lattice None: the
    fit of the cloud's own bounds at `bits`; else the given one (its bits count, `bits` is not read).
    Under a given lattice the host reads one record (the status of csrc/voxelize.hip: the point classes, M, the errors)
    -- the one sync of the call; fitting reads the 64-byte bounds first, because the step and its inverse are host
    float64 arithmetic by definition.  ValueError, naming the count and the first index, for non-finite points and for
    points outside a given lattice; no output is read then."""
    from . import ops
    dev = _device(device)
    t = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points))
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype == torch.bool or t.dtype.is_complex:
        raise ValueError(f"voxelize: expected points of shape [P, 3], got {t.dtype} {tuple(t.shape)}")
    n = t.shape[0]
    if n == 0:
        raise ValueError("empty cloud")
    if n >= 1 << 30:
        raise ValueError("too many points")
    with torch.cuda.device(dev):
        xyz = t.to(dev).to(torch.float64).contiguous()
        if lattice is None:
            lo, hi, bad, first = ops.vox_bounds(xyz)
            if bad:
                raise ValueError(f"voxelize: {bad} of {n} points are not finite (the first is point {first})")
            lattice = fit(lo, hi, bits)
        elif not isinstance(lattice, Lattice):
            lattice = Lattice(*lattice)
        q, keys, status = ops.vox_quantize(xyz, lattice.bits, lattice.origin, lattice.step, lattice.inv)
        del q                                                    # the points come back out of the sorted keys
        skeys = torch.sort(keys).values                          # plumbing: equal keys are equal points
        pts, counts = ops.vox_unique(skeys, lattice.bits, status)
        st = ops.vox_status(status)                              # the one host sync under a given lattice
    if st["nonfinite"]:
        raise ValueError(f"voxelize: {st['nonfinite']} of {n} points are not finite (the first is point "
                         f"{st['first_nonfinite']})")
    if st["outside"]:
        raise ValueError(f"voxelize: {st['outside']} of {n} points lie outside the lattice of {lattice.bits} bits, step "
                         f"{lattice.step!r}, origin {lattice.origin!r} (the first is point {st['first_outside']})")
    m = st["voxels"]
    return Voxelized(pts[:m], counts[:m], lattice, n, st["sum_err2"], st["max_err2"])


def to_source(q, lattice, device, level=0):
    """Lattice points q [n, 3] (integers, numpy or tensor) -> origin + q * (step * 2^level) as a float64 tensor [n, 3]
    on the device.  level: q lies on the lattice of a coarser level of detail, whose step is 2^level times the pack's and
    whose origin is the same."""
    from . import ops
    dev = _device(device)
    t = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype == torch.bool or t.dtype.is_complex:
        raise ValueError(f"to_source: expected lattice points of shape [n, 3], got {t.dtype} {tuple(t.shape)}")
    if t.dtype.is_floating_point and not bool((t == torch.round(t)).all()):
        raise ValueError("to_source: lattice points must be integers")
    with torch.cuda.device(dev):
        return ops.vox_dequantize(t.to(dev).to(torch.int32).contiguous(), lattice.origin, lattice.step * 2.0 ** int(level))


def voxelize_line(v):
    """The [Voxelize] line of a Voxelized.  step and origin print as Python reprs: typed back, they give the same
    float64."""
    rms, s = math.sqrt(v.sum_err2 / v.n_in), v.lattice.step
    return "[Voxelize] points: %d voxels: %d bits: %d step: %r origin: %r %r %r rms err: %.6g (%.4f steps) max err: %.6g" % (
        v.n_in, v.points.shape[0], v.lattice.bits, s, *v.lattice.origin, rms, rms / s, math.sqrt(v.max_err2))


def lattice_from_args(args, what):
    """--bits / --vox_step / --vox_origin of a parsed command line after the checks that need no device -> the Lattice,
    or None when the cloud's own fit is asked for.  Each refusal is a SystemExit with its own message."""
    bits = getattr(args, "bits", 10)
    if not hasattr(args, "vox_step"):
        if hasattr(args, "vox_origin"):
            raise SystemExit(f"{what}: --vox_origin places the lattice of --vox_step; give --vox_step too")
        return None
    if not (math.isfinite(args.vox_step) and args.vox_step > 0.0):
        raise SystemExit(f"{what}: --vox_step {args.vox_step!r} is not a finite step above 0")
    try:
        return Lattice(bits, getattr(args, "vox_origin", (0.0, 0.0, 0.0)), args.vox_step)
    except ValueError as e:
        raise SystemExit(f"{what}: {e}")


def add_lattice_arguments(p):
    """--vox_step and --vox_origin, absent from the namespace unless given."""
    import argparse
    import re
    # an origin printed by the [Voxelize] line may read -1.2e-05; argparse before 3.14 takes that for an option
    if hasattr(p, "_negative_number_matcher"):
        p._negative_number_matcher = re.compile(r"^-(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")
    p.add_argument("--vox_step", type=float, metavar="S", default=argparse.SUPPRESS,
                   help="--voxelize: the lattice step in the units of the input; with --vox_origin it fixes the lattice.  "
                        "Absent: the lattice is fitted to the cloud (largest extent / (2^bits - 1), origin at its minimum).")
    p.add_argument("--vox_origin", type=float, nargs=3, metavar=("X", "Y", "Z"), default=argparse.SUPPRESS,
                   help="--voxelize --vox_step: the point of the input's frame that lattice point 0 0 0 stands for "
                        "(0 0 0 when absent).")


def main(argv=None):
    import argparse
    from . import ply_io
    p = argparse.ArgumentParser(prog="python -m nvfpcc_amd.voxelize", description="Voxelise a PLY with float coordinates "
                                "on the device; writes the distinct lattice points as an integer PLY.")
    p.add_argument("input")
    p.add_argument("output")
    p.add_argument("--bits", type=int, choices=list(BITS), default=argparse.SUPPRESS, help="bits per axis (10 when absent)")
    add_lattice_arguments(p)
    p.add_argument("--ply_format", choices=["ascii", "binary"], default="ascii")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    lattice = lattice_from_args(args, "voxelize")
    if not torch.cuda.is_available():
        raise SystemExit("voxelize needs a HIP device: there is no CPU fallback")
    dev = torch.device(args.device)
    try:
        v = voxelize(ply_io.read_ply(args.input, coords="float")[0], dev, bits=getattr(args, "bits", 10), lattice=lattice)
    except (OSError, ValueError) as e:
        raise SystemExit(f"voxelize {args.input}: {e}")
    print(voxelize_line(v))
    ply_io.write_ply(args.output, v.points, fmt=args.ply_format, device=dev)


if __name__ == "__main__":
    main()
