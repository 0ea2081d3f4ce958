"""Geometry PSNR of a test cloud against a reference, printed the way MPEG's pc_error prints it.

    python -m nvfpcc_amd.pc_error REF.ply TEST.ply [--bits 10] [--index dense|sparse] [--peak 1023] [--knn 12] [--no-d2]

REF.ply is the original (A), TEST.ply the decoded cloud (B); each an ASCII or a binary PLY (nvfpcc_amd.ply_io) with
integer coordinates in [0, 2^bits), bits = 10, 11 or 12.  --peak defaults to 2^bits - 1; --index to the dense cell grid
at 10 bits and the sparse one above.
The normals of A come from REF.ply's nx ny nz when it has them, otherwise from a k-NN PCA (nvfpcc_amd.pc_metrics).
The exit status is 1 on bad input.
"""
import argparse
import sys


def _lines(r, d2):
    out = []
    for i, (head, key) in enumerate((("1. Use infile1 (A) as reference, loop over A, use normals on B. (A->B).",
                                      "ref_to_test"),
                                     ("2. Use infile2 (B) as reference, loop over B, use normals on A. (B->A).",
                                      "test_to_ref"),
                                     ("3. Final (symmetric).", None)), 1):
        v = r if key is None else r[key]
        tag = "F" if key is None else str(i)
        out.append(head)
        out.append(f"   mse{tag}      (p2point): {v['d1_mse']:.6g}")
        out.append(f"   mse{tag},PSNR (p2point): {v['d1_psnr']:.6g}")
        if d2:
            out.append(f"   mse{tag}      (p2plane): {v['d2_mse']:.6g}")
            out.append(f"   mse{tag},PSNR (p2plane): {v['d2_psnr']:.6g}")
        out.append(f"   h.       {tag}(p2point): {v['hausdorff_d2']}")
    return out


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("ref", help="reference cloud (A), ASCII or binary PLY")
    p.add_argument("test", help="test (decoded) cloud (B), ASCII or binary PLY")
    p.add_argument("--bits", type=int, choices=(10, 11, 12), default=10,
                   help="bits per axis: coordinates lie in [0, 2^bits)")
    p.add_argument("--index", choices=("dense", "sparse"), default=None,
                   help="cell index of the search (default: dense at 10 bits, sparse above; dense is 10-bit only)")
    p.add_argument("--peak", type=float, default=None, help="peak value of the PSNR (default: 2^bits - 1)")
    p.add_argument("--knn", type=int, default=12, help="neighbours of the PCA normal estimate (3..32)")
    p.add_argument("--no-d2", action="store_true", help="point-to-point only")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.peak is None:
        args.peak = (1 << args.bits) - 1
    import torch
    from nvfpcc_amd.pc_metrics import geometry_psnr
    from nvfpcc_amd.ply_io import read_ply
    dev = "cuda" if torch.cuda.is_available() else None     # the device geometry_psnr runs on; without one it says so
    try:
        a, na = read_ply(args.ref, device=dev, normals=True)
        b, _ = read_ply(args.test, device=dev)
        r = geometry_psnr(a, b, peak=args.peak, ref_normals=na, knn=args.knn, d2=not args.no_d2, bits=args.bits,
                          index=args.index)
    except (OSError, ValueError) as e:
        print(f"pc_error: {e}", file=sys.stderr)
        return 1
    print(f"infile1 (A): {args.ref} ({r['n_ref']} points)")
    print(f"infile2 (B): {args.test} ({r['n_test']} points)")
    print(f"peak: {args.peak:g}  normals of A: {'from infile1' if na is not None else f'PCA, knn = {args.knn}'}")
    print("\n".join(_lines(r, not args.no_d2)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
