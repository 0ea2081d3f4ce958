#!/usr/bin/env python3
"""Generate tests/golden/occ_streams.npz: what the numpy references of the two occupancy coders (tests/occ_rans_ref.py,
tests/occ_hier_ref.py) make of one seeded input -- tables, final states, every group's words and, for the scalable coder,
the words a decoder consumes at each stop level.  tests/test_occ_ref_anchor_cpu.py holds the references to this file, so
run it on the commit whose references are the yardstick, BEFORE changing them, never to make a failing test pass.

This file pins the numpy coders to inputs they generate themselves; it does not pin the FIELD they code under.  That is
tests/golden/conformance_{S,W}.npz (tools/make_conformance_fixture.py): the float32 bits of the eval forward on the two
committed trained decoders, and the side packs encoded under them.

    python tools/gen_occ_streams.py       # rewrites tests/golden/occ_streams.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_occ_ref_anchor_cpu import GOLDEN, streams          # noqa: E402

if __name__ == "__main__":
    out = streams()
    np.savez_compressed(GOLDEN, **out)
    for name in sorted(out):
        print(name, out[name].dtype, out[name].shape)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
