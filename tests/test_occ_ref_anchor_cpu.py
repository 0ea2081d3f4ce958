"""The numpy references of the two occupancy coders (tests/occ_rans_ref.py, tests/occ_hier_ref.py) held to streams
recorded once: tests/golden/occ_streams.npz, written by tools/gen_occ_streams.py.  The GPU tests compare the device to
the references, so a change to a reference that changed a stream would move the yardstick: this test holds it still."""
import os

import numpy as np

from tests import occ_hier_ref as H
from tests import occ_rans_ref as R
from tests.test_lossless_cpu import adversarial_p

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occ_streams.npz")
GROUP = 2


def anchor_input():
    """(p float32 [3, 32768], gt bool [3, 32768]): probabilities on every edge of the context function; block 0 holds
    900 seeded voxels, block 1 is empty, block 2 is full."""
    rng = np.random.default_rng(23)
    p = adversarial_p(rng, 3)
    s = rng.integers(0, 32, (900, 3))
    gt = np.zeros(p.shape, bool)
    gt[0, (s[:, 0] * 32 + s[:, 1]) * 32 + s[:, 2]] = True
    gt[2] = True
    return p, gt


def streams():
    """What the references make of anchor_input(): the arrays of the fixture, by name."""
    p, gt = anchor_input()
    out = {}
    for name, ref in (("flat", R), ("hier", H)):
        f1 = ref.table(*ref.histogram(p, gt))
        coded = ref.encode(p, gt, f1, GROUP)
        out[name + "_f1"] = np.asarray(f1, np.int64)
        out[name + "_states"] = np.stack([s for s, _ in coded]).astype(np.uint64)
        for g, (_, w) in enumerate(coded):
            out[f"{name}_words{g}"] = np.asarray(w, np.uint32)
    out["hier_symbols"] = np.asarray(H.symbols_coded(p, gt), np.int64)
    # words a decoder that stops at level 2, 1, 0 consumes, per group
    out["hier_pos"] = np.asarray([[H.decode_group(p[b:b + GROUP], out["hier_f1"], out["hier_states"][g],
                                                  out[f"hier_words{g}"], stop)[2] for stop in (2, 1, 0)]
                                  for g, b in enumerate(range(0, p.shape[0], GROUP))], np.int64)
    return out


def test_references_reproduce_the_recorded_streams():
    want = np.load(GOLDEN)
    got = streams()
    assert sorted(want.files) == sorted(got)
    for name in want.files:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    # the figures the fixture was recorded with
    assert [want[f"flat_words{g}"].size for g in range(2)] == [1217, 1536]
    assert [want[f"hier_words{g}"].size for g in range(2)] == [624, 262]
    assert int(want["hier_symbols"]) == 48368 and want["hier_pos"].tolist() == [[38, 174, 624], [6, 70, 262]]


def test_recorded_streams_decode_to_the_input():
    """The decoders of both references, on the RECORDED states and words: the occupancy of the input, at every stop
    level its max-pool, the final states 2^31 and, at level 0, every word consumed."""
    want = np.load(GOLDEN)
    p, gt = anchor_input()
    pools = H.maxpool(gt)
    for g, b in enumerate(range(0, p.shape[0], GROUP)):
        sym, x, pos = R.decode_group(p[b:b + GROUP].reshape(-1), want["flat_f1"], want["flat_states"][g], want[f"flat_words{g}"])
        assert np.array_equal(sym, gt[b:b + GROUP].reshape(-1)) and (x == R.L).all() and pos == want[f"flat_words{g}"].size
        for i, stop in enumerate((2, 1, 0)):
            occ, x, pos = H.decode_group(p[b:b + GROUP], want["hier_f1"], want["hier_states"][g], want[f"hier_words{g}"], stop)
            assert np.array_equal(occ, pools[stop][b:b + GROUP]) and pos == want["hier_pos"][g, i]
        assert (x == H.L).all()
