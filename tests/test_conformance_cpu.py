"""The committed side packs of tests/golden/conformance_{S,W}.npz against references that use no kernel of this project
(tools/make_conformance_fixture.py wrote the file on an MI355X; DESIGN.md, "What the side packs fix").  Host only: numpy,
the packs' own readers and the numpy coders of tests/occ_*_ref.py.  tests/test_gpu_conformance.py holds the device to
the same file.

  1. the `lossless_pack` bytes, decoded by tests/occ_rans_ref.py under the committed voxel contexts `ctx0` and the table
     the pack carries, are EXACTLY synth.make_blocks(12): the contexts and the stream are tied to each other and to a
     ground truth that numpy makes, not to a recording;
  2. the scalable packs too, both versions, at levels 0, 1 and 2.  Their contexts are functions of the pooled field and of
     child counts, and BOTH follow from `ctx0` alone (tests/conformance_ref.py, module docstring: the context of a
     maximum is the highest-ranked context of the children): all three levels of version 1 and of version 3 are decoded
     here, nothing of it is left to the GPU half, and no second context array is committed;
  3. every committed byte string passes its own reader, with version bytes 1 / 1 / 3 / 1;
  4. the detector is live: one mantissa bit of one sampled p changes its block's digest, and one voxel of ctx0 moved to
     the neighbouring context makes the decode of item 1 miss the ground truth or raise.

Every comparison is equality.  No number in this file is a tolerance."""
import numpy as np
import pytest

from nvfpcc_amd import lod_pack, lossless_lod_pack, lossless_nbr_pack, lossless_pack, thh_select
from tests import conformance_ref as C
from tests import occ_hier_ref as H
from tests import occ_nbr_ref as NB
from tests import occ_rans_ref as R

_CACHE = {}


def fixture(golden_dir, tag):
    if tag not in _CACHE:
        _CACHE[tag] = C.load(golden_dir, tag)
    return _CACHE[tag]


@pytest.fixture(scope="module")
def gt():
    return C.ground_truth()


def groups(side):
    """(first block, block past the last, states, words) of every group of a read pack."""
    off = np.concatenate([[0], np.cumsum(side["nwords"])])
    for g in range(len(side["nwords"])):
        lo = g * side["group"]
        yield lo, min(lo + side["group"], side["n_blocks"]), side["states"][g], side["words"][off[g]:off[g + 1]]


def decode_v1(data, ctx0):
    """lossless_pack bytes under voxel contexts uint8 [12, 32768] -> bool [12, 32768].  ValueError / IndexError on a
    stream that does not end where its frame says."""
    side = lossless_pack.read(bytes(data), C.N_BLOCKS)
    out = np.zeros((C.N_BLOCKS, C.VOX), bool)
    for lo, hi, states, words in groups(side):
        one = side["f1"][ctx0[lo:hi].reshape(-1).astype(np.int64)].astype(np.uint64)
        sym, x, pos = R.decode_steps(states.copy(), words, 0, R.padded(one))
        if pos != words.size or (x != R.L).any():
            raise ValueError("words left over or a final state that is not 2^31")
        out[lo:hi] = sym.reshape(-1)[:one.size].reshape(hi - lo, C.VOX)
    return out


@pytest.mark.parametrize("tag", C.TAGS)
def test_fixture_is_whole_and_small(tag, golden_dir):
    import os
    F = fixture(golden_dir, tag)
    assert os.path.getsize(C.fixture_path(golden_dir, tag)) < C.SIZE_CAP
    assert len(str(F["parent"])) == 40 and int(str(F["parent"]), 16) >= 0
    assert F["ctx0_blocks"].tolist() == list(range(C.N_BLOCKS)), "item 1 and 2 of this file need every block's contexts"
    assert F["ctx0"].shape == (C.N_BLOCKS, C.VOX) and F["ctx0"].dtype == np.uint8
    assert F["p_sha"].shape == F["cls1_sha"].shape == F["cls0_sha"].shape == (C.N_BLOCKS, 32)
    assert np.array_equal(F["p_sample_index"], np.arange(0, C.VOX, C.SAMPLE_STRIDE))
    # the sampled bit patterns are probabilities, and their contexts are the committed ones
    p = F["p_sample_bits"].view(np.float32)
    assert not R.bad(p).any()
    assert np.array_equal(R.contexts(p), F["ctx0"][:, F["p_sample_index"]])
    # the two trained decoders are not each other's copy
    assert tag == "S" or not np.array_equal(F["p_sha"], fixture(golden_dir, "S")["p_sha"])


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("tag", C.TAGS)
def test_lossless_pack_decodes_to_the_numpy_ground_truth_under_the_committed_contexts(tag, group, golden_dir, gt):
    F = fixture(golden_dir, tag)
    assert np.array_equal(decode_v1(F[f"lossless_g{group}"], F["ctx0"]), gt)


@pytest.mark.parametrize("tag", C.TAGS)
def test_the_pack_carries_the_table_of_the_committed_contexts(tag, golden_dir, gt):
    """f1 is lossless_pack's rule over (ctx0, gt), at both group sizes: the histogram half of the encoder."""
    F = fixture(golden_dir, tag)
    c = F["ctx0"].reshape(-1).astype(np.int64)
    want = R.table(np.bincount(c, minlength=256), np.bincount(c[gt.reshape(-1)], minlength=256))
    for group in C.GROUPS:
        assert np.array_equal(lossless_pack.read(bytes(F[f"lossless_g{group}"]))["f1"], want)


def test_the_surrogate_field_has_the_contexts_it_is_built_from():
    """What item 2 rests on: every context a probability can have owns a float32 of exactly that context, and they rise
    strictly with the rank; the pyramid of a field and of its surrogate have the same contexts and child counts."""
    ok = np.flatnonzero(~np.isnan(C.REPRESENTATIVE))
    assert np.array_equal(R.contexts(C.REPRESENTATIVE[ok]), ok)
    assert (np.diff(C.REPRESENTATIVE[ok][np.argsort(C.rank(ok))]) > 0).all()
    assert ((C.REPRESENTATIVE[ok] > np.float32(0.5)) == (ok & 1).astype(bool)).all()
    x = np.random.default_rng(5).normal(size=(2, C.VOX)) * 14
    p = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    p[0, :64] = [0.0, 1.0, 0.5, np.float32(0.5) + np.float32(2.0 ** -24)] * 16
    assert np.array_equal(R.contexts(C.surrogate_p(R.contexts(p))), R.contexts(p))
    a, b = H.pyramid(p), H.pyramid(C.surrogate_p(R.contexts(p)))
    assert np.array_equal(R.contexts(a[0]), R.contexts(b[0])) and np.array_equal(R.contexts(a[2]), R.contexts(b[2]))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("name,ref", [("lossless_lod", H), ("lossless_nbr", NB)])
@pytest.mark.parametrize("tag", C.TAGS)
def test_scalable_packs_decode_to_the_ground_truth_and_its_max_pools(tag, name, ref, group, golden_dir, gt):
    F = fixture(golden_dir, tag)
    data = bytes(F[f"{name}_g{group}"])
    side = lossless_nbr_pack.module_of(data).read(data, C.N_BLOCKS)
    p = C.surrogate_p(F["ctx0"])
    assert np.array_equal(R.contexts(p), F["ctx0"])
    want = C.unpack_levels(gt)
    for lo, hi, states, words in groups(side):
        used = []
        for stop in (2, 1, 0):
            occ, x, pos = ref.decode_group(p[lo:hi], side["f1"], states, words, stop)
            assert np.array_equal(occ, want[stop][lo:hi]), f"{tag} {name} group of {group} from block {lo}, level {stop}"
            used.append(pos)
        assert used[0] <= used[1] <= used[2] == words.size and (x == H.L).all()


@pytest.mark.parametrize("tag", C.TAGS)
def test_every_committed_byte_string_passes_its_own_reader(tag, golden_dir, gt):
    from tests.test_trained_golden import CFG
    F = fixture(golden_dir, tag)
    for group in C.GROUPS:
        for name, mod in (("lossless", lossless_pack), ("lossless_lod", lossless_lod_pack), ("lossless_nbr", lossless_nbr_pack)):
            data = bytes(F[f"{name}_g{group}"])
            assert data[0] == C.VERSION_BYTES[name]
            if name != "lossless":
                assert lossless_nbr_pack.module_of(data) is mod
            side = mod.read(data, C.N_BLOCKS)
            assert side["group"] == group and side["n_blocks"] == C.N_BLOCKS
            assert len(side["nwords"]) == -(-C.N_BLOCKS // group)
    data = bytes(F["lod_pack"])
    assert data[0] == C.VERSION_BYTES["lod_pack"]
    lod = lod_pack.read_lod_pack(data, CFG[tag][1])
    assert 0.0 < lod["t"][0] < 1.0 and 0.0 < lod["t"][1] < 1.0
    for k in lod_pack.HEAD_KEYS:      # the heads the pack carries are the float16 numbers the fixture states
        assert np.array_equal(lod["state"][k].numpy(), F["heads/" + k].astype(np.float32))
    mode, t = thh_select.read_thh_pack(bytes(F["thh_count_pack"]))
    assert mode == "count" and 0.0 < t < 1.0
    mode, k_b = thh_select.read_thh_pack(bytes(F["thh_block_pack"]))
    assert mode == "block-count" and np.array_equal(k_b, gt.sum(1))


@pytest.mark.parametrize("tag", C.TAGS)
def test_the_detector_is_live(tag, golden_dir, gt):
    """Both negative controls, each next to its positive: the digest of p sees one mantissa bit, and the decode of the
    v1 pack sees one voxel in the neighbouring context."""
    F = fixture(golden_dir, tag)
    # (a) a whole block of float32 whose sampled voxels are the committed ones: its digest, then with one bit flipped
    block = np.zeros(C.VOX, np.uint32)
    block[F["p_sample_index"]] = F["p_sample_bits"][3]
    flipped = block.copy()
    flipped[F["p_sample_index"][17]] ^= 1
    a, b = C.sha_rows(block.view(np.float32)[None]), C.sha_rows(flipped.view(np.float32)[None])
    assert np.array_equal(a, C.sha_rows(block.copy().view(np.float32)[None])) and not np.array_equal(a, b)
    want = {"sha": a, "bits": block[F["p_sample_index"]][None]}
    assert C.diagnose(block.view(np.float32)[None], want["sha"], F["p_sample_index"], want["bits"], "p") is None
    msg = C.diagnose(flipped.view(np.float32)[None], want["sha"], F["p_sample_index"], want["bits"], "p")
    assert "blocks [0]" in msg and "1 of 538 sampled voxels differ, largest ulp distance 1" in msg
    # (b) an occupied voxel of block 7 and an empty one of block 2, each moved to the context next to its own
    data = F["lossless_g2"]
    assert np.array_equal(decode_v1(data, F["ctx0"]), gt)
    f1 = lossless_pack.read(bytes(data))["f1"]
    # (two contexts of one frequency code alike -- the saturated ends of the table hold runs of them --, so the voxel is
    # the first of its kind whose neighbouring context, same side and next bucket, has another frequency)
    for blk, occupied in ((7, True), (2, False)):
        c0 = F["ctx0"][blk].astype(np.int64)
        nxt = np.minimum(c0 + 2, 255)
        v = int(np.flatnonzero((gt[blk] == occupied) & (c0 + 2 < 256) & (f1[nxt] != f1[c0]))[0])
        ctx = F["ctx0"].copy()
        ctx[blk, v] += 2
        try:
            got = decode_v1(data, ctx)
        except (ValueError, IndexError):
            continue
        assert not np.array_equal(got, gt)
