"""The eval route of THIS build against bits that are written down, and the decoders against side packs this build did
not write: tests/golden/conformance_{S,W}.npz (tools/make_conformance_fixture.py; DESIGN.md, "What the side packs fix").

tests/test_gpu_decode_bits.py holds the route to one set of bits inside a build; here the set itself is pinned, for the
two committed trained decoders and all 12 blocks of their packs:

  1. eval bits    sha256 of every block's p from Net.reconstruct at batch 1, 5 and 12, from TrainEngine.eval_forward over
                  all blocks and block by block, and of both coarse heads from Net.reconstruct_lod;
  2. contexts     the device's classification of p per block against the committed voxel contexts, and the device's
                  pyramid against the pooled contexts that follow from them (tests/conformance_ref.py);
  3. decoding     the committed lossless_pack / lossless_lod_pack (versions 1 and 3) bytes, both group sizes, batch 1, 5
                  and 12, levels 0 / 1 / 2, against the numpy ground truth and its max-pools;
  4. re-encoding  the three encoders give the committed bytes at both group sizes and at batch 5 and 12;
  5. lod_pack, thh_pack   the committed bytes select the committed cells / counts, and the count rule holds against the
                  numpy ground truth.

Everything is equality: no tolerance, no voxel left out.  A mismatch of the bits is reported as "n of m sampled voxels
differ, largest ulp distance d" (conformance_ref.diagnose).  tests/test_conformance_cpu.py is the host half."""
import numpy as np
import pytest
import torch

from tests import conformance_ref as C
from tests import occ_hier_ref as H
from tests import occ_rans_ref as R

pytestmark = pytest.mark.gpu
BATCHES = (1, 5, 12)
_STATE = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def gt():
    return C.ground_truth()


class State:
    pass


def state(tag, gpu, golden_dir):
    """The fixture, the decoder with the fixture's own heads, the pack's latents and origins: built once per tag and
    left unchanged by every test."""
    if tag not in _STATE:
        S = State()
        S.F = C.load(golden_dir, tag)
        S.net, S.lat, S.origins = C.build_decoder(golden_dir, tag, gpu, {k[len("heads/"):]: v for k, v in S.F.items()
                                                                         if k.startswith("heads/")})
        _STATE[tag] = S
    return _STATE[tag]


def check_bits(S, name, got, what):
    F = S.F
    msg = C.diagnose(got.reshape(C.N_BLOCKS, -1).cpu().numpy(), F[name + "_sha"], F[name + "_sample_index"],
                     F[name + "_sample_bits"], what)
    assert msg is None, msg


def words_of(rows):
    """bool [12, cells] -> the occupancy words as the device holds them: int64 [12, cells / 64]."""
    return H.words_of(rows).view(np.int64)


# ---------------------------------------------------------------- 1. eval bits
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("tag", C.TAGS)
def test_reconstruct_gives_the_committed_bits(tag, batch, gpu, golden_dir):
    S = state(tag, gpu, golden_dir)
    check_bits(S, "p", C.batched(lambda x: S.net.reconstruct(x, 2), S.lat, batch), f"{tag}: Net.reconstruct at batch {batch}")


@pytest.mark.parametrize("tag", C.TAGS)
def test_engine_eval_forward_gives_the_committed_bits(tag, gpu, golden_dir):
    S = state(tag, gpu, golden_dir)
    eng, lat = C.build_engine(golden_dir, tag, gpu)
    a = eng.eval_forward(q=2)
    assert torch.equal(a["x0"], lat) and torch.equal(lat, S.lat), "the engine's quantiser hands on the pack's latents"
    check_bits(S, "p", a["p2"], f"{tag}: TrainEngine.eval_forward over all blocks")
    singles = torch.cat([eng.eval_forward(lo=b, hi=b + 1, q=2)["p2"] for b in range(C.N_BLOCKS)], 0)
    check_bits(S, "p", singles, f"{tag}: TrainEngine.eval_forward(lo, lo + 1)")


@pytest.mark.parametrize("tag", C.TAGS)
def test_coarse_heads_give_the_committed_bits(tag, gpu, golden_dir):
    S = state(tag, gpu, golden_dir)
    for lod, name in ((1, "cls1"), (2, "cls0")):
        for batch in BATCHES:
            p = C.batched(lambda x: S.net.reconstruct_lod(x, lod, 2, return_p=True)[1], S.lat, batch)
            check_bits(S, name, p, f"{tag}: Net.reconstruct_lod level {lod} at batch {batch}")
        heads = C.batched(lambda x: S.net.reconstructor(x, 2)[1][2 - lod], S.lat, C.N_BLOCKS)
        check_bits(S, name, heads, f"{tag}: head {2 - lod} of the full forward")


# ---------------------------------------------------------------- 2. contexts
@pytest.mark.parametrize("tag", C.TAGS)
def test_device_contexts_are_the_committed_ones(tag, gpu, golden_dir, gt):
    from nvfpcc_amd import ops
    S = state(tag, gpu, golden_dir)
    ctx0 = S.F["ctx0"].astype(np.int64)
    p = C.batched(lambda x: S.net.reconstruct(x, 2), S.lat, C.N_BLOCKS)
    g = torch.from_numpy(gt.reshape(-1, 1, 32, 32, 32)).float().to(gpu)
    for b in range(C.N_BLOCKS):
        cnt, occ, bad = (t.cpu().numpy() for t in ops.occ_ctx_hist(p[b:b + 1].contiguous(), g[b:b + 1].contiguous()))
        assert int(bad[0]) == 0
        assert np.array_equal(cnt, np.bincount(ctx0[b], minlength=256)), f"{tag}: voxels per context, block {b}"
        assert np.array_equal(occ, np.bincount(ctx0[b][gt[b]], minlength=256)), f"{tag}: occupied per context, block {b}"
    # the pyramid of the device's field has the contexts and child counts that follow from ctx0 alone
    pyr = ops.occ_hier_pyramid(p)
    p1, k1, p2, k2 = H.pyramid(C.surrogate_p(S.F["ctx0"]))
    assert int(pyr["bad"].item()) == 0
    assert np.array_equal(R.contexts(pyr["p1"].cpu().numpy()), R.contexts(p1)) and np.array_equal(pyr["k1"].cpu().numpy(), k1)
    assert np.array_equal(R.contexts(pyr["p2"].cpu().numpy()), R.contexts(p2)) and np.array_equal(pyr["k2"].cpu().numpy(), k2)


# ---------------------------------------------------------------- 3. decoding committed packs
def coder(name):
    from nvfpcc_amd import lossless_lod_pack, lossless_nbr_pack, lossless_pack
    return {"lossless": lossless_pack, "lossless_lod": lossless_lod_pack, "lossless_nbr": lossless_nbr_pack}[name]


@pytest.mark.parametrize("name", C.CODERS)
@pytest.mark.parametrize("tag", C.TAGS)
def test_committed_packs_decode_to_the_numpy_ground_truth(tag, name, gpu, golden_dir, gt):
    from nvfpcc_amd import lossless_nbr_pack
    S = state(tag, gpu, golden_dir)
    want = C.unpack_levels(gt)
    for group in C.GROUPS:
        data = bytes(S.F[f"{name}_g{group}"])
        mod = coder(name) if name == "lossless" else lossless_nbr_pack.module_of(data)      # as decode picks it
        assert mod is coder(name)
        for batch in BATCHES:
            for level in ((0,) if name == "lossless" else (0, 1, 2)):
                kw = {} if name == "lossless" else {"level": level}
                words, counts = mod.decode_occupancy(S.net, S.lat, data, batch=batch, **kw)
                what = f"{tag} {name}: group {group}, batch {batch}, level {level}"
                assert np.array_equal(words.cpu().numpy(), words_of(want[level])), what
                assert counts.tolist() == want[level].sum(1).tolist(), what


# ---------------------------------------------------------------- 4. re-encoding
@pytest.mark.parametrize("name", C.CODERS)
@pytest.mark.parametrize("tag", C.TAGS)
def test_encoders_give_the_committed_bytes(tag, name, gpu, golden_dir, gt):
    S = state(tag, gpu, golden_dir)
    g = torch.from_numpy(gt.reshape(-1, 1, 32, 32, 32)).float().to(gpu)
    for group in C.GROUPS:
        for batch in (5, 12):
            data, _ = coder(name).encode_occupancy(S.net, S.lat, g, batch=batch, group=group)
            assert data == bytes(S.F[f"{name}_g{group}"]), f"{tag} {name}: group {group}, encode batch {batch}"


# ---------------------------------------------------------------- 5. lod_pack and thh_pack
@pytest.mark.parametrize("tag", C.TAGS)
def test_committed_lod_pack_selects_the_committed_cells(tag, gpu, golden_dir, gt):
    from nvfpcc_amd import lod_pack
    from nvfpcc_amd.recon import reconstruct_points_lod
    from tests.test_trained_golden import CFG
    S = state(tag, gpu, golden_dir)
    F = S.F
    side = lod_pack.read_lod_pack(bytes(F["lod_pack"]), CFG[tag][1])
    # a decoder as decode --lod builds it: the trained pack, then the heads of the lod_pack's own bytes
    net, lat, origins = C.build_decoder(golden_dir, tag, gpu)
    net.load_state_dict({k: v.to(gpu) for k, v in side["state"].items()}, strict=False)
    levels = C.unpack_levels(gt)
    for level in (1, 2):
        k = int(levels[level].sum())
        assert k == int(F["lod_k"][level - 1])
        want = np.unpackbits(F[f"lod_occ{level}"], axis=1).astype(bool)
        for batch in BATCHES:
            pts, counts = reconstruct_points_lod(net, lat, origins, level, side["t"][level - 1], batch=batch)
            what = f"{tag}: level {level}, batch {batch}"
            assert np.array_equal(counts, F["lod_counts"][level - 1]), what
            assert np.array_equal(C.occupancy_of_points(pts, counts, origins, level), want), what
        # the count rule against the input's own max-pool: at least k, and k exactly where nothing ties at the k-th value
        kept = int(want.sum())
        assert kept >= k and (kept == k or int(F["lod_ties"][level - 1]) > 1), (tag, level, kept, k)
    # encode --pack_lod at HEAD writes these bytes
    sel = C.lod_selection(S.net, S.lat, S.origins, levels, C.ENCODE_BATCH)
    sd = S.net.state_dict()
    assert lod_pack.write_lod_pack(sel["t"][0], sel["t"][1], *[sd[k] for k in lod_pack.HEAD_KEYS]) == bytes(F["lod_pack"])


@pytest.mark.parametrize("tag", C.TAGS)
def test_committed_thh_packs_select_the_committed_counts(tag, gpu, golden_dir, gt):
    from nvfpcc_amd import thh_select as ts
    from nvfpcc_amd.recon import reconstruct_points
    S = state(tag, gpu, golden_dir)
    F = S.F
    n_points, k_b = int(gt.sum()), gt.sum(1)
    for batch in BATCHES:
        mode, t = ts.read_thh_pack(bytes(F["thh_count_pack"]))
        pts, counts = reconstruct_points(S.net, S.lat, S.origins, t, batch=batch)
        assert mode == "count" and np.array_equal(counts, F["thh_count_counts"]), f"{tag}: count, batch {batch}"
        assert pts.shape[0] >= n_points and (pts.shape[0] == n_points or int(F["thh_count_ties"]) > 1)
        mode, k = ts.read_thh_pack(bytes(F["thh_block_pack"]))
        pts, counts = reconstruct_points(S.net, S.lat, S.origins, None, batch=batch, block_counts=k)
        assert mode == "block-count" and np.array_equal(k, k_b)
        assert np.array_equal(counts, F["thh_block_counts"]), f"{tag}: block-count, batch {batch}"
        assert (counts >= k_b).all() and ((counts == k_b) | (F["thh_block_ties"] > 1)).all()
        assert pts.shape[0] >= n_points
    # encode --thh_mode at HEAD writes these bytes
    p_all = C.batched(lambda x: S.net.reconstruct(x, 2), S.lat, C.ENCODE_BATCH)
    assert ts.write_thh_pack("count", t=ts.choose("count", p_all, n_points=n_points)["t"]) == bytes(F["thh_count_pack"])
    assert ts.write_thh_pack("block-count", block_counts=k_b) == bytes(F["thh_block_pack"])
