"""Host half of the threshold selection (nvfpcc_amd/thh_select.py): digit choice, nextafter rule, curve folding,
thh_pack coding, parser defaults, the squared-distance recovery bound, and the numpy restatement the GPU tests compare
against (tests/thh_select_ref.py), checked on hand-made cases.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from nvfpcc_amd import thh_select as ts
from tests import thh_select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def radix_kth(p, k):
    """thh_select.kth_largest's loop with the reference histogram in the kernel's place (one row = whole cloud)."""
    kk = torch.tensor([min(max(int(k), 1), p.size)])
    key, prefix = torch.zeros(1, dtype=torch.int64), None
    for shift, nbits in ts.PASSES:
        count = R.digit_hist(p, shift, nbits, prefix)[0]
        digit, kk = ts.choose_digit(torch.from_numpy(count)[None], kk)
        key = (key << nbits) | digit
        prefix = int(key)
    return key.to(torch.int32).view(torch.float32).numpy()[0]


def test_passes_cover_the_key():
    assert sum(n for _, n in ts.PASSES) == 32 and all(n <= 11 for _, n in ts.PASSES)
    assert [s for s, _ in ts.PASSES] == [21, 10, 0]


def test_choose_digit_from_cumulative_counts():
    hist = torch.tensor([[3, 0, 2, 1], [0, 5, 0, 0]])
    # row 0, descending: digit 3 x1, digit 2 x2, digit 0 x3
    for k, (d, rest) in {1: (3, 1), 2: (2, 1), 3: (2, 2), 4: (0, 1), 6: (0, 3)}.items():
        digit, kr = ts.choose_digit(hist[:1], torch.tensor([k]))
        assert (int(digit), int(kr)) == (d, rest), k
    digit, kr = ts.choose_digit(hist, torch.tensor([3, 5]))
    assert digit.tolist() == [2, 1] and kr.tolist() == [2, 5]


def test_radix_select_equals_sorting_on_hand_made_fields():
    rng = np.random.default_rng(3)
    fields = {
        "uniform": rng.random(5000, dtype=np.float32),
        "saturated": np.concatenate([np.zeros(4000, np.float32), np.ones(300, np.float32),
                                     rng.random(200, dtype=np.float32)]),
        "equal": np.full(777, 0.25, np.float32),
        "ends": np.array([0.0, -0.0, 1.0, 1e-45, 0.5, 0.5, 0.5], np.float32),
    }
    for name, p in fields.items():
        for k in (1, 2, 3, p.size // 2, p.size - 1, p.size, p.size + 5):
            got, want = radix_kth(p, k), R.kth_largest(p, k)
            assert got == want, (name, k, got, want)


def test_reference_select_on_hand_made_cases():
    p = np.array([0.1, 0.9, 0.5, 0.5, 0.5, 0.0], np.float32)
    assert R.kth_largest(p, 1) == np.float32(0.9) and R.kth_largest(p, 2) == np.float32(0.5)
    assert R.kth_largest(p, 4) == np.float32(0.5) and R.kth_largest(p, 5) == np.float32(0.1)
    assert R.kth_largest(p, 6) == 0.0 and R.kth_largest(p, 99) == 0.0 and np.isinf(R.kth_largest(p, 0))
    # the tie rule: asking for 2 keeps all three 0.5s
    t = R.threshold_for_count(p, 2)
    assert t < np.float32(0.5) and np.nextafter(t, np.float32(1)) == np.float32(0.5) and int((p > t).sum()) == 4
    assert int((p > R.threshold_for_count(p, 0)).sum()) == 0 and int((p > R.threshold_for_count(p, 6)).sum()) == 6
    c = R.curve(p, np.array([0, 1, 1, 0, 1, 0], np.uint8), np.array([4, 0, 0, 1, 0, 9]), [0.0, 0.1, 0.5])
    assert c["count"] == [5, 4, 1] and c["tp"] == [3, 3, 1] and c["sse"] == [5, 1, 0]
    cnt, s, g, bad = R.digit_hist(np.array([0.0, 1.0, 1.0, np.nan, 2.0, -1.0], np.float32), 21, 11,
                                  d2=np.arange(6), gt=np.ones(6, np.uint8))
    assert bad == 3 and cnt[0] == 1 and cnt[0x3F800000 >> 21] == 2 and cnt.sum() == 3
    assert s[0x3F800000 >> 21] == 3 and g.sum() == 3


def test_nextafter_rule():
    v = torch.tensor([0.5, 1.0, 0.0, float("inf"), 1e-45])
    t = ts.threshold_below(v)
    assert t.dtype == torch.float32
    assert t[0].item() == np.nextafter(np.float32(0.5), np.float32(-1)) and t[1].item() < 1.0
    assert t[2].item() < 0 and not (torch.tensor(0.0) <= t[2])            # p = 0 passes p > t
    assert t[3].item() == np.finfo(np.float32).max                         # k = 0: nothing is above FLT_MAX
    assert t[4].item() == 0.0
    for a, b in zip(v[:3].tolist(), t[:3].tolist()):
        assert np.nextafter(np.float32(b), np.float32(np.inf)) == np.float32(a)


def test_fold_curve_places_candidates_on_bin_edges():
    rng = np.random.default_rng(5)
    p = rng.random((3, 400), dtype=np.float32)
    p[0, :50] = 0.0
    p[1, :50] = 1.0
    gt = (rng.random((3, 400)) < 0.3).astype(np.uint8)
    d2 = rng.integers(0, 3000, (3, 400))
    cand = np.array([0.0, 0.25, 0.5, 0.5, 0.9, 1.0], np.float32)
    bins = np.stack([np.searchsorted(cand, p[b], side="left") for b in range(3)])      # edges below p
    hist = lambda w: np.stack([np.bincount(bins[b], weights=w[b], minlength=cand.size + 1) for b in range(3)]).astype(np.int64)
    out = ts.fold_curve(hist(np.ones_like(d2)), hist(d2), hist(gt))
    want = R.curve(p, gt, d2, cand)
    for k in ("count", "sse", "tp"):
        assert out[k].dtype == torch.int64 and out[k].tolist() == want[k], k
    assert ts.fold_curve(hist(np.ones_like(d2)))["sse"] is None


def test_thh_pack_round_trip_and_count_coding():
    for mode in ("count", "d1"):
        for t in (0.64, float(np.float32(0.1)), float(np.finfo(np.float32).max), -1e-45):
            data = ts.write_thh_pack(mode, t=t)
            assert isinstance(data, bytes) and len(data) == 5
            m, v = ts.read_thh_pack(data)
            assert m == mode and np.float32(v) == np.float32(t)
    k = np.array([0, 1, 936, 32768, 65535])
    data = ts.write_thh_pack("block-count", block_counts=k)
    assert len(data) == 1 + 2 * k.size and data[1:3] == b"\x00\x00" and data[7:9] == b"\x00\x80"    # little endian
    m, v = ts.read_thh_pack(data)
    assert m == "block-count" and v.dtype == np.int64 and v.tolist() == k.tolist()
    assert ts.decode_block_counts(ts.encode_block_counts(torch.tensor([32768, 0]))).tolist() == [32768, 0]
    with pytest.raises(ValueError):
        ts.encode_block_counts([65536])
    with pytest.raises(ValueError):
        ts.encode_block_counts([-1])
    with pytest.raises(ValueError):
        ts.read_thh_pack(b"\x09abcd")
    with pytest.raises(ValueError):
        ts.read_thh_pack(b"\x02abc")
    with pytest.raises(ValueError):
        ts.write_thh_pack("fixed", t=0.5)
    assert ts.threshold_line("count", t=0.64) == "[Threshold] mode: count t: 0.639999986"
    assert ts.threshold_line("block-count", block_counts=[3, 4], thresholds=[0.25, 0.5]) == \
        "[Threshold] mode: block-count blocks: 2 points asked: 7 t_min: 0.25 t_max: 0.5"


def test_parser_defaults_are_todays():
    sys_argv, sys.argv = sys.argv, [sys.argv[0]]
    try:
        import NVFPCC as cli
    finally:
        sys.argv = sys_argv
    a = cli.build_parser().parse_args(["encode", "x.ply"])
    assert a.thh_mode is None and a.thh == 0.6 and a.pack_fn == "pack.pk"
    today = {"command", "input", "checkpoint_dir", "batchsize", "lmbda", "load_weights", "load_extern", "lr", "alpha",
             "use_coords", "real", "dsep", "stat_latent", "stat_net", "w1", "w2", "notes", "load_meta", "shuffle",
             "phase_change", "wemb", "ch", "load_emb", "chanstr", "thh", "pack_fn", "N", "qp", "device", "epochs", "seed",
             "ref_ply"}
    assert set(vars(a)) == today | {"thh_mode"}
    for m in ("fixed", "count", "block-count", "d1"):
        assert cli.build_parser().parse_args(["decode", "pack.pk", "--thh_mode", m]).thh_mode == m
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["decode", "pack.pk", "--thh_mode", "best"])


def test_squared_distance_is_recovered_exactly_below_the_bound():
    """d2_from_dist: every integer below 2^22 survives sqrt -> float32 -> square -> round (and float64 likewise)."""
    assert ts.D2_EXACT_BOUND == 1 << 22 and 3 * 1023 ** 2 < ts.D2_EXACT_BOUND
    n = np.arange(ts.D2_EXACT_BOUND, dtype=np.int64)
    assert np.array_equal(ts.d2_from_dist(np.sqrt(n.astype(np.float64)).astype(np.float32)).numpy(), n)
    assert np.array_equal(ts.d2_from_dist(np.sqrt(n[::7].astype(np.float64))).numpy(), n[::7])
    assert ts.d2_from_dist(torch.sqrt(torch.arange(4000.0))).dtype == torch.int32
    with pytest.raises(ValueError):
        ts.d2_from_dist(np.array([2048.0]))
    with pytest.raises(ValueError):
        ts.d2_from_dist(np.array([np.nan]))


def test_shortlist_and_budget():
    ks = ts.shortlist_counts(900, 12 * 32768)
    assert len(ks) == 16 and ks[0] == 600 and ks[-1] == 1350 and ks == sorted(ks)
    assert ts.shortlist_counts(0, 100) == [] and ts.shortlist_counts(3, 100) == [2, 3, 4]
    assert ts.shortlist_counts(900, 1000)[-1] == 1000
    assert ts.check_resident(917) == 917 * 131072 and ts.check_resident(32768) == ts.MAX_RESIDENT_BYTES
    with pytest.raises(RuntimeError, match="budget"):
        ts.check_resident(32769)


def test_trained_golden_offers_a_real_shortlist(golden_dir):
    """The d1 test on the GPU runs on the trained narrow golden: its probabilities must give at least 3 distinct
    thresholds whose decoded counts lie between 2/3 and 3/2 of the input's points (checked here with the oracle's
    decoder, as tests/test_trained_golden.py runs it)."""
    from nvfpcc_amd.seeds import synthetic_seed
    from nvfpcc_amd.synth import make_blocks
    from oracle import nvf_oracle as O
    from tests.test_trained_golden import CFG, load_pack, state_from_pack
    pack, G = load_pack(golden_dir, "S")
    ch, channels = CFG["S"]
    P, _ = O.build_state(ch, channels, synthetic_seed())
    P.update(state_from_pack(pack))
    lat = torch.from_numpy(G["latents"].astype(np.float32))
    torch.set_num_threads(8)
    with torch.no_grad():
        probs = np.concatenate([O.decoder(P, lat[i:i + 1], 2)[0].reshape(1, -1).numpy() for i in range(lat.shape[0])])
    n_points = int(make_blocks(lat.shape[0])[0].sum())
    ks = ts.shortlist_counts(n_points, probs.size)
    tset = sorted(set(float(R.threshold_for_count(probs, k)) for k in ks))
    counts = [int((probs > np.float32(t)).sum()) for t in tset]
    inside = [c for c in counts if 2 / 3 * n_points <= c <= 3 / 2 * n_points]
    assert len(set(inside)) >= 3, (n_points, counts)
