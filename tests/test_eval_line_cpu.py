"""Host arithmetic of the TEST and TRAIN log lines (NVFPCC.test_fields_from_sums, TrainEngine.train_log_fields) on
hand-made sums with hand-computed fields; no device."""
import types

import numpy as np

import NVFPCC
from nvfpcc_amd.engine import TrainEngine

# focal terms | main output: tp ap tn an sse denom | head 0 | head 1 | latent bits
SUMS = np.array([12.5, 3.25, 1.75, 30, 40, 900, 1000, 50.0, 25, 5, 8, 30, 60, 0, 10, 4, 16, 160, 200, 0, 20, 400.0])
ARGS = dict(weight_bits=2000.0, n_pts=80.0, n_points=1000.0, lmbda=200.0, network_bits=2600.0)


def psnr(mse, peak):
    return 20 * np.log10(peak / np.sqrt(mse / 3))


def test_test_line_fields_from_hand_made_sums():
    f = NVFPCC.test_fields_from_sums(SUMS, **ARGS)
    # b_latent = 400 / 80 = 5, b_net = 2000 / 1000 = 2; Loss = 17.5 + 200 * (5 + 2): no w1 / w2 (reference NVFPCC.py:347)
    want = [1417.5, 0.0, 0.0, 0.75, 0.9, 3.25, 1.75, 0.625, 0.5, 0.25, 0.8, 7.0, 5.0, 2.0, 3.0, 2.0, psnr(2.0, 1023)]
    assert len(f) == 17
    np.testing.assert_allclose(np.asarray(f, np.float64), want, rtol=1e-12)
    # the peak moves PSNR1 only: 20 log10(4095 / 1023) dB
    f12 = NVFPCC.test_fields_from_sums(SUMS, peak=4095, **ARGS)
    assert f12[:16] == f[:16]
    np.testing.assert_allclose(f12[16] - f[16], 20 * np.log10(4095 / 1023), rtol=1e-12)
    line = NVFPCC.TEST_LINE % ((7, 1.5) + tuple(f))
    assert line.startswith("[Epoch 0007 TEST 1.5 seconds] Loss: 1.4175e+03 PosiPenal: 0.0000 PosiGain: 0.0000 Pacc: 0.7500 "
                           "Nacc: 0.9000 S1 Loss: 3.2500 S2 Loss: 1.7500 S1Pacc: 0.6250 S1Nacc: 0.5000 S2Pacc: 0.2500 "
                           "S2Nacc: 0.8000 bpp: 7.0000 b_latent: 5.0000 b_net: 2.0000 b_all: 3.0000 MSE1: 2.0000 PSNR1: ")
    assert line.endswith("%.4f" % psnr(2.0, 1023))


def test_zero_over_zero_prints_nan_as_the_reference_does():
    s = SUMS.copy()
    s[3 + 6:3 + 8] = 0          # head 0 has no occupied voxel: S1Pacc = 0 / 0
    s[3 + 12 + 2:3 + 12 + 4] = 0  # head 1 has no empty voxel: S2Nacc = 0 / 0
    s[3 + 4:3 + 6] = 0          # nothing above 0.6: MSE1 = 0 / 0
    f = np.asarray(NVFPCC.test_fields_from_sums(s, **ARGS), np.float64)
    assert np.isnan(f[[7, 10, 15, 16]]).all()
    assert np.isfinite(np.delete(f, [7, 10, 15, 16])).all() and f[8] == 0.5 and f[9] == 0.25 and f[3] == 0.75
    assert "S1Pacc: nan" in NVFPCC.TEST_LINE % ((0, 0.0) + tuple(f)) and "MSE1: nan PSNR1: nan" in NVFPCC.TEST_LINE % ((0, 0.0) + tuple(f))
    # selected voxels that all sit on the surface: MSE1 = 0, PSNR1 = +inf (the reference prints inf)
    s = SUMS.copy()
    s[3 + 4] = 0
    f = NVFPCC.test_fields_from_sums(s, **ARGS)
    assert f[15] == 0.0 and np.isposinf(f[16])


def test_train_line_fields_from_hand_made_epoch_sums():
    eng = types.SimpleNamespace(lmbda=200.0, w1=10.0, w2=57.0)
    # focal terms x 3, b_latent, b_net, bad terms, bad gradients, steps, six ratio sums, sse, denom -- over 4 steps
    acc = np.array([8.0, 2.0, 1.0, 0.5, 0.25, 0, 0, 4, 3.0, 3.6, 2.0, 1.0, 0.5, 3.2, 90.0, 30.0])
    f = TrainEngine.train_log_fields(eng, acc, 4)
    # means: ls = 2, 0.5, 0.25; bl = 0.125, bn = 0.0625; Loss = 2.75 + 200 * (1.25 + 3.5625)
    want = [965.25, 0.0, 0.0, 0.75, 0.9, 0.5, 0.25, 0.5, 0.25, 0.125, 0.8, 0.1875, 0.125, 0.0625, 3.0, psnr(3.0, 1023)]
    assert len(f) == 16
    np.testing.assert_allclose(np.asarray(f, np.float64), want, rtol=1e-12)
    f12 = TrainEngine.train_log_fields(eng, acc, 4, peak=4095)
    np.testing.assert_allclose(f12[15], psnr(3.0, 4095), rtol=1e-12)
    assert list(f12[:15]) == list(f[:15])
    line = NVFPCC.TRAIN_LINE % ((3, 2.0) + tuple(f))
    assert "Pacc: 0.7500 Nacc: 0.9000" in line and "MSE1: 3.0000 PSNR1: %.4f" % psnr(3.0, 1023) in line
    acc[14:16] = 0              # nothing above 0.6 in the whole epoch
    f = TrainEngine.train_log_fields(eng, acc, 4)
    assert np.isnan(f[14]) and np.isnan(f[15]) and np.isfinite(np.asarray(f[:14], np.float64)).all()
    assert (NVFPCC.TRAIN_LINE % ((3, 2.0) + tuple(f))).endswith("MSE1: nan PSNR1: nan")
