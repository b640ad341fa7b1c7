"""CPU: the float64 restatement of the reconstruction score (tests/quality_ref.py) on known answers and against a
window-by-window evaluation; quality.scores_from_sums / evaluate; the metrics.csv writer and the CLI's reducers."""
import math

import numpy as np
import pytest
import torch

from gflow_amd import fit_video as FV
from gflow_amd import quality as QL
from tests import quality_ref as R


def _bytes(rng, h, w):
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_window():
    g = R.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15
    np.testing.assert_array_equal(g, g[::-1])
    assert g[5] / g[4] == pytest.approx(math.exp(1.0 / 4.5), rel=1e-15)


@pytest.mark.parametrize("h,w", [(11, 11), (13, 29), (40, 17)])
def test_identical_images_score_one_and_80_db(h, w):
    k = _bytes(np.random.default_rng(h * w), h, w)
    gt = R.read_back(k).astype(np.float32)                # (uint8 / 255 in float32: the target IS the read-back prediction)
    sse, ssim_sum = R.sums(k, gt)
    assert sse == 0.0
    assert abs(float(R.ssim(ssim_sum, h, w)) - 1.0) <= 1e-12
    assert abs(float(R.psnr(sse, h, w)) - 80.0) <= 1e-12
    psnr, ssim = QL.scores_from_sums(sse, ssim_sum, h, w)
    assert abs(float(psnr) - 80.0) <= 1e-12 and abs(float(ssim) - 1.0) <= 1e-12


@pytest.mark.parametrize("ka,kb", [(0, 255), (255, 0), (17, 200), (128, 128), (0, 0), (3, 4)])
def test_constant_images_have_the_closed_form(ka, kb):
    h, w = 15, 22
    pred = np.full((h, w, 3), ka, dtype=np.uint8)
    gt = np.full((h, w, 3), np.float32(kb) / np.float32(255.0), dtype=np.float32)
    a, b = float(np.float32(ka) / np.float32(255.0)), float(np.float32(kb) / np.float32(255.0))
    sse, ssim_sum = R.sums(pred, gt)
    assert float(R.ssim(ssim_sum, h, w)) == pytest.approx((2 * a * b + R.C1) / (a * a + b * b + R.C1), abs=1e-12)
    assert sse == pytest.approx(3 * h * w * (a - b) ** 2, rel=1e-12, abs=1e-300)


def test_restatement_equals_a_window_by_window_evaluation():
    rng = np.random.default_rng(5)
    h, w = 13, 14
    k = _bytes(rng, h, w)
    gt = rng.uniform(-0.2, 1.2, size=(h, w, 3)).astype(np.float32)
    x, y = R.read_back(k), np.clip(gt, 0, 1).astype(np.float64)
    g2 = np.outer(R.window(), R.window())
    total = 0.0
    for c in range(3):
        for i in range(h - 10):
            for j in range(w - 10):
                a, b = x[i:i + 11, j:j + 11, c], y[i:i + 11, j:j + 11, c]
                ma, mb = (g2 * a).sum(), (g2 * b).sum()
                saa, sbb, sab = (g2 * a * a).sum() - ma * ma, (g2 * b * b).sum() - mb * mb, (g2 * a * b).sum() - ma * mb
                total += (2 * ma * mb + R.C1) * (2 * sab + R.C2) / ((ma * ma + mb * mb + R.C1) * (saa + sbb + R.C2))
    sse, ssim_sum = R.sums(k, gt)
    assert ssim_sum == pytest.approx(total, rel=1e-12)
    assert sse == pytest.approx(((x - y) ** 2).sum(), rel=1e-14)


def test_bytes_of_truncates_and_clamps():
    vals = torch.tensor([-0.5, -0.0, 0.0, 0.9 / 255, 1.5 / 255, 254.9 / 255, 1.0, float(np.nextafter(np.float32(1), np.float32(2))),
                         7.0], dtype=torch.float32)
    chw = vals.reshape(1, 1, -1).repeat(4, 1, 1)
    k = R.bytes_of(chw)
    assert k.shape == (1, vals.numel(), 3)
    np.testing.assert_array_equal(k[0, :, 0], [0, 0, 0, 0, 1, 254, 255, 255, 255])


def test_scores_from_sums_and_evaluate():
    h, w = 30, 50
    sse, ss = np.array([0.0, 4.5, 900.0]), np.array([2400.0, 1200.0, 0.0])
    psnr, ssim = QL.scores_from_sums(sse, ss, h, w)
    np.testing.assert_array_equal(psnr, R.psnr(sse, h, w))
    np.testing.assert_array_equal(ssim, R.ssim(ss, h, w))
    assert psnr.dtype == np.float64 and ssim[0] == 1.0 and ssim[1] == 0.5
    ev = QL.evaluate(dict(PSNR=psnr, SSIM=ssim))
    assert ev == {"PSNR": float(np.mean(psnr)), "SSIM": float(np.mean(ssim)), "frames": 3}
    assert math.isnan(QL.evaluate(dict(PSNR=[], SSIM=[]))["PSNR"])


def test_recorder_refuses_images_smaller_than_the_window():
    for h, w in ((10, 40), (40, 10)):
        with pytest.raises(ValueError):
            QL.ReconRecorder(2, h, w, "cpu")


def test_csv_for_a_partial_set_of_blocks(tmp_path):
    p = tmp_path / "metrics.csv"
    QL.write_metrics_csv(p, {"RPE_t": 0.25, "ATE": None, "RPE_r": 1.5, "SSIM": 0.75, "PSNR": 31.0})
    assert p.read_text() == "PSNR,31.0\nSSIM,0.75\nATE,None\nRPE_t,0.25\nRPE_r,1.5\n"
    full = {k: float(i) for i, k in enumerate(QL.CSV_KEYS)}
    QL.write_metrics_csv(p, dict(reversed(list(full.items()))))
    assert [ln.split(",")[0] for ln in p.read_text().splitlines()] == [
        "PSNR", "SSIM", "Occlusion_Accuracy", "Average_Jaccard", "Average_PTS_within_threshold", "J_zero", "F_zero",
        "J&F_zero", "ATE", "RPE_t", "RPE_r"]
    assert [float(ln.split(",")[1]) for ln in p.read_text().splitlines()] == list(full.values())
    QL.write_metrics_csv(p, {})
    assert p.read_text() == ""
    with pytest.raises(ValueError):
        QL.write_metrics_csv(p, {"LPIPS": 0.1})


def test_csv_metrics_takes_only_the_blocks_that_are_there():
    line = {"psnr_sum": 1.0, "recon": {"PSNR": 30.0, "SSIM": 0.9, "frames": 8, "clips": 2},
            "camera": {"ATE": None, "RPE_t": None, "RPE_r": None, "clips": 0, "clips_unscored": 2}}
    assert FV.csv_metrics(line) == {"PSNR": 30.0, "SSIM": 0.9, "ATE": None, "RPE_t": None, "RPE_r": None}
    line = {"tapvid": {"occlusion_accuracy": 0.5, "average_jaccard": 0.25, "average_pts_within_thresh": 0.75, "clips": 1,
                       "queries_dropped": 0},
            "davis": {"J": 0.1, "F": 0.2, "J&F": 0.15, "frames_scored": 3, "clips": 1}}
    assert FV.csv_metrics(line) == {"Occlusion_Accuracy": 0.5, "Average_Jaccard": 0.25, "Average_PTS_within_threshold": 0.75,
                                    "J_zero": 0.1, "F_zero": 0.2, "J&F_zero": 0.15}
    assert FV.csv_metrics({"frames": 3}) == {}


def test_reducers_average_over_clips():
    recs = {0: dict(PSNR=np.array([30.0, 32.0]), SSIM=np.array([0.5, 0.7])), 3: dict(PSNR=np.array([20.0]), SSIM=np.array([0.2]))}
    r = FV.reduce_recon(recs)
    assert r == {"PSNR": (31.0 + 20.0) / 2, "SSIM": (0.6 + 0.2) / 2, "frames": 3, "clips": 2}
    cams = {0: dict(extr=None, ATE=0.5, RPE_t=0.25, RPE_r=2.0), 1: dict(extr=None, ATE=None, RPE_t=None, RPE_r=None),
            2: dict(extr=None, ATE=1.5, RPE_t=0.75, RPE_r=4.0)}
    c = FV.reduce_camera(cams)
    assert c == {"ATE": 1.0, "RPE_t": 0.5, "RPE_r": 3.0, "clips": 2, "clips_unscored": 1}
    c = FV.reduce_camera({1: cams[1]})
    assert c == {"ATE": None, "RPE_t": None, "RPE_r": None, "clips": 0, "clips_unscored": 1}
