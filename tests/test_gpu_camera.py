"""The camera score of a clip fit, and ``recon`` / ``camera`` on every path (``-m gpu``; gflow_amd/camera.py,
gflow_amd/quality.py, fit_video): the recorded poses are the trainer's, their score equals camera.evaluate and the direct
minimisation of tests/camera_ref.py; a fit with both scores is bit for bit the fit without them; the operator path and
concurrent fits hold the same contracts; the CLI's blocks and metrics.csv are the clips' own numbers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import score_fit as SF
from tests.score_fit import FIT, H, W, clip

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fit_camera_path_and_its_score():
    frames, q, out, keep = SF.scored_fit()
    assert all("extr_gt" in fr and "extr" not in fr for fr in frames)
    ev = SF.check_camera_contract(frames, out, keep)
    print("camera quality", json.dumps(ev))


def test_scores_change_nothing_else():
    frames, q, out, keep = SF.scored_fit()
    plain, keep0 = SF.fit(frames, False, cfg=dict(FIT, traj_num=50), q=q)
    assert "recon" not in plain and "camera" not in plain and "recon_inputs" not in keep0
    SF.assert_same_fit(out, keep, plain, keep0)


def test_operator_path_gives_the_same_contracts():
    frames = clip(n_frames=4)
    out, keep = SF.fit(frames, True, fused=False)
    SF.check_recon_contract(frames, out, keep)
    SF.check_camera_contract(frames, out, keep)


def test_loaded_poses_are_the_recorded_poses():
    # frames that carry ``extr`` and load it, a fit without camera stages: the recorded path is the loaded one, and ``extr``
    # is the ground truth where there is no ``extr_gt``
    frames = []
    for fr in clip(n_frames=3):
        d = dict(fr)
        d["extr"] = d.pop("extr_gt")
        frames.append(d)
    out, keep = SF.fit(frames, True, cfg=dict(FIT, camera_first=False))
    gt = SF.clip_camera_gt(frames)
    np.testing.assert_allclose(out["camera"]["extr"], gt, rtol=0, atol=1e-6)
    assert out["camera"]["ATE"] <= 1e-5 and out["camera"]["RPE_t"] <= 1e-5


def test_concurrent_clips_take_both_scores():
    from gflow_amd.fit_video import fit_clips_concurrent
    clips = [clip(seed=0, n_frames=3), clip(seed=1, n_frames=3)]
    res = fit_clips_concurrent(clips, DEV, FIT, seeds=[0, 1], deterministic=True, recon=True, camera=True)
    for ci, r in enumerate(res):
        lone, _ = SF.fit(clips[ci], True, seed=ci)
        for k in ("sse", "ssim_sum", "PSNR", "SSIM"):
            np.testing.assert_array_equal(r["recon"][k], lone["recon"][k])
        np.testing.assert_array_equal(r["camera"]["extr"], lone["camera"]["extr"])
        for k in ("ATE", "RPE_t", "RPE_r"):
            assert r["camera"][k] == lone["camera"][k], k


def test_cli_blocks_and_csv_equal_the_clips_results(tmp_path):
    from gflow_amd import quality as QL
    from gflow_amd import synthetic as S
    from gflow_amd.fit_video import fit_clip, upload_clip
    n = 3
    csv = tmp_path / "metrics.csv"
    args = ["--clips", "2", "--frames", str(n), "--height", str(H), "--width", str(W), "--recon", "--camera", "--no-load-extr",
            "--deterministic", "--num_points", "1500", "--iterations_first", "60", "--iterations_after", "40",
            "--iterations_camera", "20", "--metrics-csv", str(csv)]
    r = subprocess.run([sys.executable, "-m", "gflow_amd.fit_video", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    cfg = dict(num_points=1500, iterations_first=60, iterations_after=40, iterations_camera=20)
    recs, cams = [], []
    for ci in range(2):
        out = fit_clip(upload_clip(S.make_clip(n, H, W, seed=ci, device=DEV), DEV), DEV, cfg, seed=ci, deterministic=True,
                       load_extr=False, recon=True, camera=True)
        recs.append(QL.evaluate(out["recon"]))
        cams.append(out["camera"])
    rc, cm = line["recon"], line["camera"]
    assert sorted(rc) == ["PSNR", "SSIM", "clips", "frames"]
    assert sorted(cm) == ["ATE", "RPE_r", "RPE_t", "clips", "clips_unscored"]
    assert rc["clips"] == 2 and rc["frames"] == 2 * n and cm["clips"] == 2 and cm["clips_unscored"] == 0
    for k in ("PSNR", "SSIM"):
        assert rc[k] == (recs[0][k] + recs[1][k]) / 2, k
    for k in ("ATE", "RPE_t", "RPE_r"):
        assert cm[k] == (cams[0][k] + cams[1][k]) / 2, k
    rows = [ln.split(",") for ln in csv.read_text().splitlines()]
    assert [k for k, _ in rows] == ["PSNR", "SSIM", "ATE", "RPE_t", "RPE_r"]
    assert [float(v) for _, v in rows] == [rc["PSNR"], rc["SSIM"], cm["ATE"], cm["RPE_t"], cm["RPE_r"]]
