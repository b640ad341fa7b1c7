"""Moving-region segmentation on the device (``-m gpu``; gfl_seg_score, gflow_amd/segmentation.py): exact properties only
-- the kernel's six counts against the numpy restatement (tests/seg_ref.py, itself held against the reference's J and F in
test_seg_host.py), fits with ``segment=True`` against the hull and the restatement run on the inputs they recorded, and a
fit with the feature against the same fit without it, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import seg_ref as R
from tests.score_fit import FIT, H, W, clip, queries

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "davis_seg.npz")
GARBAGE = 0x5EEDBEEF


def _score(pred, gt, radius, valid=None):
    """gfl_seg_score through the C ABI on (T, H, W) arrays; the output buffer is pre-filled with garbage.
    Returns (status, counts (T, 6) int64)."""
    from gflow_amd import _lib as L
    pred, gt = np.asarray(pred), np.asarray(gt)
    n, h, w = pred.shape
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.uint8) * np.uint8(255)).to(DEV)
    g = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(DEV)                  # (255 and 1: nonzero is foreground)
    v = None if valid is None else torch.tensor(valid, dtype=torch.uint8, device=DEV)
    counts = torch.full((max(n, 1), 6), GARBAGE, dtype=torch.int32, device=DEV)
    rc = L.load().gfl_seg_score(L.ptr(p), L.ptr(g), L.ptr(v), n, h, w, int(radius), L.ptr(counts), L.stream())
    torch.cuda.synchronize()
    return rc, counts[:n].cpu().numpy().view(np.uint32).astype(np.int64)


def _noise(rng, n, h, w, density=0.5):
    """blobs with holes: a smooth shape XOR sparse noise, so that boundaries are dense and both sides differ"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        m = (xx - cx) ** 2 / max(w / 3, 1) ** 2 + (yy - cy) ** 2 / max(h / 3, 1) ** 2 <= 1
        out.append(m ^ (rng.random((h, w)) < density * 0.1))
    return np.stack(out)


def test_counts_equal_the_restatement_on_every_golden_case():
    from gflow_amd import segmentation as SG
    gold = np.load(GOLD)
    n = int(gold["n_cases"])
    assert n == 12
    for i in range(n):
        pred, gt = gold[f"c{i}_pred"], gold[f"c{i}_gt"]
        radius = SG.bound_pix(*pred.shape, float(gold[f"c{i}_bound_th"]))
        rc, got = _score(pred[None], gt[None], radius)
        assert rc == 0
        np.testing.assert_array_equal(got[0], R.counts(pred, gt, radius), err_msg=str(gold["names"][i]))
        # and through the module: the reference's J and F from the device's counts
        c = SG.seg_counts(torch.from_numpy(pred.astype(np.uint8)).to(DEV)[None], torch.from_numpy(gt.astype(np.uint8)).to(DEV)[None],
                          radius)
        J, F, _ = SG.scores_from_counts(c)
        assert J[0] == float(gold[f"c{i}_J"]) and F[0] == float(gold[f"c{i}_F"]), str(gold["names"][i])


def test_counts_with_a_disc_larger_than_the_image():
    gold = np.load(GOLD)
    i = [str(s) for s in gold["names"]].index("70x130_th8")
    pred, gt = gold[f"c{i}_pred"], gold[f"c{i}_gt"]
    rc, got = _score(pred[None], gt[None], 64)
    assert rc == 0
    want = R.counts(pred, gt, 64)
    np.testing.assert_array_equal(got[0], want)
    assert want[4] == want[2] and want[5] == want[3]            # (every boundary pixel has a partner within 64 px here)


# widths on both sides of a 64-bit word edge, one and two rows, halos that cross tile edges in both directions (tiles are
# 64 x 32) and leave the image, more than one tile in both directions
@pytest.mark.parametrize("h,w,radius", [(1, 64, 1), (1, 65, 3), (2, 63, 2), (2, 130, 64), (33, 129, 7), (65, 63, 33),
                                        (40, 200, 12), (97, 70, 64)])
def test_counts_on_noisy_masks(h, w, radius):
    rng = np.random.default_rng(h * 1000 + w)
    pred, gt = _noise(rng, 2, h, w), _noise(rng, 2, h, w)
    rc, got = _score(pred, gt, radius)
    assert rc == 0
    want = R.counts_stack(pred, gt, radius)
    np.testing.assert_array_equal(got, want)
    assert want[:, 1].all()


def test_invalid_frames_stay_zero_and_the_call_writes():
    rng = np.random.default_rng(3)
    pred, gt = _noise(rng, 3, 37, 53), _noise(rng, 3, 37, 53)
    valid = [1, 0, 1]
    rc, got = _score(pred, gt, 3, valid)
    assert rc == 0
    want = R.counts_stack(pred, gt, 3, valid)
    np.testing.assert_array_equal(got, want)
    assert not got[1].any() and got[0].all() and got[2].all()
    # (every call starts from a buffer full of garbage: the counts are written, not accumulated)
    rc, again = _score(pred, gt, 3, valid)
    np.testing.assert_array_equal(again, want)


def test_counts_at_480p():
    rng = np.random.default_rng(480854)
    pred, gt = _noise(rng, 4, 480, 854, density=0.05), _noise(rng, 4, 480, 854, density=0.05)
    rc, got = _score(pred, gt, 8)
    assert rc == 0
    np.testing.assert_array_equal(got, R.counts_stack(pred, gt, 8))


def test_argument_errors():
    from gflow_amd import _lib as L
    z = np.zeros((1, 4, 4), bool)
    inv = L.load().gfl_status_string(-1)
    for radius in (0, 65, -1):
        rc, got = _score(z, z, radius)
        assert rc == -1 and L.load().gfl_status_string(rc) == inv
        assert (got == np.uint32(GARBAGE)).all()                # nothing written
    rc, _ = _score(np.zeros((0, 4, 4), bool), np.zeros((0, 4, 4), bool), 8)
    assert rc == 0


# ------------------------------------------------------------------------------------------------------------- fits
def _fit(frames, segment, fused=True, cfg=FIT, seed=0, q=None):
    from gflow_amd.fit_video import fit_clip
    keep = {"record_seg_inputs": True}
    out = fit_clip(frames, DEV, cfg, seed=seed, fused=fused, deterministic=True if fused else None, track_queries=q,
                   segment=segment, keep=keep)
    return out, keep


@pytest.fixture(scope="module")
def seg_fit():
    frames = clip()
    _, q = queries()
    out, keep = _fit(frames, True, cfg=dict(FIT, traj_num=50), q=q)
    return frames, q, out, keep


def _check_contract(frames, out, keep):
    from gflow_amd import segmentation as SG
    from gflow_amd.hull import FastConcaveHull2D
    seg = out["segmentation"]
    n = len(frames)
    assert seg["masks"].shape == (n, H, W) and seg["masks"].dtype == np.uint8
    assert seg["valid"].shape == (n,) and seg["valid"].dtype == bool
    assert seg["counts"].shape == (n, 6) and seg["counts"].dtype == np.int64
    inputs = keep["seg_inputs"]
    assert len(inputs) == n and all(x is not None for x in inputs)
    last, hulls = None, 0
    for t, (uv, sel) in enumerate(inputs):
        pts = uv[sel].cpu().numpy()
        if pts.shape[0] > 5:
            last = (FastConcaveHull2D(pts).mask(W, H) * 255).astype(np.uint8)
            hulls += 1
        assert seg["valid"][t] == (last is not None)
        np.testing.assert_array_equal(seg["masks"][t], last if last is not None else np.zeros((H, W), np.uint8))
    assert hulls >= 1
    gt = np.stack([np.asarray(fr["move_mask"].cpu()) for fr in frames])
    radius = SG.bound_pix(H, W)
    assert radius == 2
    want = R.counts_stack(seg["masks"], gt, radius, seg["valid"])
    np.testing.assert_array_equal(seg["counts"], want)
    for t in range(n):
        j, f = R.scores(want[t]) if seg["valid"][t] else (0.0, 0.0)
        assert seg["J"][t] == j and seg["F"][t] == f and seg["JF"][t] == (j + f) / 2
        assert 0.0 <= j <= 1.0 and 0.0 <= f <= 1.0
    ev = SG.evaluate(seg)
    assert ev["frames_scored"] == int(seg["valid"].sum()) >= 1
    for k in ("J", "F", "J&F"):
        assert 0.0 <= ev[k] <= 1.0
    return ev


def test_fit_masks_and_scores_equal_the_restatement(seg_fit):
    frames, q, out, keep = seg_fit
    ev = _check_contract(frames, out, keep)
    print("segmentation quality", json.dumps(ev))


def test_first_mask_is_the_trajectory_seeds_mask(seg_fit):
    frames, q, out, keep = seg_fit
    tr = keep["trainer"]
    assert tr.move_seg is not None and out["segmentation"]["valid"][0]
    assert out["segmentation"]["masks"][0].tobytes() == np.ascontiguousarray(tr.move_seg).tobytes()


def test_segment_changes_nothing_else(seg_fit):
    frames, q, out, keep = seg_fit
    plain, keep0 = _fit(frames, False, cfg=dict(FIT, traj_num=50), q=q)
    assert "segmentation" not in plain and "seg_inputs" not in keep0 and keep0["trainer"].seg_recorder is None
    for k in ("psnr_sum", "frames", "iterations", "rasterisations", "splats_final", "void_iterations"):
        assert out[k] == plain[k], k
    ea, eb = keep["trainer"].engine, keep0["trainer"].engine
    assert ea.N == eb.N
    for k in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(ea, k)[:ea.N], getattr(eb, k)[:eb.N]), k
    for k in ("pose", "depth_ab", "render"):
        assert torch.equal(getattr(ea, k), getattr(eb, k)), k
    assert torch.equal(torch.stack([p.float() for p in keep["psnr"]]), torch.stack([p.float() for p in keep0["psnr"]]))
    for k in ("tracks", "occluded", "anchor", "shift"):
        np.testing.assert_array_equal(out["tracks"][k], plain["tracks"][k])
    np.testing.assert_array_equal(out["traj"]["images"], plain["traj"]["images"])
    np.testing.assert_array_equal(out["traj"]["uv"], plain["traj"]["uv"])


def test_operator_path_gives_the_same_contract():
    frames = clip(n_frames=4)
    out, keep = _fit(frames, True, fused=False)
    _check_contract(frames, out, keep)


def test_concurrent_clips_take_segment():
    from gflow_amd.fit_video import fit_clips_concurrent
    clips = [clip(seed=0, n_frames=3), clip(seed=1, n_frames=3)]
    res = fit_clips_concurrent(clips, DEV, FIT, seeds=[0, 1], deterministic=True, segment=True)
    for ci, r in enumerate(res):
        lone, _ = _fit(clips[ci], True, seed=ci)
        for k in ("masks", "valid", "counts", "J", "F", "JF"):
            np.testing.assert_array_equal(r["segmentation"][k], lone["segmentation"][k])


def test_cli_davis_block_equals_the_clips_results(tmp_path):
    from gflow_amd import segmentation as SG
    from gflow_amd import synthetic as S
    from gflow_amd.fit_video import fit_clip, upload_clip
    from PIL import Image
    n = 3
    args = ["--clips", "2", "--frames", str(n), "--height", str(H), "--width", str(W), "--seg", "--deterministic",
            "--num_points", "1500", "--iterations_first", "60", "--iterations_after", "40", "--iterations_camera", "20",
            "--seg-out", str(tmp_path / "out")]
    r = subprocess.run([sys.executable, "-m", "gflow_amd.fit_video", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    cfg = dict(num_points=1500, iterations_first=60, iterations_after=40, iterations_camera=20)
    evs, frames_scored = [], 0
    for ci in range(2):
        out = fit_clip(upload_clip(S.make_clip(n, H, W, seed=ci, device=DEV), DEV), DEV, cfg, seed=ci, deterministic=True, segment=True)
        seg = out["segmentation"]
        ev = SG.evaluate(seg)
        assert ev["frames_scored"] >= 1
        evs.append(ev)
        frames_scored += ev["frames_scored"]
        files = sorted(os.listdir(tmp_path / "out" / f"clip_{ci}"))
        assert files == [f"move_mask_{t:05d}.png" for t in range(n) if seg["valid"][t]]
        for t in range(n):
            if seg["valid"][t]:
                png = np.asarray(Image.open(tmp_path / "out" / f"clip_{ci}" / f"move_mask_{t:05d}.png"))
                np.testing.assert_array_equal(png, seg["masks"][t])
    dv = line["davis"]
    assert sorted(dv) == ["F", "J", "J&F", "clips", "frames_scored"]
    assert dv["clips"] == 2 and dv["frames_scored"] == frames_scored
    for k in ("J", "F", "J&F"):
        assert dv[k] == (evs[0][k] + evs[1][k]) / 2, k
