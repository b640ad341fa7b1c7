"""What the GPU tests of the clip fit's scores share.  The small clip they fit -- ``FIT``'s settings on 96 x 128 synthetic
frames (``clip``) and its first-visible queries (``queries``).  For tests/test_gpu_recon.py and tests/test_gpu_camera.py ONE
deterministic 8-frame fit of it with ``recon=True, camera=True`` (trajectories and tracked queries on), computed on first
use and left unchanged, and the two contracts a fit's ``out["recon"]`` and ``out["camera"]`` hold."""
import functools

import numpy as np
import pytest
import torch

from tests import camera_ref as CR
from tests import quality_ref as QR

DEV = "cuda"
FIT = dict(num_points=1500, iterations_first=60, iterations_after=40, iterations_camera=20, densify_interval=30,
           densify_times=1, densify_interval_after=20, densify_times_after=1, lambda_depth=1e-2)
H, W, T = 96, 128, 8
# float64 on both sides over at most 1.3 M terms (n 2^-53 ~ 1.4e-10)
SSE_REL, SSE_ABS_AT_ZERO, SSIM_ABS = 1e-9, 1e-12, 1e-9
PSNR_DB = 1e-2                    # the bound the project already uses between its float32 PSNR sum and float64
CAMERA_REL = 1e-6                 # the optimiser's stopping accuracy (tests/camera_ref.py)


def clip(seed=0, n_frames=T, load_gt_pose=False):
    """``load_gt_pose``: every frame carries its ground-truth camera as ``extr``, which the fit then loads"""
    from gflow_amd import synthetic as S
    frames = S.make_clip(n_frames, H, W, seed=seed)
    if load_gt_pose:
        for fr in frames:
            fr["extr"] = fr["extr_gt"]
    return frames


def queries(n_frames=T, n=48, seed=0):
    """(the clip's ground-truth tracks of ``n`` points, their first-visible queries)"""
    from gflow_amd import synthetic as S
    from gflow_amd import tracking as TK
    g = S.make_clip_tracks(n_frames, H, W, seed=seed, n_queries=n, query_seed=0)
    return g, TK.first_visible_queries(g["points"].astype(np.float32), g["occluded"], H, W)


def fit(frames, on, fused=True, cfg=FIT, seed=0, q=None, **kw):
    from gflow_amd.fit_video import fit_clip
    keep = {"record_recon_inputs": True} if on else {}
    out = fit_clip(frames, DEV, cfg, seed=seed, fused=fused, deterministic=True if fused else None, track_queries=q,
                   recon=on, camera=on, keep=keep, **kw)
    return out, keep


@functools.lru_cache(maxsize=None)
def scored_fit():
    """(frames, queries, out, keep) of the shared fit"""
    frames = clip()
    _, q = queries()
    out, keep = fit(frames, True, cfg=dict(FIT, traj_num=50), q=q)
    return frames, q, out, keep


def assert_sums(got_sse, got_ssim_sum, want_sse, want_ssim_sum, h, w, what=""):
    count = 3 * (h - 10) * (w - 10)
    print(f"{what} {h}x{w}: sse {got_sse!r} / {want_sse!r}, ssim {got_ssim_sum / count!r} / {want_ssim_sum / count!r}")
    if want_sse == 0.0:
        assert abs(got_sse) <= SSE_ABS_AT_ZERO, what
    else:
        assert abs(got_sse - want_sse) <= SSE_REL * want_sse, what
    assert abs(got_ssim_sum / count - want_ssim_sum / count) <= SSIM_ABS, what


def check_recon_contract(frames, out, keep):
    from gflow_amd import quality as QL
    rec, n = out["recon"], len(frames)
    assert sorted(rec) == ["PSNR", "SSIM", "sse", "ssim_sum"]
    for k in rec:
        assert rec[k].shape == (n,) and rec[k].dtype == np.float64, k
    inputs = keep["recon_inputs"]
    assert len(inputs) == n == len(keep["psnr"])
    h, w = frames[0]["image"].shape[:2]
    for t in range(n):
        assert tuple(inputs[t].shape) == (3, h, w)
        sse, ssim_sum = QR.sums(QR.bytes_of(inputs[t]), frames[t]["image"].cpu().numpy())
        assert_sums(rec["sse"][t], rec["ssim_sum"][t], sse, ssim_sum, h, w, f"frame {t}")
        assert rec["PSNR"][t] == QR.psnr(rec["sse"][t], h, w) and rec["SSIM"][t] == QR.ssim(rec["ssim_sum"][t], h, w)
        assert abs(rec["PSNR"][t] - float(keep["psnr"][t])) <= PSNR_DB, t
        assert 0.0 < rec["SSIM"][t] <= 1.0
    ev = QL.evaluate(rec)
    assert ev == {"PSNR": float(np.mean(rec["PSNR"])), "SSIM": float(np.mean(rec["SSIM"])), "frames": n}
    return ev


def clip_camera_gt(frames):
    return np.stack([(fr["extr_gt"] if fr.get("extr_gt") is not None else fr["extr"]).cpu().double().numpy() for fr in frames])


def check_camera_contract(frames, out, keep):
    from gflow_amd import camera as CM
    cam, n = out["camera"], len(frames)
    assert sorted(cam) == ["ATE", "RPE_r", "RPE_t", "extr"]
    assert cam["extr"].shape == (n, 3, 4) and cam["extr"].dtype == np.float32
    np.testing.assert_array_equal(cam["extr"][-1], keep["trainer"].get_extr().detach().cpu().numpy())
    gt = clip_camera_gt(frames)
    here = CM.evaluate(cam["extr"], gt)
    direct = CR.evaluate(cam["extr"], gt)
    print("camera", {k: cam[k] for k in CM.SCORE_KEYS}, "direct minimisation", direct)
    for k in CM.SCORE_KEYS:
        assert cam[k] is not None and np.isfinite(cam[k]) and cam[k] >= 0.0, k
        assert cam[k] == here[k], k
        assert cam[k] == pytest.approx(direct[k], rel=CAMERA_REL), k
    return {k: cam[k] for k in CM.SCORE_KEYS}


def assert_same_fit(out, keep, plain, keep0):
    """everything tests/test_gpu_seg.py::test_segment_changes_nothing_else compares"""
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
