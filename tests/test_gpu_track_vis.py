"""GPU: gfl_track_vis / gflow_amd.track_vis.draw_tracks byte for byte against the painter's restatement of the drawing rule
(tests/track_vis_ref.py), the overflow contract, and fit_clip(track_vis=True)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import score_fit as SF
from tests import track_vis_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def draw(video, tracks, occ, **kw):
    from gflow_amd.track_vis import draw_tracks
    out = draw_tracks(torch.from_numpy(video).to(DEV), torch.from_numpy(np.asarray(tracks, dtype=np.float32)).to(DEV),
                      torch.from_numpy(np.asarray(occ)).to(DEV), **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == video.shape
    return out.cpu().numpy()


def raw_call(video, tracks, occ, K_cap, still_length=0):
    """the library call itself: (out, overflow[0])"""
    from gflow_amd import _lib as L
    from gflow_amd import color
    lib = L.load()
    T, H, W = video.shape[:3]
    N = tracks.shape[1]
    v = torch.from_numpy(video).to(DEV)
    tr = torch.from_numpy(np.ascontiguousarray(tracks, dtype=np.float32)).to(DEV)
    oc = torch.from_numpy(np.ascontiguousarray(occ).astype(np.uint8)).to(DEV)
    out = torch.full_like(v, 77)
    ovf = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    ws = L.scratch(lib.gfl_track_vis_workspace_bytes(T, N, W, H, K_cap), v.device)
    L.check(lib.gfl_track_vis(L.ptr(v), L.ptr(tr), L.ptr(oc), T, N, W, H, still_length, L.ptr(color.lut("gist_rainbow", v.device)),
                              K_cap, L.ptr(out), L.ptr(ovf), L.ptr(ws), ws.numel(), L.stream()), "track vis")
    return out.cpu().numpy(), int(ovf.item())


def noise_video(T, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, H, W, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the hand-built scene
HB_H, HB_W, HB_T, HB_N = 40, 72, 5, 8


def hand_built():
    """40 x 72 (no multiple of 16), five frames, eight tracks"""
    nan = float("nan")
    tr = np.zeros((HB_T, HB_N, 2), dtype=np.float32)
    # 0: x == 0 in frame 2 (truncated from 0.3): neither a marker there nor the segment that STARTS there
    tr[:, 0] = [[10.2, 5.5], [6.7, 9.1], [0.3, 12.0], [5.0, 15.9], [9.9, 19.0]]
    # 1: -0.6 truncates to 0 (frame 1, y): inside the image, but hidden by the zero rule
    tr[:, 1] = [[20.0, 1.0], [24.5, -0.6], [28.0, 4.2], [31.0, 8.0], [35.5, 6.0]]
    # 2: leaves the image at x >= W (frame 1), comes back, then a NaN (frame 3)
    tr[:, 2] = [[66.0, 30.0], [72.0, 31.0], [70.9, 33.0], [nan, 34.0], [60.0, 38.9]]
    # 3: corner to corner, every frame: one segment across every tile row and column
    tr[:, 3] = [[2.0, 2.0], [70.0, 38.0], [2.0, 38.0], [70.0, 2.0], [3.0, 37.0]]
    # 4 and 5: the same pixels from different floats: the later paint (5) decides; they also cross track 3's diagonals
    tr[:, 4] = [[30.1, 30.2], [36.3, 26.4], [42.5, 22.6], [48.7, 18.8], [54.9, 14.1]]
    tr[:, 5] = [[30.9, 30.8], [36.7, 26.6], [42.1, 22.2], [48.2, 18.1], [54.3, 14.7]]
    # 6: static: zero-length segments
    tr[:, 6] = [[50.2, 33.7]] * HB_T
    # 7: an ordinary walk along the right border and the bottom rows
    tr[:, 7] = [[71.9, 10.0], [68.0, 16.5], [64.2, 39.9], [58.0, 39.0], [52.0, 36.0]]
    occ = np.zeros((HB_T, HB_N), dtype=bool)
    occ[1::2, ::2] = True
    occ[::2, 1::3] = True
    occ[:, 6] = [False, True, False, True, True]
    return noise_video(HB_T, HB_H, HB_W, 0), tr, occ


@pytest.mark.parametrize("still_length", [0, 3, 8])
def test_hand_built_scene_equals_the_painter(still_length):
    video, tr, occ = hand_built()
    want = TR.paint(video, tr, occ, still_length)
    got = draw(video, tr, occ, still_length=still_length)
    np.testing.assert_array_equal(got, want)
    # what the scene is there for
    pts = TR.int_coords(tr)
    assert pts[2, 0, 0] == 0 and pts[1, 1, 1] == 0 and pts[1, 2, 0] >= HB_W and pts[3, 2, 0] < 0
    assert (pts[:, 4] == pts[:, 5]).all()
    assert (want != video).any()
    if still_length == 3:
        assert (want != TR.paint(video, tr, occ, 0)).any()           # (the moving tracks' own colour range shows)


def test_hand_built_scene_from_host_tensors_and_a_float_video():
    from gflow_amd.render import render2img_device
    from gflow_amd.track_vis import draw_tracks
    video, tr, occ = hand_built()
    want = TR.paint(video, tr, occ, 3)
    got = draw_tracks(video, tr, occ, still_length=3)                # numpy arrays on the host
    assert got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    chw = torch.rand(HB_T, 3, HB_H, HB_W, generator=torch.Generator().manual_seed(0)) * 1.2 - 0.1
    as_u8 = torch.stack([render2img_device(f) for f in chw]).numpy()
    got = draw_tracks(chw.to(DEV), torch.from_numpy(tr), torch.from_numpy(occ), still_length=3)
    np.testing.assert_array_equal(got.cpu().numpy(), TR.paint(as_u8, tr, occ, 3))


def test_one_frame_one_track():
    video = noise_video(1, HB_H, HB_W, 1)
    for occluded in (False, True):
        tr, occ = np.array([[[17.5, 16.2]]], dtype=np.float32), np.array([[occluded]])
        want = TR.paint(video, tr, occ)
        assert (want != video).any()
        np.testing.assert_array_equal(draw(video, tr, occ), want)


def test_no_tracks_copies_the_video():
    video = noise_video(3, HB_H, HB_W, 2)
    got = draw(video, np.zeros((3, 0, 2), dtype=np.float32), np.zeros((3, 0), dtype=bool))
    np.testing.assert_array_equal(got, video)
    from gflow_amd.track_vis import draw_tracks
    empty = draw_tracks(torch.zeros(0, HB_H, HB_W, 3, dtype=torch.uint8, device=DEV), torch.zeros(0, 4, 2), torch.zeros(0, 4))
    assert tuple(empty.shape) == (0, HB_H, HB_W, 3)


# ------------------------------------------------------------------------------------------------------ random walks
RW_H, RW_W, RW_T, RW_N = 96, 128, 12, 300


@functools.lru_cache(maxsize=None)
def random_walks():
    """300 walks of at most 6 px a step; half of them start inside one 20 x 20 patch, so that the tiles around it hold lists
    several staging rounds long.  (video, tracks, occluded, the painter's picture, pairs per tile)"""
    rng = np.random.default_rng(7)
    start = np.concatenate([rng.uniform([54, 38], [74, 58], (RW_N // 2, 2)),
                            rng.uniform([1, 1], [RW_W - 1, RW_H - 1], (RW_N - RW_N // 2, 2))])
    rng.shuffle(start)
    steps = rng.uniform(-6, 6, (RW_T, RW_N, 2))
    steps[0] = 0
    tr = (start[None] + np.cumsum(steps, axis=0)).astype(np.float32)
    occ = rng.random((RW_T, RW_N)) < 0.3
    video = noise_video(RW_T, RW_H, RW_W, 3)
    return video, tr, occ, TR.paint(video, tr, occ, 120), TR.pairs_per_tile(tr, RW_W, RW_H)


def test_random_walks_with_lists_longer_than_a_staging_round():
    from gflow_amd.track_vis import STAGE
    video, tr, occ, want, pairs = random_walks()
    assert pairs.max() > 2 * STAGE and RW_N > STAGE, pairs.max()
    assert np.abs(np.diff(tr, axis=0)).max() <= 6.0 + 1e-4
    got = draw(video, tr, occ, still_length=120)
    np.testing.assert_array_equal(got, want)
    again = draw(video, tr, occ, still_length=120)
    np.testing.assert_array_equal(again, got)                        # (the lists' fill order never shows)


def test_a_pool_too_small_leaves_the_markers_only_and_draw_tracks_raises():
    from gflow_amd.track_vis import draw_tracks
    video, tr, occ, want, pairs = random_walks()
    need = int(pairs.sum())
    out, flag = raw_call(video, tr, occ, need, still_length=120)     # exactly enough room
    assert flag == 0
    np.testing.assert_array_equal(out, want)
    markers_only = TR.paint(video, tr, occ, 120, traces=False)
    assert (markers_only != want).any()
    for k_cap in (need - 1, 1):
        out, flag = raw_call(video, tr, occ, k_cap, still_length=120)
        assert flag == 1
        np.testing.assert_array_equal(out, markers_only)
    with pytest.raises(RuntimeError, match="K_cap"):
        draw_tracks(video, tr, occ, still_length=120, K_cap=need - 1)
    np.testing.assert_array_equal(draw(video, tr, occ, still_length=120, K_cap=need), want)


# ------------------------------------------------------------------------------------------------------- through a fit
def occlusions_like_process_occu(masks, uv):
    T, H, W = masks.shape
    out = np.zeros(uv.shape[:2], dtype=bool)
    at = lambda t, j: masks[t][round(float(min(max(uv[t, j, 1], 0), H - 1))), round(float(min(max(uv[t, j, 0], 0), W - 1)))]
    for j in range(uv.shape[1]):
        moving = bool(at(0, j))
        for t in range(T):
            out[t, j] = (not moving) and bool(at(t, j))
    return out


def test_fit_clip_track_vis_changes_nothing_else_and_equals_the_painter():
    from gflow_amd.render import render2img_device
    n = 4
    frames = SF.clip(n_frames=n)
    _, q = SF.queries(n_frames=n)
    cfg = dict(SF.FIT, traj_num=50)
    plain, keep0 = SF.fit(frames, True, cfg=cfg, q=q)
    out, keep = SF.fit(frames, True, cfg=cfg, q=q, track_vis=True)
    assert "track_vis" not in plain and "track_vis_inputs" not in keep0
    SF.assert_same_fit(out, keep, plain, keep0)
    assert out["rasterisations"] == plain["rasterisations"]
    vis, inputs = out["track_vis"], keep["track_vis_inputs"]
    video, masks = inputs["video"], inputs["masks"]
    assert video.shape == (n, SF.H, SF.W, 3) and video.dtype == np.uint8 and masks.shape == (n, SF.H, SF.W)
    for t in range(n):                                               # the renders the frames' PSNR was taken from
        np.testing.assert_array_equal(video[t], render2img_device(keep["recon_inputs"][t]).cpu().numpy())
    uv, split = out["traj"]["uv"], out["traj"]["split_interval"]
    occ = occlusions_like_process_occu(masks, uv)
    s = uv.shape[1] if split is None else split
    want = {"pred": TR.paint(video, out["tracks"]["tracks"].transpose(1, 0, 2), out["tracks"]["occluded"].T),
            "seeds": TR.paint(video, uv, occ, s), "seeds_still": TR.paint(video, uv[:, :s], occ[:, :s])}
    if s < uv.shape[1]:
        want["seeds_move"] = TR.paint(video, uv[:, s:], occ[:, s:])
    assert sorted(vis) == sorted(want)
    for k in want:
        assert vis[k].dtype == np.uint8 and (vis[k] != video).any(), k
        np.testing.assert_array_equal(vis[k], want[k], err_msg=k)


def test_track_vis_needs_tracks_on_the_device_too():
    from gflow_amd.fit_video import fit_clip
    with pytest.raises(ValueError, match="track_vis"):
        fit_clip(SF.clip(n_frames=1), DEV, SF.FIT, track_vis=True)


def test_concurrent_fits_hand_the_option_through():
    from gflow_amd.fit_video import fit_clip, fit_clips_concurrent
    n = 2
    clips = [SF.clip(seed=s, n_frames=n) for s in (0, 1)]
    _, q = SF.queries(n_frames=n, n=12)
    extra = dict(mine=(np.full((n, 3, 2), 20.5, dtype=np.float32), np.zeros((n, 3), dtype=bool)))
    both = fit_clips_concurrent(clips, DEV, SF.FIT, deterministic=True, track_queries=[q, q], track_vis=[True, extra])
    for ci, opt in enumerate((True, extra)):
        alone = fit_clip(clips[ci], DEV, SF.FIT, seed=ci, deterministic=True, track_queries=q, track_vis=opt)
        assert sorted(both[ci]["track_vis"]) == (["mine", "pred"] if ci else ["pred"])
        for k, img in alone["track_vis"].items():
            np.testing.assert_array_equal(both[ci]["track_vis"][k], img, err_msg=f"clip {ci} {k}")
    with pytest.raises(ValueError, match="one entry per clip"):
        fit_clips_concurrent(clips, DEV, SF.FIT, track_queries=[q, q], track_vis=[True])


def test_cli_writes_one_folder_of_frames_per_overlay(tmp_path):
    from PIL import Image
    from gflow_amd import fit_video
    n = 2
    fit_video.main(["--clips", "1", "--frames", str(n), "--height", str(SF.H), "--width", str(SF.W), "--num_points", "1500",
                    "--iterations_first", "40", "--iterations_after", "20", "--iterations_camera", "10", "--track",
                    "--traj-num", "50", "--track-vis", str(tmp_path / "vis")])
    root = tmp_path / "vis" / "clip_0"
    names = sorted(os.listdir(root))
    assert set(names) >= {"gt", "pred", "seeds", "seeds_still"} and set(names) <= {"gt", "pred", "seeds", "seeds_still", "seeds_move"}
    for name in names:
        assert sorted(os.listdir(root / name)) == [f"{t:05d}.png" for t in range(n)]
        assert np.asarray(Image.open(root / name / "00001.png")).shape == (SF.H, SF.W, 3)
