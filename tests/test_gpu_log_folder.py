"""GPU: a clip fit saved as the reference's log folder (fit_clip(save=DIR), gflow_amd.log_folder; fit_video --out).
The small clip and config of tests/score_fit.py, four frames, deterministic; ONE saved fit shared by the tests."""
import io
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from tests import score_fit as SF

pytestmark = pytest.mark.gpu

DEV = SF.DEV
N = 4
CFG = dict(SF.FIT, traj_num=50)


def _fit(save=None):
    from gflow_amd.fit_video import fit_clip
    keep = {}
    out = fit_clip(SF.clip(n_frames=N), DEV, CFG, seed=0, deterministic=True, segment=True, keep=keep, save=save)
    return out, keep


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """(folder, out, keep) of the saved fit: computed once, never written to"""
    folder = str(tmp_path_factory.mktemp("log") / "clip")
    out, keep = _fit(save=folder)
    return folder, out, keep


def _png(path):
    return np.asarray(Image.open(path))


def _files(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder).replace(os.sep, "/") for d, _, fs in os.walk(folder) for f in fs)


def test_file_set_is_the_references(saved):
    from gflow_amd import log_folder as LF
    folder, out, _ = saved
    names = LF.frame_names(SF.clip(n_frames=N))
    assert names == [f"{t:05d}" for t in range(N)] and out["saved"] == folder
    valid = out["segmentation"]["valid"]
    assert valid.any()
    want = LF.expected_files(names, valid, traj=True)
    assert len(want) == N + 7 * N + int(valid.sum()) + 8 + 3
    assert _files(folder) == want
    for kind in ("img", "img_center", "img_depth", "img_still", "img_still_center", "img_move", "img_move_center"):
        im = Image.open(os.path.join(folder, "images", f"{kind}_{names[-1]}.png"))
        assert im.size == (SF.W, SF.H) and im.mode == "RGB"
    assert _png(os.path.join(folder, "images", f"img_still_{names[-1]}.png")).max() > 0


def test_checkpoints_load_and_the_last_is_the_trainers_state(saved):
    from gflow_amd.trainer import SimpleGaussian
    folder, _, keep = saved
    tr = keep["trainer"]
    f0 = SF.clip(n_frames=1)[0]
    other = SimpleGaussian(f0["image"], f0["depth"], num_points=CFG["num_points"], device=DEV, seed=1)
    paths = sorted(os.listdir(os.path.join(folder, "ckpt")))
    assert paths == [f"{t:05d}.tar" for t in range(N)]
    for p in paths:
        ck = torch.load(os.path.join(folder, "ckpt", p), map_location="cpu", weights_only=False)
        assert sorted(ck) == ["attributes", "extr", "height", "intr", "last_uv", "move_seg", "still_mask", "width"]
        assert (ck["width"], ck["height"]) == (SF.W, SF.H)
        other.load_checkpoint(os.path.join(folder, "ckpt", p))
        n = ck["attributes"]["xyz"].shape[0]
        assert other.current_pts_num() == n and ck["still_mask"].shape[0] == n and ck["last_uv"].shape[1] == 2
        # (load_camera turns the matrix into the trainer's pose and get_extr back: float32 rounding of a rotation)
        assert torch.allclose(other.get_extr().detach().cpu(), ck["extr"], atol=1e-5)
    for k, v in tr._attributes.items():
        assert torch.equal(ck["attributes"][k], v.detach().cpu()), k
    assert torch.equal(ck["extr"], tr.get_extr().detach().cpu())
    assert torch.equal(ck["still_mask"], tr.still_mask.cpu()) and torch.equal(ck["intr"], tr.intr.cpu())


def test_last_image_is_the_final_states_render(saved):
    folder, _, keep = saved
    tr = keep["trainer"]
    with torch.no_grad():
        scene = tr.second.scene_u8(tr.engine, tr.bg).cpu().numpy()
    for k, kind in enumerate(("img", "img_depth", "img_center")):
        assert np.array_equal(_png(os.path.join(folder, "images", f"{kind}_{N - 1:05d}.png")), scene[k]), kind
    assert len(set(scene[0].reshape(-1).tolist())) > 30


def test_masks_videos_and_trajectories(saved):
    from gflow_amd import video
    folder, out, _ = saved
    seg = out["segmentation"]
    for t in range(N):
        path = os.path.join(folder, "images_seg", f"move_mask_{t:05d}.png")
        assert os.path.exists(path) == bool(seg["valid"][t])
        if seg["valid"][t]:
            im = Image.open(path)
            assert im.mode == "L" and np.array_equal(np.asarray(im), seg["masks"][t])
    for name in ("sequence", "sequence_center", "sequence_depth", "sequence_still", "sequence_still_center", "sequence_move",
                 "sequence_move_center", "sequence_move_seg", "sequence_traj", "sequence_traj_upon"):
        got = video.read_avi(os.path.join(folder, name + ".avi"))
        assert len(got["frames"]) == N and got["fps"] == 5.0 and (got["width"], got["height"]) == (SF.W, SF.H), name
    # sequence.avi is the device's JPEG of the saved images
    pngs = np.stack([_png(os.path.join(folder, "images", f"img_{t:05d}.png")) for t in range(N)])
    assert video.read_avi(os.path.join(folder, "sequence.avi"))["frames"] == video.encode_jpeg(pngs, quality=90)
    with open(os.path.join(folder, "sequence_traj.pkl"), "rb") as f:
        traj = pickle.load(f)
    assert len(traj) == N and all(np.array_equal(a, b) for a, b in zip(traj, out["traj"]["uv"]))


def test_viewer_opens_the_folder(saved):
    from gflow_amd import viewer as V
    folder, _, _ = saved
    session = V.ViewerSession(folder, DEV, bg=0.0)
    assert len(session) == N and (session.W, session.H) == (SF.W, SF.H)
    img = session.frame(0)
    assert img.shape == (SF.H, SF.W, 3) and img.dtype == torch.uint8
    d = np.abs(img.cpu().numpy().astype(np.int32) - _png(os.path.join(folder, "images", "img_00000.png")).astype(np.int32))
    share = float((d != 0).mean())
    print(f"viewer frame 0 against img_00000.png: {share:.2e} of the bytes differ (allowed 3.0e-04), max {int(d.max())} level(s)")
    # the tolerance tests/test_gpu_render_batch.py holds the batched rasteriser to
    assert int(d.max()) <= 1 and share <= 3e-4
    assert bool(session.labels.any()) and not bool(session.labels.all())          # the layers come from the saved still_mask


def test_saving_reads_and_never_steps(saved):
    _, out, keep = saved
    plain, keep0 = _fit()
    assert "saved" not in plain
    assert out["psnr_sum"] == plain["psnr_sum"] and out["iterations"] == plain["iterations"]
    assert out["splats_final"] == plain["splats_final"]
    assert out["rasterisations"] == plain["rasterisations"] + 2 * N              # the two layer forwards of every frame
    a, b = keep["trainer"], keep0["trainer"]
    for k in a._attributes:
        assert torch.equal(a._attributes[k], b._attributes[k]), k
    assert torch.equal(a.get_extr(), b.get_extr())
    np.testing.assert_array_equal(out["segmentation"]["masks"], plain["segmentation"]["masks"])
    np.testing.assert_array_equal(out["traj"]["images"], plain["traj"]["images"])


def test_save_refuses_before_anything_is_fitted(tmp_path):
    from gflow_amd.fit_video import ClipFit
    frames = SF.clip(n_frames=2)
    with pytest.raises(ValueError, match="fused"):
        ClipFit(frames, DEV, SF.FIT, fused=False, save=str(tmp_path / "a"))
    named = [dict(fr, name="same") for fr in frames]
    with pytest.raises(ValueError, match="names"):
        ClipFit(named, DEV, SF.FIT, save=str(tmp_path / "b"))
    assert not os.listdir(tmp_path)


def test_fit_video_out_writes_a_folder_per_clip(tmp_path):
    from gflow_amd import fit_video, video
    from gflow_amd import viewer as V
    n = 2
    fit_video.main(["--clips", "2", "--frames", str(n), "--height", str(SF.H), "--width", str(SF.W), "--num_points", "1500",
                    "--iterations_first", "40", "--iterations_after", "20", "--iterations_camera", "10", "--clips-per-gpu", "2",
                    "--out", str(tmp_path / "log")])
    assert sorted(os.listdir(tmp_path / "log")) == ["clip_0", "clip_1"]
    for ci in range(2):
        root = tmp_path / "log" / f"clip_{ci}"
        assert sorted(os.listdir(root / "ckpt")) == [f"{t:05d}.tar" for t in range(n)]
        assert len(os.listdir(root / "images")) == 7 * n
        assert len(video.read_avi(str(root / "sequence.avi"))["frames"]) == n
    a, b = (_png(tmp_path / "log" / f"clip_{ci}" / "images" / "img_00001.png") for ci in range(2))
    assert not np.array_equal(a, b)
    assert V.main(["--folder", str(tmp_path / "log" / "clip_0"), "--path", "follow", "--out", str(tmp_path / "view")]) == 0
    assert len(os.listdir(tmp_path / "view")) == n
