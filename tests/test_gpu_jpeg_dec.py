"""Decoding video files on the device (``-m gpu``): gfl_jpeg_decode (include/gflow_hip.h, "video files": Decoding) through
``video.decode_jpeg`` against PIL, bit for bit, over shapes, samplings and restart intervals; the round trip with the
project's own encoder and AVI writer; malformed input, after the host harness has passed on the same files; the loader's
``decode="device"`` against ``decode="host"``; a fit from an ``.avi`` file alone."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from gflow_amd.video import ZIGZAG
from tests import jpeg_dec_ref as R
from tests import test_jpeg_dec_host as HT
from tests.test_jpeg_dec_host import MODES, as_hwc, pil_file, pil_pixels
from tests.test_video_host import content

DEV = "cuda"
SHAPES = [(1, 1), (8, 8), (17, 23), (16, 17), (33, 31), (50, 70)]
# the third frame of a stack, by shape: a saturated checker (the clamps), the (7, 7) basis image (zero runs of 62), or 8x8
# blocks of black and white at quality 100 (DC differences of +-2040)
THIRD = {(1, 1): ("checker", 30), (8, 8): ("cosine", 90), (17, 23): ("blocks", 100), (16, 17): ("cosine", 90),
         (33, 31): ("checker", 30), (50, 70): ("blocks", 100)}


@functools.lru_cache(maxsize=None)
def blocks_file(H, W, mode, q, rmb):
    import io
    from PIL import Image
    y, x = np.mgrid[0:H, 0:W]
    a = ((((x // 8) + (y // 8)) % 2) * 255).astype(np.uint8)
    a = a if mode == "grey" else np.repeat(a[..., None], 3, axis=-1)
    kw = dict(quality=q)
    if mode != "grey":
        kw["subsampling"] = MODES[mode]
    if rmb:
        kw["restart_marker_blocks"] = rmb
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def restart_choices():
    from gflow_amd import video
    return [0, 1, 3, video.restart_interval()]


def stack_files(H, W, mode, rmb):
    """T = 3 files of one shape whose tables differ: content and optimize=True change the DHTs, the qualities the DQTs"""
    kind, q = THIRD[(H, W)]
    third = blocks_file(H, W, mode, q, rmb) if kind == "blocks" else pil_file(kind, H, W, mode, q, False, rmb)
    return [pil_file("smooth", H, W, mode, 90, False, rmb), pil_file("noise", H, W, mode, 100, True, rmb), third]


def _reached(data):
    """which of the decoder's rarer branches a file's entropy-coded data takes (from the reference's coefficients)"""
    p = R.parse(data)
    _, status, planes = R.decode_parsed(data, p)
    assert not any(status)
    zz = np.concatenate([pl.reshape(-1, 64)[:, list(ZIGZAG)] for pl in planes]).astype(np.int64)
    out = set()
    for b in zz:
        nz = np.flatnonzero(b[1:]) + 1
        if nz.size and np.diff(np.concatenate([[0], nz])).max() > 16:
            out.add("zrl")
        if b[62] != 0 and b[63] == 0:
            out.add("eob at 63")
    dc = planes[0][..., 0].astype(np.int64)
    if p["dri"] == 0 and p["comps"][0][1:3] == (1, 1) and dc.size > 1 and np.abs(np.diff(dc.reshape(-1))).max() >= 1024:
        out.add("dc category 11")                               # (luminance 1x1: raster order is scan order)
    return out


def test_shapes_reach_the_branches():
    """The cases of test_decode_equals_pil were chosen for these; if a PIL build codes them otherwise this says which is lost."""
    from gflow_amd import video
    assert video.restart_interval() not in (0, 1, 3)
    p = video.parse_jpeg(stack_files(1, 1, "420", 0)[0])
    assert (p["hs"], p["vs"]) == (2, 2) and -(-p["width"] // 2) == 1                         # cw == 1, ch == 1
    assert video.parse_jpeg(stack_files(1, 1, "422", 0)[0])["hs"] == 2
    p = video.parse_jpeg(stack_files(17, 23, "420", 0)[0])
    assert p["width"] % 16 and p["height"] % 16 and p["mcus"] == (2, 2)                      # partial MCUs on both edges
    assert video.parse_jpeg(stack_files(16, 17, "422", 0)[0])["mcus"] == (2, 2)              # 17 = 16 + 1: a column of one
    assert len(video.parse_jpeg(stack_files(50, 70, "444", 3)[0])["units"]) == 21            # more than 8: RSTm wraps
    assert len(video.parse_jpeg(stack_files(50, 70, "420", 1)[0])["units"]) == 20
    assert len(video.parse_jpeg(stack_files(50, 70, "444", video.restart_interval())[0])["units"]) == 2
    assert "zrl" in _reached(stack_files(16, 17, "444", 0)[2])
    assert "eob at 63" in _reached(stack_files(50, 70, "444", 0)[1])
    assert "dc category 11" in _reached(stack_files(17, 23, "grey", 0)[2])
    tabs = [video.parse_jpeg(f) for f in stack_files(33, 31, "420", 0)]
    assert tabs[0]["huffman"] != tabs[1]["huffman"] and not np.array_equal(tabs[0]["quant"][0], tabs[2]["quant"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("ri", range(4))
def test_decode_equals_pil(mode, ri):
    from gflow_amd import video
    rmb = restart_choices()[ri]
    for H, W in SHAPES:
        files = stack_files(H, W, mode, rmb)
        got = video.decode_jpeg(files, DEV)
        C = 1 if mode == "grey" else 3
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W, C) and got.is_cuda
        got = got.cpu().numpy()
        for t, f in enumerate(files):
            want = as_hwc(pil_pixels(f))
            assert np.array_equal(got[t], want), (H, W, mode, rmb, t, int(np.abs(got[t].astype(int) - want).max()))


@pytest.mark.gpu
def test_empty_and_mixed_stacks():
    from gflow_amd import video
    assert tuple(video.decode_jpeg([], DEV).shape)[0] == 0
    with pytest.raises(ValueError, match="frame 1"):
        video.decode_jpeg([pil_file("smooth", 16, 17, "444", 90), pil_file("smooth", 16, 17, "420", 90)], DEV)
    with pytest.raises(ValueError, match="frame 1.*progressive"):
        import io
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.asarray(content("smooth", 16, 17))).save(buf, format="JPEG", progressive=True)
        video.decode_jpeg([pil_file("smooth", 16, 17, "444", 90), buf.getvalue()], DEV)


@pytest.mark.gpu
def test_round_trip_with_the_projects_encoder(tmp_path):
    from gflow_amd import video
    for C in (3, 1):
        x = np.stack([np.asarray(content(k, 33, 70, C)) for k in ("smooth", "noise", "checker")])
        files = video.encode_jpeg(x, quality=90)
        got = video.decode_jpeg(files, DEV).cpu().numpy()
        for t, f in enumerate(files):
            assert np.array_equal(got[t], as_hwc(pil_pixels(f))), (C, t)
    x = np.stack([np.asarray(content("smooth", 24, 40, 3, seed)) for seed in range(5)])
    x[1:] = np.roll(x[1:], 3, axis=2)
    path = str(tmp_path / "clip.avi")
    video.write_avi(path, x, fps=5, quality=90, chunk=2)
    frames = video.read_avi(path)["frames"]
    got = video.read_avi_frames(path, DEV, chunk=2)
    assert tuple(got.shape) == (5, 24, 40, 3)
    for t, f in enumerate(frames):
        assert np.array_equal(got[t].cpu().numpy(), pil_pixels(f)), t
    some = video.read_avi_frames(path, DEV, select=[4, 1])
    assert torch.equal(some, got[[4, 1]])
    assert video.main(["--unpack", path, "--out", str(tmp_path / "png")]) == 0
    from PIL import Image
    assert sorted(os.listdir(tmp_path / "png")) == [f"frame_{t:05d}.png" for t in range(5)]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "png" / "frame_00003.png")), got[3].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(7))
def test_malformed_input(i):
    """Exactly the mutated files of tests/test_jpeg_dec_host.py, and only after the sanitized host build of the same source has
    decoded them without a report (``checked_mutation`` runs it first and holds it to the reference): the device gives the
    same status array and the same pixels, ``decode_jpeg`` raises ValueError naming the frame, and a good decode on the same
    stream afterwards is exact."""
    from gflow_amd import video
    want_images, want_status = HT.checked_mutation(i)
    s = HT.mutation_sets()[i]
    units, tables, data, shape = s["arrays"]
    images, status = video.decode_stack(units, tables, data, shape["W"], shape["H"], shape["C"], shape["hs"], shape["vs"], DEV)
    assert np.array_equal(status, want_status), (s["name"], status.tolist(), want_status.tolist())
    assert np.array_equal(images.cpu().numpy(), want_images), s["name"]
    if s["files"] is not None and want_status.any():
        first = int(units["frame"][np.flatnonzero(want_status)[0]])
        with pytest.raises(ValueError, match=f"frame {first}, unit"):
            video.decode_jpeg(s["files"], DEV)
    for name, f in s["refused"]:
        with pytest.raises(ValueError, match="frame 0"):
            video.decode_jpeg([f], DEV)
    good = pil_file(*HT.BASE_A)
    assert np.array_equal(video.decode_jpeg([good], DEV)[0].cpu().numpy(), pil_pixels(good))


def _jpeg_sequence(tmp_path, n=5, H=32, W=48):
    """a written clip whose images are .jpg files (4:2:0, as a camera's)"""
    from PIL import Image
    from gflow_amd import io as gio
    from gflow_amd import synthetic as SY
    sp = gio.write_sequence(SY.make_clip(n, H=H, W=W), str(tmp_path / "seq"))
    for name in sorted(os.listdir(sp)):
        Image.open(os.path.join(sp, name)).save(os.path.join(sp, name[:-4] + ".jpg"), quality=92)
        os.remove(os.path.join(sp, name))
    return sp


@pytest.mark.gpu
def test_loader_parity(tmp_path):
    from PIL import Image
    from gflow_amd import io as gio
    sp = _jpeg_sequence(tmp_path)
    for resize in (None, 24):
        host = gio.load_sequence(sp, resize=resize, device=DEV, decode="host")
        with warnings.catch_warnings():
            warnings.simplefilter("error")                         # every file is one the device takes: no warning
            dev = gio.load_sequence(sp, resize=resize, device=DEV, decode="device")
        assert len(host) == len(dev) == 4
        for a, b in zip(host, dev):
            assert a.keys() == b.keys() and a["name"] == b["name"]
            assert torch.equal(a["image"], b["image"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["flow"], b["flow"])
    # a PNG among them is left to PIL, and said so once
    Image.open(os.path.join(sp, "00001.jpg")).save(os.path.join(sp, "00001.png"))
    os.remove(os.path.join(sp, "00001.jpg"))
    host = gio.load_sequence(sp, device=DEV)
    with pytest.warns(UserWarning, match="1 of 4 images were decoded on the host"):
        dev = gio.load_sequence(sp, device=DEV, decode="device")
    assert [f["name"] for f in dev] == [f["name"] for f in host]
    assert all(torch.equal(a["image"], b["image"]) for a, b in zip(host, dev))
    est = dict(flows="estimate", move_masks="epipolar", occ_masks="flow")
    for a, b in zip(gio.load_sequence(sp, device=DEV, **est), gio.load_sequence(sp, device=DEV, decode="device", **est)):
        assert torch.equal(a["flow"], b["flow"]) and torch.equal(a["move_mask"], b["move_mask"])


@pytest.mark.gpu
def test_fit_from_an_avi(tmp_path, capsys):
    """a clip that is ONE file: the four --make-* options supply everything else.  The frames are the tensors the same JPEG
    images give from a folder, and a tiny fit runs (completion and finiteness only)."""
    from gflow_amd import fit_video, video
    from gflow_amd import io as gio
    from gflow_amd import synthetic as SY
    clip = SY.make_clip(4, H=48, W=64)
    x = torch.stack([(torch.as_tensor(fr["image"]).float().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8) for fr in clip])
    avi = str(tmp_path / "clip.avi")
    video.write_avi(avi, x, fps=5, quality=95)
    os.makedirs(tmp_path / "folder")
    for t, f in enumerate(video.read_avi(avi)["frames"]):
        with open(tmp_path / "folder" / f"frame_{t:05d}.jpg", "wb") as out:
            out.write(f)
    est = dict(flows="estimate", move_masks="epipolar", occ_masks="flow", depth_camera="estimate")
    a = gio.load_sequence(avi, device=DEV, **est)
    b = gio.load_sequence(str(tmp_path / "folder"), device=DEV, **est)
    assert len(a) == len(b) == 3 and [f["name"] for f in a] == ["frame_00000", "frame_00001", "frame_00002"]
    for fa, fb in zip(a, b):
        assert fa.keys() == fb.keys() and fa["name"] == fb["name"]
        for k in ("image", "depth", "flow", "move_mask"):
            assert torch.equal(fa[k], fb[k]), k
    assert len(gio.load_sequence(avi, device=DEV, frame_start=1, frame_range=2, **est)) == 2
    out = fit_video.main(["--sequence", avi, "--make-flows", "--make-move-masks", "--make-occ-masks", "--make-depth-camera",
                          "--num_points", "1000", "--iterations_first", "30", "--iterations_after", "30", "--iterations_camera", "30"])
    capsys.readouterr()
    assert out["frames"] == 3 and np.isfinite(out["psnr_mean_db"])
    assert sorted(os.listdir(tmp_path)) == ["clip.avi", "folder"]                       # nothing was written
