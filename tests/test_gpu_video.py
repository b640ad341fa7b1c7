"""Video files on the device (``-m gpu``): gfl_jpeg_sizes / gfl_jpeg_emit (include/gflow_hip.h, "video files") and
gflow_amd.video on top of them, against the float64 / integer restatement tests/jpeg_ref.py (which tests/test_video_host.py
pins to PIL).  Three things are held: the files open (PIL, read_avi); the entropy coding is EXACT -- the device's scan decodes,
and re-coding what it decodes gives the device's bytes; the coefficients are float64's, except by one where float32 may round
the other way (test_video_host.WINDOW holds the derivation)."""
import functools

import numpy as np
import pytest
import torch

from tests import jpeg_ref as R
from tests.test_video_host import content, near_half, pil_decode, pil_jpeg, psnr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ri():
    from gflow_amd import video
    return video.restart_interval()


def shape_of(name):
    """(H, W) of the named shape: the smallest that reach every branch, from the library's restart interval"""
    ri = _ri()
    return {"one": (8, 8),                       # one MCU, one interval
            "edge": (9, 17),                     # both edges hang over
            "row": (8, 8 * (ri + 1)),            # ri + 1 MCUs in a row: the last interval holds one
            "wrap": (80, 8 * (ri + 1)),          # 10 ri + 10 MCUs: RST7 is followed by a second RST0
            "odd": (33, 70)}[name]


def test_shapes_reach_the_branches():
    ri = _ri()
    n = {k: R.n_mcus(*shape_of(k)[::-1]) for k in ("one", "edge", "row", "wrap")}
    assert n["one"] == 1 and n["edge"] == 6 and n["row"] == ri + 1 and n["row"] % ri == 1
    assert n["wrap"] >= 9 * ri + 1 and -(-n["wrap"] // ri) >= 10                 # (the last interval has no marker)


# (content, shape, C, quality)
CASES = [("flat", "one", 3, 90), ("noise", "edge", 3, 90), ("smooth", "row", 3, 90), ("noise", "wrap", 3, 100),
         ("smooth", "wrap", 3, 50), ("checker", "edge", 3, 100), ("cosine", "odd", 3, 90), ("smooth", "edge", 1, 50),
         ("noise", "odd", 1, 100), ("smooth", "odd", 3, 90)]


@functools.lru_cache(maxsize=None)
def device_file(kind, shape, C, q):
    """the complete file the device makes of one image; coded once"""
    from gflow_amd import video
    H, W = shape_of(shape)
    files = video.encode_jpeg(content(kind, H, W, C)[None], quality=q)
    assert len(files) == 1
    return files[0]


@functools.lru_cache(maxsize=None)
def reference(kind, shape, C, q):
    """(ratios F / q, coefficients) in float64"""
    H, W = shape_of(shape)
    r = R.ratios(content(kind, H, W, C), q)
    r.setflags(write=False)
    return r, R.quantise(r)


@pytest.mark.parametrize("kind,shape,C,q", CASES)
def test_pil_opens_the_file(kind, shape, C, q):
    from gflow_amd import video
    H, W = shape_of(shape)
    data = device_file(kind, shape, C, q)
    assert data.startswith(video.jpeg_header(W, H, C, q)) and data.endswith(video.EOI)
    im = pil_decode(data)
    assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")
    img = content(kind, H, W, C)
    ours, pils = psnr(np.asarray(im), img), psnr(np.asarray(pil_decode(pil_jpeg(img, q))), img)
    print(f"{kind} {shape} C={C} q={q}: device {ours:.3f} dB, PIL {pils:.3f} dB")
    assert ours >= pils - 0.2 or ours == float("inf")


@pytest.mark.parametrize("kind,shape,C,q", CASES)
def test_entropy_coding_is_exact(kind, shape, C, q):
    """decode the device's scan, code what it held again with the reference coder: the device's bytes, bit for bit -- the
    markers, the padding and the stuffing included"""
    H, W = shape_of(shape)
    ri = _ri()
    scan = R.scan_of(device_file(kind, shape, C, q))
    coef = R.decode_scan(scan, R.n_mcus(W, H), C, ri)
    assert R.entropy_encode(coef, ri) == scan


@pytest.mark.parametrize("kind,shape,C,q", CASES)
def test_coefficients_are_float64s_but_for_ties(kind, shape, C, q):
    """every coefficient is the reference's, or one off where the reference's F / q lies within WINDOW / q of a half integer;
    on the reference alone, that window holds at most 5 % of the input's coefficients.
    Measured over CASES: 0.00 - 3.44 % of the coefficients lie inside the window (the most on noise at quality 100, where
    q = 1); the device differs in 4 of 2 880 coefficients of the grey noise image, all inside the window, and in none of the
    other nine inputs."""
    H, W = shape_of(shape)
    ratio, want = reference(kind, shape, C, q)
    tie = near_half(ratio, q, C)
    assert tie.mean() <= 0.05, f"{100 * tie.mean():.2f} % of the coefficients lie inside the window"
    got = R.decode_scan(R.scan_of(device_file(kind, shape, C, q)), R.n_mcus(W, H), C, _ri())
    d = got - want
    print(f"{kind} {shape} C={C} q={q}: {100 * tie.mean():.2f} % inside the window, {int((d != 0).sum())} of {d.size} differ")
    assert np.abs(d).max() <= 1
    assert not np.any((d != 0) & ~tie), f"{int(((d != 0) & ~tie).sum())} coefficients differ outside the window"


def test_contents_reach_the_coder_branches():
    """on the REFERENCE's streams: byte stuffing, ZRL, the largest AC categories, DC-only blocks"""
    ri = _ri()
    assert b"\xff\x00" in R.entropy_encode(reference("noise", "wrap", 3, 100)[1], ri)
    flat = reference("flat", "one", 3, 90)[1]
    assert np.all(flat[:, :, 1:] == 0)
    cos = reference("cosine", "odd", 3, 90)[1]
    assert np.any(np.all(cos[:, 0, 1:63] == 0, axis=-1) & (cos[:, 0, 63] != 0))           # a run of 62: ZRL three times
    assert np.abs(reference("checker", "edge", 3, 100)[1][:, 0, 1:]).max() >= 512          # category 10
    wrap = R.entropy_encode(reference("smooth", "wrap", 3, 50)[1], ri)
    assert len(R.split_intervals(wrap)) >= 10 and wrap.count(b"\xff\xd0") >= 2              # RST0 .. RST7, RST0 again


def test_stack_of_frames_offsets_and_avi(tmp_path):
    """T = 3 frames of different content: every frame is what it is alone, grey and colour; write_avi -> read_avi gives
    those bytes"""
    from gflow_amd import video
    H, W = shape_of("odd")
    for C in (3, 1):
        stack = np.stack([content(k, H, W, C) for k in ("smooth", "noise", "flat")])
        alone = [video.encode_jpeg(stack[t:t + 1], quality=90)[0] for t in range(3)]
        assert len(set(alone)) == 3
        assert video.encode_jpeg(torch.from_numpy(stack.copy()).to(DEV), quality=90) == alone     # a device tensor
        assert video.encode_jpeg(stack, quality=90) == alone                                       # a host array
        path = str(tmp_path / f"c{C}.avi")
        info = video.write_avi(path, stack, fps=12.5, quality=90, chunk=2)                         # stacks of 2 and 1
        got = video.read_avi(path)
        assert got["frames"] == alone and info["frames"] == 3 and (got["width"], got["height"]) == (W, H)
        assert got["fps"] == 12.5
        for t in range(3):
            assert pil_decode(got["frames"][t]).size == (W, H)
    assert video.encode_jpeg(np.zeros((0, 8, 8, 3), dtype=np.uint8)) == []
    with pytest.raises(ValueError):
        video.encode_jpeg(np.zeros((1, 8, 8, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        video.encode_jpeg(np.zeros((1, 8, 8, 3), dtype=np.float32))


def test_the_two_passes_agree():
    """frame_offsets[T] is what the second pass writes -- no byte behind it is touched -- and a second run gives the same bytes;
    an `out` that is too small is never written past"""
    from gflow_amd import _lib as L
    from gflow_amd import video
    H, W = shape_of("wrap")
    T, C, q = 3, 3, 100
    stack = torch.from_numpy(np.stack([content(k, H, W, C) for k in ("noise", "smooth", "checker")])).to(DEV)
    lib = L.load()
    qt = torch.from_numpy(video.quant_tables(q).astype(np.int16)).to(DEV)
    ws = L.scratch(lib.gfl_jpeg_workspace_bytes(T, C, W, H), DEV)
    off = torch.full((T + 1,), -1, dtype=torch.int64, device=DEV)
    args = (L.ptr(stack), T, C, W, H, L.ptr(qt))

    def run(out_bytes=None):
        L.check(lib.gfl_jpeg_sizes(*args, L.ptr(off), L.ptr(ws), ws.numel(), L.stream()), "sizes")
        o = off.cpu().numpy()
        total = int(o[T])
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        L.check(lib.gfl_jpeg_emit(*args, L.ptr(out), total if out_bytes is None else out_bytes, L.ptr(ws), ws.numel(),
                                  L.stream()), "emit")
        return o, out.cpu().numpy()

    o, a = run()
    total = int(o[T])
    assert o[0] == 0 and np.all(np.diff(o) > 0)
    assert np.all(a[total:] == 0xA5)                                   # the canary
    ri = _ri()
    for t in range(T):
        scan = a[o[t]:o[t + 1]].tobytes()
        coef = R.decode_scan(scan, R.n_mcus(W, H), C, ri)               # (every byte in front of the total was written)
        assert R.entropy_encode(coef, ri) == scan
    o2, b = run()
    assert np.array_equal(o, o2) and np.array_equal(a, b)
    # a buffer one byte short: the last interval is left out, nothing lands behind the buffer
    _, c = run(out_bytes=total - 1)
    tail = a[o[T - 1]:total].tobytes()
    last = int(o[T - 1]) + max(tail.rfind(bytes([0xFF, 0xD0 + m])) for m in range(8)) + 2      # where the last interval starts
    assert np.array_equal(c[:last], a[:last]) and np.all(c[last:] == 0xA5)


def _tiny_fit(folder):
    """the saved fit tests/test_gpu_render_batch.py builds for its viewer test: two frames of 96 x 64"""
    from gflow_amd import synthetic as S
    from gflow_amd.trainer import SimpleGaussian
    clip = S.make_clip(2, H=64, W=96, seed=5)
    for k, frame in enumerate(clip):
        tr = SimpleGaussian(frame["image"], frame["depth"], num_points=800, device=DEV, seed=k, log_dir=str(folder))
        tr.load_camera(focal=frame["focal"], pp=frame["pp"], extr=frame["extr_gt"])
        tr.init_gaussians_from_image(frame["image"], frame["depth"], num_points=800)
        tr.train(iterations=8, lr=4e-3, lr_camera=1e-3, lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0,
                 move_mask=frame["move_mask"], densify_interval=6, densify_times=1, snapshot_interval=0)
        tr.save_checkpoint(ckpt_name=f"{k:04d}")


def test_viewer_writes_a_video(tmp_path):
    """--video gives one AVI whose frames are as close to the path's images (--format png) as PIL's own JPEG of them at the
    same quality and sampling, to within 1 dB"""
    from gflow_amd import video
    from gflow_amd import viewer as V
    from PIL import Image
    _tiny_fit(tmp_path)
    avi, png, Q = tmp_path / "v" / "orbit.avi", tmp_path / "png", 85
    path = ["--folder", str(tmp_path), "--path", "orbit:1,5,0.05"]
    assert V.main(path + ["--video", str(avi), "--fps", "12", "--quality", str(Q)]) == 0          # no --out
    assert V.main(path + ["--out", str(png), "--format", "png"]) == 0
    got = video.read_avi(str(avi))
    assert len(got["frames"]) == 5 and (got["width"], got["height"], got["fps"]) == (96, 64, 12.0)
    for k, data in enumerate(got["frames"]):
        src = np.asarray(Image.open(png / f"{k:06d}.png"))
        im = pil_decode(data)
        assert im.size == (96, 64) and im.mode == "RGB"
        ours, pils = psnr(np.asarray(im), src), psnr(np.asarray(pil_decode(pil_jpeg(src, Q))), src)
        print(f"viewer frame {k}: device {ours:.2f} dB, PIL {pils:.2f} dB")
        assert abs(ours - pils) <= 1.0
    both = tmp_path / "both"
    assert V.main(path + ["--video", str(tmp_path / "b.avi"), "--out", str(both), "--format", "jpeg"]) == 0
    assert len(list(both.iterdir())) == 5 and len(video.read_avi(str(tmp_path / "b.avi"))["frames"]) == 5


def test_track_vis_write_video(tmp_path):
    from gflow_amd import track_vis, video
    H, W = shape_of("odd")
    stack = torch.from_numpy(np.stack([content(k, H, W, 3) for k in ("smooth", "noise", "flat", "checker")])).to(DEV)
    path = str(tmp_path / "clip_0" / "pred.avi")
    info = track_vis.write_video(stack, path)
    got = video.read_avi(path)
    assert info["frames"] == len(got["frames"]) == got["total_frames"] == 4 and got["fps"] == 5.0
    assert got["frames"] == video.encode_jpeg(stack, quality=90)


def test_fit_video_writes_an_avi_beside_every_folder_of_frames(tmp_path):
    """--track-vis DIR --video: DIR/clip_0/<name>.avi at 5 fps beside DIR/clip_0/<name>/, whose PNGs are as they were; the
    AVI's frames are the device's JPEG of those PNGs"""
    import os
    from PIL import Image
    from gflow_amd import fit_video, video
    from tests import score_fit as SF
    n = 2
    fit_video.main(["--clips", "1", "--frames", str(n), "--height", str(SF.H), "--width", str(SF.W), "--num_points", "1500",
                    "--iterations_first", "40", "--iterations_after", "20", "--iterations_camera", "10", "--track",
                    "--track-vis", str(tmp_path / "vis"), "--video"])
    root = tmp_path / "vis" / "clip_0"
    names = sorted(os.listdir(root))
    assert names == ["gt", "gt.avi", "pred", "pred.avi"]
    for name in ("gt", "pred"):
        assert sorted(os.listdir(root / name)) == [f"{t:05d}.png" for t in range(n)]
        got = video.read_avi(str(root / (name + ".avi")))
        assert got["fps"] == 5.0 and (got["width"], got["height"]) == (SF.W, SF.H)
        pngs = np.stack([np.asarray(Image.open(root / name / f"{t:05d}.png")) for t in range(n)])
        assert got["frames"] == video.encode_jpeg(pngs, quality=90)


def test_module_cli_packs_a_folder(tmp_path, capsys):
    from PIL import Image
    from gflow_amd import video
    H, W = shape_of("odd")
    kinds = ("smooth", "noise", "flat")
    for k, kind in enumerate(kinds):
        Image.fromarray(np.asarray(content(kind, H, W, 3))).save(tmp_path / f"{k:03d}.png")
    out = tmp_path / "packed.avi"
    assert video.main(["--frames", str(tmp_path), "--out", str(out), "--fps", "24", "--quality", "75"]) == 0
    got = video.read_avi(str(out))
    assert got["fps"] == 24.0 and (got["width"], got["height"]) == (W, H)
    assert got["frames"] == video.encode_jpeg(np.stack([content(k, H, W, 3) for k in kinds]), quality=75)
    assert "3 frames" in capsys.readouterr().out
