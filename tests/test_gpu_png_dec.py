"""Decoding PNG files on the device (``-m gpu``): gfl_png_decode (include/gflow_hip.h, "PNG files": Decoding) through
``png.decode_png`` against PIL, bit for bit, over the grid of tests/test_png_dec_host.py and its hand-made files; the round
trip with the project's own encoder; malformed input, after the host harness has passed on the same streams; the loader's
``decode="device-all"`` against ``decode="host"``; the images of a saved log folder."""
import os
import warnings

import numpy as np
import pytest
import torch

from tests import png_dec_ref as R
from tests import test_png_dec_host as HT
from tests.test_png_dec_host import GRID, MODES, as_hwc, content, pil_file, pil_pixels

DEV = "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_decode_png_equals_pil_on_the_grid(mode):
    """stacks of one shape, whatever wrote their members: every content and PIL setting of a size and mode in ONE call; the
    whole cross at every size, 200 x 300 included"""
    from gflow_amd import png
    stacks = {}
    for case in dict.fromkeys(GRID + HT.GRID_LARGE):
        if case[3] == mode:
            stacks.setdefault(case[1:3], []).append(case)
    assert len(stacks) == 5
    for (H, W), cases in stacks.items():
        files = [pil_file(*c) for c in cases]
        got = png.decode_png(files, DEV)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(files), H, W, MODES[mode])
        got = got.cpu().numpy()
        for t, f in enumerate(files):
            assert np.array_equal(got[t], as_hwc(pil_pixels(f))), cases[t]


@pytest.mark.gpu
def test_decode_png_on_the_handmade_files():
    from gflow_amd import png
    stacks = {}
    for name, data, want in HT.handmade_files():
        stacks.setdefault(want.shape, []).append((name, data, want))
    for members in stacks.values():
        got = png.decode_png([d for _, d, _ in members], DEV, names=[n for n, _, _ in members]).cpu().numpy()
        for t, (name, _, want) in enumerate(members):
            assert np.array_equal(got[t], want), name
    assert tuple(png.decode_png([], DEV).shape) == (0, 0, 0, 1)
    with pytest.raises(ValueError, match="one call decodes one shape"):
        png.decode_png([pil_file("smooth", 1, 1, "L", 0), pil_file("smooth", 1, 300, "L", 0)], DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["three strips", "stored strips", "palette"])
def test_round_trip_with_the_projects_encoder(what):
    from gflow_amd import png
    if what == "three strips":                                          # W = 700, C = 3: 15 rows a strip, dynamic blocks
        x = np.stack([content("photo", 33, 700, 3, seed=s) for s in range(2)])
        assert png.strip_rows(3, 700) == 15
        files = png.encode_png(x)
    elif what == "stored strips":
        x = np.stack([content("noise", 40, 90, 3), content("noise", 40, 90, 3, seed=1)])
        files = png.encode_png(x)
    else:
        x = (content("photo", 50, 70, 1)[None] // 16).astype(np.uint8)
        files = png.encode_png(x, palette=np.arange(48, dtype=np.uint8).reshape(16, 3))
        assert png.parse_png(files[0])["colour_type"] == 3 and png.parse_png(files[0])["palette"].shape == (16, 3)
    stats = R.new_stats()
    want, status, _ = R.decode(files[0], stats)
    assert status == 0 and np.array_equal(want, x[0]) and stats["blocks"] >= ({0} if what == "stored strips" else {2})
    got = png.decode_png(files, DEV).cpu().numpy()
    assert np.array_equal(got, x)
    assert all(np.array_equal(as_hwc(pil_pixels(f)), x[t]) for t, f in enumerate(files))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(HT.N_SETS))
def test_malformed_streams(i):
    """the host harness -- the same source under the sanitizers -- passes on the set first (HT.checked_mutation asserts it);
    then the device gives the same status, entry for entry, and the same images: zeros where the status is not 0, the good
    stream beside them exact"""
    from gflow_amd import png
    s = HT.mutation_sets()[i]
    want_images, want_status = HT.checked_mutation(i)
    images, status = png.decode_streams(s["streams"], s["W"], s["H"], s["bpp"], DEV)
    assert status.tolist() == want_status.tolist(), s["name"]
    assert np.array_equal(images.cpu().numpy(), want_images), s["name"]
    assert status[-1] == 0
    files = HT.set_files(s)
    names = [f"file_{t}.png" for t in range(len(files))]
    bad = np.flatnonzero(status)
    if bad.size:
        with pytest.raises(ValueError, match=names[int(bad[0])]) as e:
            png.decode_png(files, DEV, names=names)
        assert f"status {int(status[bad[0]])}" in str(e.value) and png.STATUS[int(status[bad[0]])] in str(e.value)
    good = png.decode_png(files[-1:], DEV).cpu().numpy()
    assert np.array_equal(good[0], want_images[-1])


def _sequence(tmp_path, n=5, H=32, W=48):
    """a written clip whose images and masks are PNG files, with object annotations (palette files) beside it"""
    from PIL import Image
    from gflow_amd import io as gio
    from gflow_amd import synthetic as SY
    sp = gio.write_sequence(SY.make_clip(n, H=H, W=W), str(tmp_path / "seq"))
    os.makedirs(sp + "_mask")
    y, x = np.mgrid[0:H, 0:W]
    for k in range(n):
        ids = ((x + 3 * k) // 16 + 2 * (y // 16)).astype(np.uint8)
        img = Image.fromarray(ids)                                      # (frame 2: a grey file, read by read_mask's rule)
        if k != 2:
            img = Image.frombytes("P", (W, H), ids.tobytes())
            img.putpalette(bytes(range(256)) * 3)              # (256 entries: PIL writes 8 bits, as DAVIS-2017 does)
        img.save(os.path.join(sp + "_mask", f"{k:05d}.png"))
    return sp


TENSORS = ("image", "depth", "flow", "move_mask", "occ_mask", "object_mask")


def _same_frames(host, dev):
    assert len(host) == len(dev) == 4
    for a, b in zip(host, dev):
        assert a.keys() == b.keys() and a["name"] == b["name"]
        for k in TENSORS:
            if k in a:
                assert b[k].is_cuda and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (a["name"], k)


@pytest.mark.gpu
def test_loader_parity(tmp_path):
    from PIL import Image
    from gflow_amd import io as gio
    sp = _sequence(tmp_path)
    for resize in (None, 24):
        host = gio.load_sequence(sp, resize=resize, device=DEV, decode="host", object_masks="files")
        assert all(k in host[1] for k in TENSORS)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                             # every file is one the device takes: no warning
            dev = gio.load_sequence(sp, resize=resize, device=DEV, decode="device-all", object_masks="files")
        _same_frames(host, dev)
    # a 16-bit PNG among them is left to PIL, and said so once
    grey = np.asarray(Image.open(os.path.join(sp, "00001.png")))[..., 0].astype(np.uint16) * 257
    Image.fromarray(grey).save(os.path.join(sp, "00001.png"))
    assert np.asarray(Image.open(os.path.join(sp, "00001.png"))).dtype == np.uint16
    for resize in (None, 24):
        host = gio.load_sequence(sp, resize=resize, device=DEV, object_masks="files")
        with pytest.warns(UserWarning, match="1 of 15 image and mask files were decoded on the host"):
            dev = gio.load_sequence(sp, resize=resize, device=DEV, decode="device-all", object_masks="files")
        _same_frames(host, dev)
    est = dict(depth_camera="estimate", occ_masks="files", move_masks="files")
    with pytest.warns(UserWarning, match="1 of 11 image and mask files"):
        dev = gio.load_sequence(sp, device=DEV, decode="device-all", **est)
    for a, b in zip(gio.load_sequence(sp, device=DEV, **est), dev):
        assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["image"], b["image"])


@pytest.mark.gpu
def test_images_of_a_saved_log_folder(tmp_path):
    from gflow_amd import png
    from gflow_amd.fit_video import fit_clip
    from tests import score_fit as SF
    cfg = dict(SF.FIT, num_points=600, iterations_first=20, iterations_after=10, iterations_camera=5)
    folder = str(tmp_path / "clip")
    fit_clip(SF.clip(n_frames=2), DEV, cfg, seed=0, deterministic=True, save=folder)
    names = sorted(f for f in os.listdir(os.path.join(folder, "images")) if f.endswith(".png"))
    assert len(names) >= 14
    files = [open(os.path.join(folder, "images", n), "rb").read() for n in names]
    stacks = {}
    for n, f in zip(names, files):
        p = png.parse_png(f, n)
        stacks.setdefault((p["height"], p["width"], p["bpp"]), []).append((n, f))
    for members in stacks.values():
        got = png.decode_png([f for _, f in members], DEV, names=[n for n, _ in members]).cpu().numpy()
        for t, (n, f) in enumerate(members):
            assert np.array_equal(got[t], as_hwc(pil_pixels(f))), n
