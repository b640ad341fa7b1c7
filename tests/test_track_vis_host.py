"""CPU: the track overlays' drawing rule (tests/track_vis_ref.py) against PIL's ImageDraw and matplotlib's colormap, the
host-side helpers of gflow_amd.track_vis, and the argument checks of gfl_track_vis, which run before anything touches a
device."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageDraw

from tests import track_vis_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, CASES = 48, 64, 500


def grown(mask):
    """the 3 x 3 neighbourhood of a pixel set"""
    p = np.pad(mask, 1)
    out = np.zeros_like(mask)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def within_one_pixel(ours, pil, what):
    assert not (ours & ~grown(pil)).any(), f"{what}: a pixel of the rule's set is more than one pixel from PIL's"
    assert not (pil & ~grown(ours)).any(), f"{what}: a pixel of PIL's set is more than one pixel from the rule's"


def pil_mask(draw_fn):
    img = Image.new("L", (W, H), 0)
    draw_fn(ImageDraw.Draw(img))
    return np.array(img) != 0


def points(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1)


@pytest.mark.parametrize("width", [2, 4])
def test_segments_lie_within_one_pixel_of_pils_lines(width):
    a, b = points(10 + width, CASES), points(20 + width, CASES)
    b[::25] = a[::25]                                                # zero-length segments among them
    for k in range(CASES):
        xy = (int(a[k, 0]), int(a[k, 1]), int(b[k, 0]), int(b[k, 1]))
        ours = TR.segment_mask(H, W, a[k], b[k], width)
        pil = pil_mask(lambda d: d.line(xy, fill=255, width=width))
        within_one_pixel(ours, pil, f"line {xy} width {width}")
        assert ours[a[k, 1], a[k, 0]] and ours[b[k, 1], b[k, 0]]


def test_a_zero_length_segment_is_one_pixel_in_both():
    for w in (2, 4):
        ours = TR.segment_mask(H, W, (7, 9), (7, 9), w)
        pil = pil_mask(lambda d: d.line((7, 9, 7, 9), fill=255, width=w))
        assert ours.sum() == 1 and ours[9, 7]
        assert np.array_equal(ours, pil)


def test_the_disc_is_pils_ellipse_exactly():
    c = points(3, CASES)
    for k in range(CASES):
        x, y = int(c[k, 0]), int(c[k, 1])
        pil = pil_mask(lambda d: d.ellipse([(x - 4, y - 4), (x + 4, y + 4)], fill=255, outline=255))
        assert np.array_equal(TR.disc_mask(H, W, c[k]), pil), (x, y)


def test_crosses_lie_within_one_pixel_of_pils():
    c = points(4, CASES)
    for k in range(CASES):
        x, y = int(c[k, 0]), int(c[k, 1])

        def both(d):
            d.line([(x - 4, y), (x + 4, y)], fill=255, width=4)
            d.line([(x, y - 4), (x, y + 4)], fill=255, width=4)

        within_one_pixel(TR.cross_mask(H, W, c[k]), pil_mask(both), f"cross at {(x, y)}")


def test_whole_pictures_lie_within_one_pixel_of_the_pil_painters():
    """the painter's order end to end: wherever the rule's picture and PIL's differ, the other has that colour next door"""
    rng = np.random.default_rng(0)
    T, N = 4, 12
    video = rng.integers(0, 40, (T, H, W, 3)).astype(np.uint8)       # (dark: no track colour occurs in it)
    tracks = np.cumsum(rng.uniform(-6, 6, (T, N, 2)), axis=0) + rng.uniform(8, 40, (1, N, 2))
    occ = rng.random((T, N)) < 0.4
    ours, pil = TR.paint(video, tracks, occ, still_length=5), TR.pil_paint(video, tracks, occ, still_length=5)
    for t in range(T):
        a, b = (ours[t] != video[t]).any(-1), (pil[t] != video[t]).any(-1)
        within_one_pixel(a, b, f"frame {t}")
        assert a.any()


def test_colours_are_matplotlibs_gist_rainbow():
    """Largest difference seen against matplotlib's float64 table: 1 of 255 (the shipped table is float32, so 255 * entry
    can land on the other side of an integer); 0 in all but a few entries."""
    matplotlib = pytest.importorskip("matplotlib")
    from matplotlib.colors import Normalize
    cmap = matplotlib.colormaps["gist_rainbow"]
    rng = np.random.default_rng(1)
    worst = 0
    for case in range(40):
        n = int(rng.integers(1, 60))
        y0 = rng.integers(0, 480, n) if case % 4 else np.full(n, int(rng.integers(0, 480)))     # (ymin == ymax among them)
        still = int(rng.integers(0, n + 2))
        got = TR.colours(y0, still).astype(np.int64)
        want = np.zeros((n, 3), dtype=np.int64)
        norm = Normalize(y0.min(), y0.max())
        for i in range(n):
            want[i] = (np.array(cmap(norm(y0[i]))[:3]) * 255).astype(int)
        if 0 < still < n:
            norm = Normalize(y0[still:].min(), y0[still:].max())
            for i in range(still, n):
                want[i] = (np.array(cmap(norm(y0[i]))[:3]) * 255).astype(int)
        worst = max(worst, int(np.abs(got - want).max()))
    print("largest colour difference", worst)
    assert worst <= 1


def test_colours_with_one_y_value_take_the_first_entry():
    got = TR.colours([7, 7, 7])
    assert (got == np.trunc(TR.lut()[0].astype(np.float64) * 255).astype(np.uint8)).all()


def test_int_coords_truncate_toward_zero_and_clamp():
    v = np.array([[-0.6, 0.9], [3.99, -1.2], [np.nan, np.inf], [-np.inf, 5e9]], dtype=np.float32)
    assert TR.int_coords(v).tolist() == [[0, 0], [3, -1], [-2 ** 20, 2 ** 20], [-2 ** 20, 2 ** 20]]


def test_seed_occlusions_on_a_hand_worked_case():
    from gflow_amd.track_vis import seed_occlusions
    # 4 x 6 masks; the moving region is column 4 in frame 0, columns 2..3 in frame 1, column 1 in frame 2
    m = np.zeros((3, 4, 6), dtype=np.uint8)
    m[0, :, 4] = 255
    m[1, :, 2:4] = 255
    m[2, :, 1] = 255
    tracks = np.zeros((3, 4, 2), dtype=np.float32)
    # seed 0: still at x = 2.5 -> round half to even = 2: on frame 1's mask only
    tracks[:, 0] = [[2.5, 1.0], [2.5, 1.0], [2.5, 1.0]]
    # seed 1: starts ON the moving mask (x = 4): never occluded, wherever it goes
    tracks[:, 1] = [[4.0, 0.0], [3.0, 0.0], [1.0, 0.0]]
    # seed 2: x = 3.5 rounds to 4 (half to even) -> on frame 0's mask -> moving -> never
    tracks[:, 2] = [[3.5, 2.0], [3.5, 2.0], [1.0, 2.0]]
    # seed 3: outside the image, clipped to the border: x = -3 -> 0, y = 9 -> 3; then x = 1.4 -> 1 in frame 2
    tracks[:, 3] = [[-3.0, 9.0], [9.0, 9.0], [1.4, -2.0]]
    got = seed_occlusions(m, tracks)
    assert got.dtype == bool and got.shape == (3, 4)
    assert got.tolist() == [[False, False, False, False], [True, False, False, False], [False, False, False, True]]
    assert seed_occlusions(list(m), tracks.astype(np.float64)).tolist() == got.tolist()


def test_write_frames_writes_one_png_per_frame(tmp_path):
    from gflow_amd.track_vis import write_frames
    imgs = np.random.default_rng(0).integers(0, 255, (3, 5, 7, 3)).astype(np.uint8)
    paths = write_frames(imgs, str(tmp_path / "a" / "pred"))
    assert [os.path.basename(p) for p in paths] == ["00000.png", "00001.png", "00002.png"]
    for t, p in enumerate(paths):
        assert np.array_equal(np.array(Image.open(p)), imgs[t])
    with pytest.raises(ValueError):
        write_frames(imgs.astype(np.float32), str(tmp_path / "b"))


def test_default_k_cap_follows_the_clip():
    from gflow_amd.track_vis import default_k_cap
    assert default_k_cap(60, 300, 854, 480) == 8 * 59 * 300
    assert default_k_cap(5, 8, 72, 40) == 4 * 8 * 15                 # every segment in every tile: 5 x 3 tiles
    assert default_k_cap(1, 1, 72, 40) == 1 and default_k_cap(12, 0, 72, 40) == 1


def test_track_vis_needs_tracks_to_draw():
    from gflow_amd.fit_video import fit_clip
    with pytest.raises(ValueError, match="track_vis"):
        fit_clip([], "cpu", dict(traj_num=0), track_vis=True)


def test_the_entry_points_are_declared_and_the_version_is_unchanged():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert re.search(r"^#define GFL_VERSION 312$", hdr, flags=re.M) and _lib.MIN_VERSION == 312
    assert "track overlays (additive within 312" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("gfl_track_vis_workspace_bytes", "gfl_track_vis"):
        assert name in _lib.SIGNATURES
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1).split(",")
        assert len(_lib.SIGNATURES[name][1]) == len(args), name


def test_invalid_arguments_are_rejected_before_anything_touches_a_device():
    from gflow_amd import _lib
    lib = _lib.load()
    INVALID = -1
    assert lib.gfl_status_string(INVALID) == b"invalid argument"
    T, N, Wd, Ht, K = 3, 4, 72, 40, 100
    need = lib.gfl_track_vis_workspace_bytes(T, N, Wd, Ht, K)
    assert need >= 8 * T * N + 4 * N + 4 * K
    for bad in [(-1, N, Wd, Ht, K), (T, -1, Wd, Ht, K), (T, N, 0, Ht, K), (T, N, Wd, 0, K), (T, N, Wd, Ht, 0),
                (T, N, -5, Ht, K), (T, N, Wd, Ht, -3), (T, N, 16385, Ht, K), (T, N, Wd, 16385, K), (1 << 16, 1 << 15, Wd, Ht, K)]:
        assert lib.gfl_track_vis_workspace_bytes(*bad) == 0, bad
    # host memory stands in for every buffer: a call that got past the checks would hand it to the device runtime, so each
    # call below must come back with GFL_ERR_INVALID
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)

    def call(T=T, N=N, W=Wd, H=Ht, K=K, video=p, tracks=p, occ=p, lut=p, out=p, ovf=p, ws=p, ws_bytes=need):
        return lib.gfl_track_vis(video, tracks, occ, T, N, W, H, 0, lut, K, out, ovf, ws, ws_bytes, null)

    assert call(T=-1) == INVALID and call(N=-1) == INVALID
    assert call(W=0) == INVALID and call(H=0) == INVALID and call(K=0) == INVALID
    assert call(W=-72) == INVALID and call(H=-40) == INVALID and call(K=-1) == INVALID
    assert call(W=16385) == INVALID and call(T=1 << 16, N=1 << 15) == INVALID
    for name in ("video", "tracks", "occ", "lut", "out", "ovf", "ws"):
        assert call(**{name: null}) == INVALID, name
    assert call(ws_bytes=need - 1) == INVALID and call(ws_bytes=0) == INVALID
    # T == 0 succeeds and writes nothing (no launch: this passes without a device)
    assert call(T=0, ws_bytes=lib.gfl_track_vis_workspace_bytes(0, N, Wd, Ht, K)) == 0
    assert buf.raw == b"\0" * 64
