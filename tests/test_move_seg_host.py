"""CPU: the move mask from the flow -- the numpy restatement (tests/move_seg_ref.py) on known answers, the host side of
gflow_amd/move_seg.py (argument checks, the sampler, the files the CLI writes), ``io.load_sequence(move_masks=...)`` and
the ABI numbers.  Also holds the scene the GPU tests (tests/test_gpu_move_seg.py) share."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import move_seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the scene
def rodrigues(r):
    r = np.asarray(r, dtype=np.float64)
    th = np.linalg.norm(r)
    k = r / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * kx @ kx


def make_scene(H, W, seed=0, noise=0.02):
    """(flow (H, W, 2) float32, disc (H, W) bool): the rigid flow of a smooth depth map (depth 1 .. 10, focal 0.9 W, pixel
    centres at + 0.5) under the rotation (0.01, -0.02, 0.005) and the translation (0.06, 0.02, 0.03); a disc of radius 0.16 H
    carries an extra (-0.9, 2.1) px; seeded Gaussian noise of ``noise`` px on everything."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f, cx, cy = 0.9 * W, W / 2.0, H / 2.0
    depth = 1.0 / (0.55 + 0.3 * np.sin(5.0 * xx / W + 0.4) * np.cos(4.0 * yy / H - 0.2) + 0.15 * np.cos(3.0 * (xx + yy) / (W + H)))
    X = np.stack([(xx + 0.5 - cx) / f * depth, (yy + 0.5 - cy) / f * depth, depth], axis=-1)
    Y = X @ rodrigues([0.01, -0.02, 0.005]).T + np.array([0.06, 0.02, 0.03])
    u, v = f * Y[..., 0] / Y[..., 2] + cx - 0.5, f * Y[..., 1] / Y[..., 2] + cy - 0.5
    flow = np.stack([u - xx, v - yy], axis=-1)
    disc = (xx - 0.62 * W) ** 2 + (yy - 0.45 * H) ** 2 <= (0.16 * H) ** 2
    flow[disc] += np.array([-0.9, 2.1])
    flow += rng.normal(scale=noise, size=flow.shape)
    return np.ascontiguousarray(flow, dtype=np.float32), disc


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return (a & b).sum() / max(int((a | b).sum()), 1)


@functools.lru_cache(maxsize=None)
def scene_case(H, W, seed, K):
    """(flow, disc, samples (K, 8), the restatement's result): computed once, shared, left unchanged"""
    from gflow_amd import move_seg as MS
    flow, disc = make_scene(H, W, seed)
    samples = MS.draw_samples(MS.known_pixels(flow), K, seed)
    ref = R.move_mask(flow, samples)
    for a in (flow, disc, samples):
        a.setflags(write=False)
    return flow, disc, samples, ref


# ------------------------------------------------------------------------------------------------- restatement: known answers
def test_pure_x_translation_gives_the_skew_matrix_of_the_x_axis():
    """A camera that moves along x: F is the skew matrix of (1, 0, 0) and every Sampson error is 0.  With a CONSTANT depth
    the scene is a plane, the classical degeneracy of the 8-point fit (x2^T F x1 = 0 for every pixel has a three-dimensional
    solution space), so the fitted F is held against the answer on a depth map with relief, where it is unique; on the
    constant depth the exact matrix is held to give exactly zero errors."""
    H, W = 24, 32
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 1.0 / (0.55 + 0.3 * np.sin(5.0 * xx / W + 0.4) * np.cos(4.0 * yy / H - 0.2))
    flow = np.zeros((H, W, 2), np.float32)
    flow[..., 0] = 0.9 * W * 0.06 / depth                 # y2 == y1 exactly: the float32 rounding of x2 is another valid shift
    rng = np.random.default_rng(0)
    samples = np.stack([rng.choice(H * W, 8, replace=False) for _ in range(64)])
    ref = R.fundamental(flow, samples)
    want = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) / np.sqrt(2.0)
    x1, x2, known = R.correspondences(flow)
    assert known.all() and np.isfinite(ref["medians"]).all()
    eps = np.finfo(np.float64).eps
    for k in range(64):
        F = ref["F_all"][k]
        # a singular vector of the SVD is good to eps sigma_max / sigma_1 times a modest constant (measured: 0.55)
        bound = 16 * eps / np.sqrt(ref["ratio"][k])
        assert min(np.abs(F - want).max(), np.abs(F + want).max()) <= bound, k
        assert R.sampson(F, x1, x2).max() <= bound ** 2 and ref["medians"][k] <= bound ** 2
    assert ref["best"] == int(np.argmin(ref["medians"]))
    # the exact matrix: every error is exactly 0 (the two products of z cancel bit for bit), also on a constant depth
    assert not R.sampson(want, x1, x2).any()
    flat = np.zeros((H, W, 2), np.float32)
    flat[..., 0] = 1.75
    f1, f2, _ = R.correspondences(flat)
    assert not R.sampson(want, f1, f2).any() and not R.mask_from(flat, want)["mask"].any()


def test_correspondences_are_the_float32_values_of_the_script():
    H, W = 5, 7
    flow = np.random.default_rng(1).normal(size=(H, W, 2)).astype(np.float32)
    x1, x2, known = R.correspondences(flow)
    uv = torch.stack(torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")[::-1], -1)
    t1 = torch.stack([2 * (uv[..., 0] + 0.5) / W - 1, 2 * (uv[..., 1] + 0.5) / H - 1], dim=-1)
    fl = torch.from_numpy(flow)
    t2 = t1 + torch.stack([2.0 * fl[..., 0] / (W - 1), 2.0 * fl[..., 1] / (H - 1)], dim=-1)
    assert np.array_equal(x1, t1.reshape(-1, 2).double().numpy()) and np.array_equal(x2, t2.reshape(-1, 2).double().numpy())
    assert known.all()


def test_lower_median_and_degenerate_samples():
    assert R.lower_median([3.0, 1.0, 2.0, 4.0]) == 2.0 and R.lower_median([5.0, 1.0, 3.0]) == 3.0
    known = np.ones(100, bool)
    known[7] = False
    assert not R.is_degenerate(np.arange(8) + 10, known)
    for bad in ([0, 1, 2, 3, 4, 5, 6, 7], [10, 11, 12, 13, 14, 15, 16, 10], [-1, 11, 12, 13, 14, 15, 16, 17],
                [100, 11, 12, 13, 14, 15, 16, 17]):
        assert R.is_degenerate(np.array(bad), known), bad


PATTERN = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [0, 1, 1, 1, 1, 1, 0, 0, 0],
                    [0, 1, 1, 1, 1, 1, 0, 0, 0],
                    [0, 1, 1, 1, 1, 1, 0, 1, 0],
                    [0, 1, 1, 1, 1, 1, 0, 0, 0],
                    [0, 1, 1, 1, 1, 1, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0]], bool)
# a 5 x 5 square eroded by disk(2) is its centre; dilated again it is the disc: the corners and the lone pixel are gone
OPENED = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0],
                   [0, 0, 0, 1, 0, 0, 0, 0, 0],
                   [0, 0, 1, 1, 1, 0, 0, 0, 0],
                   [0, 1, 1, 1, 1, 1, 0, 0, 0],
                   [0, 0, 1, 1, 1, 0, 0, 0, 0],
                   [0, 0, 0, 1, 0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0, 0, 0, 0]], bool)


def test_morphology_on_hand_drawn_patterns():
    assert R.disk(2).sum() == 13 and R.disk(3).sum() == 29 and R.disk(5).sum() == 81
    np.testing.assert_array_equal(R.opening(PATTERN), OPENED)
    eroded = np.zeros((9, 9), bool)
    eroded[3, 3] = True
    np.testing.assert_array_equal(R.erode(PATTERN, 2), eroded)
    # three full rows at the top edge: outside counts as set, so the edge row survives the erosion and the opening gives
    # the band back (with a zero border the erosion would eat it)
    band = np.zeros((9, 9), bool)
    band[:3] = True
    top = np.zeros((9, 9), bool)
    top[0] = True
    np.testing.assert_array_equal(R.erode(band, 2), top)
    np.testing.assert_array_equal(R.opening(band), band)
    assert R.erode(np.ones((9, 9), bool), 5).all() and R.erode(np.ones((8, 8), bool), 5).all()
    # dilation: outside is unset -- one pixel in the corner becomes the quarter of disk(3) that is inside
    corner = np.zeros((9, 9), bool)
    corner[0, 0] = True
    yy, xx = np.mgrid[0:9, 0:9]
    np.testing.assert_array_equal(R.dilate(corner, 3), xx * xx + yy * yy <= 9)
    assert not R.dilate(np.zeros((9, 9), bool), 3).any()
    o, e, d = R.morphology(PATTERN)
    assert o.dtype == np.uint8 and set(np.unique(o)) == {0, 255} and not e.any() and d.max() == 255


@pytest.mark.parametrize("H,W,seed", [(40, 56, 0), (40, 56, 1), (37, 53, 2)])
def test_scene_mask_covers_the_disc(H, W, seed):
    flow, disc, samples, ref = scene_case(H, W, seed, 256)
    assert iou(ref["open"], disc) >= 0.9
    assert abs(ref["err_norm"].max() - 1.0) < 1e-15 and ref["best"] >= 0
    ok = np.isfinite(ref["ratio"])
    assert ok.all() and (ref["ratio"] < 1e-9).mean() <= 0.05


def test_unknown_pixels_stay_out_of_the_restatement():
    flow, disc = make_scene(20, 24, 3)
    flow = flow.copy()
    flow[2:5, 3:9, 0] = np.nan
    flow[10, 10, 1] = np.inf
    x1, x2, known = R.correspondences(flow)
    assert (~known).sum() == 19
    from gflow_amd import move_seg as MS
    samples = MS.draw_samples(known, 8, 0)
    ref = R.move_mask(flow, samples)
    assert np.isfinite(ref["medians"]).all()
    assert not ref["err_norm"].reshape(-1)[~known].any() and not ref["mask"].reshape(-1)[~known].any()
    assert ref["err_norm"].max() == 1.0


# --------------------------------------------------------------------------------------------------------------- host API
def test_bad_shapes_raise():
    from gflow_amd import move_seg as MS
    for shape in [(8, 8), (8, 8, 3), (1, 16, 2), (16, 1, 2), (2, 3, 2), (4, 8, 2, 1)]:
        with pytest.raises(ValueError):
            MS.epipolar_move_mask(torch.zeros(shape))
    with pytest.raises(ValueError):
        MS.epipolar_move_mask(torch.zeros(8, 8, 2), threshold=float("nan"))
    with pytest.raises(ValueError):
        MS.epipolar_move_mask(torch.zeros(8, 8, 2), samples=np.zeros((4, 7), np.int32))
    with pytest.raises(ValueError):
        MS.epipolar_move_mask(torch.zeros(8, 8, 2), hypotheses=0)
    with pytest.raises(ValueError):
        MS.draw_samples(np.arange(64) < 7, 4, 0)


def test_samples_come_from_known_pixels_only():
    from gflow_amd import move_seg as MS
    flow = np.zeros((12, 16, 2), np.float32)
    flow[3:9, 2:14, 0] = np.nan
    flow[0, 0, 1] = -np.inf
    flow[11, 15] = 3e38                                   # finite, but 2 flow overflows float32
    known = MS.known_pixels(flow)
    assert known.shape == (192,) and (~known).sum() == 72 + 2 and not known[0] and not known[191]
    assert np.array_equal(known, R.correspondences(flow)[2])
    s = MS.draw_samples(known, 300, 5)
    assert s.shape == (300, 8) and s.dtype == np.int32 and known[s].all()
    assert all(len(set(row.tolist())) == 8 for row in s)
    assert np.array_equal(s, MS.draw_samples(known, 300, 5)) and not np.array_equal(s, MS.draw_samples(known, 300, 6))
    # nine known pixels: every row is eight of them, still distinct
    few = np.zeros(192, bool)
    few[10:19] = True
    s = MS.draw_samples(few, 50, 0)
    assert few[s].all() and all(len(set(row.tolist())) == 8 for row in s)


def test_cli_files_and_bytes_on_a_stub_result(tmp_path):
    from PIL import Image
    from gflow_amd import move_seg as MS
    err = np.array([[0.0, 0.5, 1.0], [0.999, 1.0 / 255.0, 0.0039]], np.float32)
    stub = dict(err_norm=torch.from_numpy(err), open=np.array([[0, 255, 0], [255, 0, 0]], np.uint8),
                erode=np.zeros((2, 3), np.uint8), dilate=np.full((2, 3), 255, np.uint8))
    paths = MS.write_result(stub, str(tmp_path / "seq_epipolar"), "00007")
    assert [os.path.basename(p) for p in paths] == ["00007_epipolar_error.png", "00007_open.png", "00007_erode.png",
                                                    "00007_dilate.png"]
    assert sorted(os.listdir(tmp_path / "seq_epipolar")) == sorted(os.path.basename(p) for p in paths)
    read = [np.asarray(Image.open(p)) for p in paths]
    # move_seg.py:242: (err * 255.0).astype(np.uint8) truncates
    np.testing.assert_array_equal(read[0], np.array([[0, 127, 255], [254, 1, 0]], np.uint8))
    np.testing.assert_array_equal(read[1], stub["open"])
    assert not read[2].any() and (read[3] == 255).all() and all(r.dtype == np.uint8 and r.shape == (2, 3) for r in read)


def test_load_sequence_reads_the_mask_files_as_before(tmp_path):
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    frames = S.make_clip(3, 24, 32, seed=0)
    assert any(bool(torch.as_tensor(fr["move_mask"]).any()) for fr in frames)
    sp = gio.write_sequence(frames, str(tmp_path / "seq"))
    a = gio.load_sequence(sp)
    b = gio.load_sequence(sp, move_masks="files")
    assert len(a) == len(b) == 2                          # (the reference's file lists drop the last image)
    for fa, fb, fr in zip(a, b, frames):
        assert sorted(fa) == sorted(fb)
        for k in fa:
            same = torch.equal(fa[k], fb[k]) if torch.is_tensor(fa[k]) else fa[k] == fb[k]
            assert same, k
        assert fa["move_mask"].dtype == torch.bool
        assert torch.equal(fa["move_mask"], torch.as_tensor(fr["move_mask"]).cpu().bool())
    # without the folder's files: zeros, as before
    for f in os.listdir(sp + "_epipolar"):
        os.remove(os.path.join(sp + "_epipolar", f))
    assert not any(bool(fr["move_mask"].any()) for fr in gio.load_sequence(sp))
    with pytest.raises(ValueError):
        gio.load_sequence(sp, move_masks="cv2")


def test_fit_video_has_the_flag(capsys):
    from gflow_amd import fit_video
    with pytest.raises(SystemExit) as e:
        fit_video.main(["--make-move-masks", "--help"])           # (parsed before a device is asked for)
    assert e.value.code == 0 and "--make-move-masks" in capsys.readouterr().out


def test_abi_numbers_agree():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert int(re.search(r"^#define GFL_VERSION (\d+)$", hdr, flags=re.M).group(1)) == 312
    assert _lib.MIN_VERSION == 312 and _lib.load().gfl_version() == 312
    for name in ("gfl_epi_workspace_bytes", "gfl_epi_fundamental", "gfl_epi_mask"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", hdr)
    lib = _lib.load()
    # refused sizes ask for nothing and are rejected before anything is launched
    for w, h, k in ((1, 40, 4), (40, 1, 4), (2, 3, 4), (8, 8, 0), (8, 8, 65536)):
        assert lib.gfl_epi_workspace_bytes(w, h, k) == 0
        assert lib.gfl_epi_fundamental(None, w, h, None, k, None, None, None, None, None, 0, None) == -1
    assert lib.gfl_epi_mask(None, 1, 40, None, 0.01, None, None, None, None, None, None, 0, None) == -1
    small, big = lib.gfl_epi_workspace_bytes(56, 40, 1), lib.gfl_epi_workspace_bytes(56, 40, 64)
    assert 56 * 40 * 10 <= small < big and big - small >= 63 * 2048 * 4
