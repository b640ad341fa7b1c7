"""CPU: occlusion masks from the flows -- the float64 restatement (tests/occ_ref.py) against torch's grid_sample and on
known answers, the analytic backward flow of the synthetic clip, the host side of gflow_amd/occlusion.py, the loader option,
the fit_video flag and the ABI entry.  Also holds the scenes the GPU tests (tests/test_gpu_occlusion.py) share."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import occ_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISC_FLOW = (4.25, -2.75)


# ------------------------------------------------------------------------------------------------------------ the scenes
def make_scene(H, W, seed=0, noise=0.05):
    """(fwd, bwd) (H, W, 2) float32: a smooth field with a disc of radius 0.22 min(H, W) at (0.4 W, 0.5 H) that moves by
    (4.25, -2.75); the backward flow is the negated field at (x - 1.5, y + 0.5), the disc shifted by its motion; seeded
    N(0, noise^2) on both."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    field = lambda x, y: np.stack([1.5 + 0.8 * np.sin(x / 7.0 + 0.3) * np.cos(y / 5.0),
                                   -0.5 + 0.6 * np.cos(x / 9.0) * np.sin(y / 6.0 + 1.0)], axis=-1)
    r, cx, cy = 0.22 * min(H, W), 0.4 * W, 0.5 * H
    fwd = field(xx, yy)
    fwd[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = DISC_FLOW
    bwd = -field(xx - 1.5, yy + 0.5)
    bwd[(xx - cx - DISC_FLOW[0]) ** 2 + (yy - cy - DISC_FLOW[1]) ** 2 < r * r] = (-DISC_FLOW[0], -DISC_FLOW[1])
    fwd += rng.normal(scale=noise, size=fwd.shape)
    bwd += rng.normal(scale=noise, size=bwd.shape)
    return np.ascontiguousarray(fwd, dtype=np.float32), np.ascontiguousarray(bwd, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def scene_case(H, W, seed):
    """(fwd, bwd, the restatement's result): computed once, shared, left unchanged"""
    fwd, bwd = make_scene(H, W, seed)
    ref = R.flow_occlusion(fwd, bwd)
    for a in (fwd, bwd) + tuple(ref.values()):
        a.setflags(write=False)
    return fwd, bwd, ref


def band(ref, key=""):
    """the pixels whose mask the float32 kernel may decide either way: |d - thr| <= 1e-4 (1 + thr)"""
    return ref["known" + key] & (np.abs(ref["diff" + key] - ref["thr"]) <= 1e-4 * (1.0 + ref["thr"]))


def constant_pair(H, W, flow):
    fwd = np.empty((H, W, 2), np.float32)
    fwd[:] = flow
    return fwd, -fwd


SYNTHETIC = [(cs, k) for cs in (0.01, 0.03) for k in (1, 3)]


@functools.lru_cache(maxsize=None)
def synthetic_pair(cam_step, k, H=120, W=160):
    """(flow k - 1 -> k, flow k -> k - 1, frame k's occ_mask) of the synthetic clip's scene"""
    from gflow_amd import synthetic as S
    sc = S._Scene(H, W, 0, cam_step=cam_step)
    out = (sc.frame(k - 1)["flow"].numpy(), sc.backward_flow(k).numpy(), sc.frame(k)["occ_mask"].numpy())
    for a in out:
        a.setflags(write=False)
    return out


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return (a & b).sum() / max(int((a | b).sum()), 1)


# -------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_is_grid_sample_align_corners_zeros():
    """explicit floor and gather == grid_sample(bilinear, zeros, align_corners=True) at the normalised x + flow, to 1e-12:
    the synthetic pairs, the smooth scene and the known answers"""
    pairs = [synthetic_pair(cs, k)[:2] for cs, k in SYNTHETIC] + [scene_case(33, 47, 0)[:2], scene_case(97, 131, 1)[:2],
                                                                  constant_pair(9, 12, (3.0, -2.0)),
                                                                  constant_pair(9, 12, (0.5, 0.0))]
    for fwd, bwd in pairs:
        ref = R.flow_occlusion(fwd, bwd)
        assert ref["known"].all() and ref["known_bwd"].all()
        d_f, d_b, thr = R.flow_occlusion_grid_sample(fwd, bwd)
        for got, want in ((ref["diff"], d_f), (ref["diff_bwd"], d_b), (ref["thr"], thr)):
            err = np.abs(got - want).max()
            print(fwd.shape, err)
            assert err <= 1e-12


def test_known_answer_constant_flow():
    H, W = 9, 12
    fwd, bwd = constant_pair(H, W, (3.0, -2.0))
    ref = R.flow_occlusion(fwd, bwd)
    yy, xx = np.mgrid[0:H, 0:W]
    out_f = (xx + 3 > W - 1) | (yy - 2 < 0)
    out_b = (xx - 3 < 0) | (yy + 2 > H - 1)
    assert np.array_equal(ref["occ"], np.where(out_f, 255, 0)) and np.array_equal(ref["occ_bwd"], np.where(out_b, 255, 0))
    assert not ref["diff"][~out_f].any() and not ref["diff_bwd"][~out_b].any()
    np.testing.assert_allclose(ref["diff"][out_f], np.hypot(3.0, 2.0), rtol=1e-15)
    np.testing.assert_allclose(ref["thr"], 0.01 * 2 * np.hypot(3.0, 2.0) + 0.5, rtol=1e-15)


def test_known_answer_half_pixel():
    H, W = 9, 12
    ref = R.flow_occlusion(*constant_pair(H, W, (0.5, 0.0)))
    assert not ref["diff"][:, :-1].any() and (ref["diff"][:, -1] == 0.25).all()       # half of the sample is outside
    assert not ref["diff_bwd"][:, 1:].any() and (ref["diff_bwd"][:, 0] == 0.25).all()
    assert not ref["occ"].any() and not ref["occ_bwd"].any()                           # 0.25 < 0.01 * 1 + 0.5


def test_unknown_pixels_of_the_restatement():
    fwd, bwd = constant_pair(8, 10, (1.0, 0.0))
    fwd, bwd = fwd.copy(), bwd.copy()
    fwd[3, 4] = (np.nan, 0.0)
    bwd[5, 6] = (1e30, 0.0)
    ref = R.flow_occlusion(fwd, bwd)
    # its own pixel (d and thr), and in the other direction the pixels whose sample reads it: the NaN at weight 1 from
    # (3, 5) and at weight 0 from the row above (the integer flow reads columns x - 1, x and rows y, y + 1), the 1e30 at
    # weight 1 only (0 * 1e30 = 0)
    assert not ref["known"][3, 4] and not ref["known_bwd"][3, 4] and not ref["known_bwd"][3, 5]
    assert not ref["known_bwd"][2, 4] and not ref["known_bwd"][2, 5]
    assert not ref["known_bwd"][5, 6] and not ref["known"][5, 6] and not ref["known"][5, 5]
    assert (~ref["known"]).sum() == 3 and (~ref["known_bwd"]).sum() == 5
    for k in ("", "_bwd"):
        assert not ref["diff" + k][~ref["known" + k]].any() and not ref["occ" + k][~ref["known" + k]].any()
    # a NaN poisons at weight 0 as well: the sample of (2, 5) lands exactly on (2, 6) and reads (2, 7) with t = 0
    fwd, bwd = constant_pair(8, 10, (1.0, 0.0))
    bwd = bwd.copy()
    bwd[2, 7] = (np.nan, np.nan)
    ref = R.flow_occlusion(fwd, bwd)
    assert not ref["known"][2, 6] and not ref["known"][2, 5] and not ref["known"][1, 6] and not ref["known"][1, 5]
    assert ref["known"][2, 4] and ref["known"][3, 6] and (~ref["known"]).sum() == 5          # (the fifth: its own pixel)


@pytest.mark.parametrize("cam_step,k", SYNTHETIC)
def test_synthetic_backward_flow_finds_the_occlusion_mask(cam_step, k):
    fwd, bwd, occ = synthetic_pair(cam_step, k)
    assert bwd.shape == fwd.shape and bwd.dtype == np.float32
    got = R.flow_occlusion(fwd, bwd)["occ_bwd"] != 0
    score, recall = iou(got, occ), (got & occ).sum() / max(int(occ.sum()), 1)
    print(cam_step, k, "IoU", score, "recall", recall, "pixels", int(occ.sum()))
    assert occ.sum() > 50 and score >= 0.88


def test_backward_flow_leaves_the_frames_alone():
    from gflow_amd import synthetic as S
    sc = S._Scene(24, 32, 0)
    a = sc.frame(2)
    bwd = sc.backward_flow(2)
    b = sc.frame(2)
    assert all(torch.equal(a[key], b[key]) for key in ("image", "depth", "flow", "move_mask", "occ_mask"))
    # on the disc: minus the previous frame's forward step; background: along x only
    move = a["move_mask"]
    step = sc.frame(1)["flow"][sc.frame(1)["move_mask"]][0]
    assert torch.allclose(bwd[move], -step.expand_as(bwd[move]), atol=1e-6) and not bwd[~move][:, 1].any()
    with pytest.raises(ValueError):
        sc.backward_flow(0)


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_entry_within_312():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert int(re.search(r"^#define GFL_VERSION (\d+)$", hdr, flags=re.M).group(1)) == 312
    assert _lib.MIN_VERSION == 312 and _lib.load().gfl_version() == 312
    assert "gfl_flow_occlusion" in _lib.SIGNATURES and re.search(r"\bgfl_flow_occlusion\(", hdr)
    assert "UNPINNED" in hdr[hdr.index("occlusion masks from the flows"):hdr.index("gfl_flow_occlusion(const float* fwd")]
    res, args = _lib.SIGNATURES["gfl_flow_occlusion"]
    assert res is ctypes.c_int and len(args) == 12 and args[5] is ctypes.c_float and args[6] is ctypes.c_float


def test_refused_arguments_return_invalid_before_any_launch():
    from gflow_amd import _lib
    lib = _lib.load()
    nan = float("nan")
    for n, w, h, alpha, beta in ((1, 1, 40, 0.01, 0.5), (1, 40, 1, 0.01, 0.5), (0, 8, 8, 0.01, 0.5), (1, 8, 8, nan, 0.5),
                                 (1, 8, 8, 0.01, -0.1), (1, 8, 8, float("inf"), 0.5), (1, 8, 8, -1.0, 0.5),
                                 (1, 8, 8, 0.01, nan), (1, 1 << 15, (1 << 15) + 1, 0.01, 0.5), (1025, 1024, 1024, 0.01, 0.5),
                                 (1, 8, 8, 0.01, 0.5)):                       # (the last: null inputs)
        assert lib.gfl_flow_occlusion(None, None, n, w, h, alpha, beta, None, None, None, None, None) == -1


def test_a_stale_library_asks_for_a_rebuild(monkeypatch):
    from gflow_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "gfl_no_such_entry", (ctypes.c_int, []))
    with pytest.raises(RuntimeError, match="rebuild the library"):
        _lib.load()


# ------------------------------------------------------------------------------------------------- the Python layer, host
def test_argument_checks_and_no_cpu_fallback():
    from gflow_amd import occlusion as OC
    z = torch.zeros(8, 8, 2)
    for bad in ((torch.zeros(8, 8), torch.zeros(8, 8)), (torch.zeros(8, 8, 3), torch.zeros(8, 8, 3)),
                (z, torch.zeros(8, 9, 2)), (torch.zeros(1, 8, 2), torch.zeros(1, 8, 2)),
                (torch.zeros(0, 8, 8, 2), torch.zeros(0, 8, 8, 2))):
        with pytest.raises(ValueError):
            OC.flow_occlusion(*bad)
    for kw in (dict(alpha=float("nan")), dict(beta=-0.5), dict(alpha=float("inf"))):
        with pytest.raises(ValueError):
            OC.flow_occlusion(z, z, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            OC.flow_occlusion(z, z)


def _sequence_with_backward_flows(tmp_path, n=3, H=24, W=32):
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    sc = S._Scene(H, W, 0)
    sp = gio.write_sequence([sc.frame(k) for k in range(n)], str(tmp_path / "seq"))
    for k in range(1, n):
        gio.write_flow(os.path.join(sp + "_flow_unimatch", f"{k - 1:05d}_pred_bwd.flo"), sc.backward_flow(k).numpy())
    return sp


def test_sequence_paths_lists_the_backward_flows(tmp_path):
    from gflow_amd import io as gio
    sp = _sequence_with_backward_flows(tmp_path, n=4)
    p = gio.sequence_paths(sp)
    assert [f.name for f in p["flow"]] == ["00000_pred.flo", "00001_pred.flo", "00002_pred.flo"]
    assert [f.name for f in p["flow_bwd"]] == ["00000_pred_bwd.flo", "00001_pred_bwd.flo", "00002_pred_bwd.flo"]
    p = gio.sequence_paths(sp, frame_start=1, frame_range=2)
    assert [f.name for f in p["flow_bwd"]] == ["00001_pred_bwd.flo", "00002_pred_bwd.flo"] and len(p["flow"]) == 2


def test_load_sequence_occ_masks_option(tmp_path):
    from gflow_amd import io as gio
    sp = _sequence_with_backward_flows(tmp_path)
    a, b = gio.load_sequence(sp), gio.load_sequence(sp, occ_masks="files")
    assert "occ_mask" in a[1] and "occ_mask" not in a[0]
    for fa, fb in zip(a, b):
        assert sorted(fa) == sorted(fb)
        assert all(torch.equal(fa[k], fb[k]) if torch.is_tensor(fa[k]) else fa[k] == fb[k] for k in fa)
    with pytest.raises(ValueError):
        gio.load_sequence(sp, occ_masks="cv2")
    # without backward flows nothing is computed and no frame gets a mask: no device is needed
    for f in os.listdir(sp + "_flow_unimatch"):
        if f.endswith("_pred_bwd.flo"):
            os.remove(os.path.join(sp + "_flow_unimatch", f))
    assert not any("occ_mask" in fr for fr in gio.load_sequence(sp, occ_masks="flow"))


def test_cli_refuses_before_it_needs_a_device(tmp_path):
    from gflow_amd import occlusion as OC
    sp = _sequence_with_backward_flows(tmp_path)
    flows = sp + "_flow_unimatch"
    with pytest.raises(SystemExit, match="overwrite"):              # write_sequence left *_occ_bwd.png there
        OC.main(["--img_dir", sp])
    os.remove(os.path.join(flows, "00001_pred_bwd.flo"))
    with pytest.raises(SystemExit, match="2 forward flows.*1 backward"):
        OC.main(["--img_dir", sp, "--out", str(tmp_path / "elsewhere")])
    assert not os.path.exists(tmp_path / "elsewhere")


def test_write_masks_files_and_bytes(tmp_path):
    from PIL import Image
    from gflow_amd import occlusion as OC
    res = dict(occ=torch.tensor([[0, 255, 0], [255, 0, 0]], dtype=torch.uint8), occ_bwd=np.full((2, 3), 255, np.uint8))
    paths = OC.write_masks(res, str(tmp_path / "out"), "00003")
    assert [os.path.basename(p) for p in paths] == ["00003_occ.png", "00003_occ_bwd.png"]
    imgs = [Image.open(p) for p in paths]
    assert all(im.mode == "L" for im in imgs)
    np.testing.assert_array_equal(np.asarray(imgs[0]), res["occ"].numpy())
    assert (np.asarray(imgs[1]) == 255).all()
    with pytest.raises(FileExistsError):
        OC.write_masks(res, str(tmp_path / "out"), "00003")
    OC.write_masks(res, str(tmp_path / "out"), "00003", overwrite=True)


def test_fit_video_has_the_flag(capsys):
    from gflow_amd import fit_video
    with pytest.raises(SystemExit) as e:
        fit_video.main(["--make-occ-masks", "--help"])            # (parsed before a device is asked for)
    assert e.value.code == 0 and "--make-occ-masks" in capsys.readouterr().out
