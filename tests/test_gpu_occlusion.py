"""Occlusion masks from the flows on the device (``-m gpu``; gfl_flow_occlusion, gflow_amd/occlusion.py) through the C ABI,
every output pre-filled with garbage, against the float64 restatement (tests/occ_ref.py) on the scenes of
tests/test_occlusion_host.py.

Bounds.  DIFF_REL: |d_device - d_ref| <= 2e-5 (1 + d_ref) -- about ten float32 roundings (6e-8 each, relative) of values of
at most 10 px, with a factor of five of margin.  The masks must be equal outside the band |d_ref - thr_ref| <=
1e-4 (1 + thr_ref) (test_occlusion_host.band), where float32 may decide either way, and the band may hold at most BAND_SHARE
of a case's pixels: a property of the scene and the restatement alone (per direction it holds 0 or 1 pixels on these scenes
and 2 of 409920 at 480 x 854)."""
import os

import numpy as np
import pytest
import torch

from tests import occ_ref as R
from tests.test_occlusion_host import SYNTHETIC, band, constant_pair, iou, scene_case, synthetic_pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIFF_REL = 2e-5
BAND_SHARE = 0.005
OUTPUTS = ("diff", "diff_bwd", "occ", "occ_bwd")
GARBAGE_F32, GARBAGE_U8 = -1234.5678, 0xA5
SIZES = [(2, 2), (5, 7), (33, 47), (97, 131)]


def _occ(fwd, bwd, outputs=OUTPUTS, alpha=0.01, beta=0.5):
    """gfl_flow_occlusion through the C ABI on (H, W, 2) or (P, H, W, 2); outputs not asked for are passed as NULL.
    Returns (status, dict of numpy arrays)."""
    from gflow_amd import _lib as L
    lib = L.load()
    fwd, bwd = (np.ascontiguousarray(f, dtype=np.float32) for f in (fwd, bwd))
    lead = fwd.shape[:-1]
    h, w = lead[-2:]
    p = lead[0] if len(lead) == 3 else 1
    f, b = torch.tensor(fwd, device=DEV), torch.tensor(bwd, device=DEV)
    bufs = {k: torch.full(lead, GARBAGE_F32 if k.startswith("diff") else GARBAGE_U8,
                          dtype=torch.float32 if k.startswith("diff") else torch.uint8, device=DEV) for k in outputs}
    rc = lib.gfl_flow_occlusion(L.ptr(f), L.ptr(b), p, w, h, alpha, beta, *(L.ptr(bufs.get(k)) for k in OUTPUTS), L.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def _compare(got, ref, what):
    """the four outputs of one pair against the restatement; prints the figures before it asserts"""
    n = ref["thr"].size
    for key in ("", "_bwd"):
        d, m = got["diff" + key], got["occ" + key]
        assert d.dtype == np.float32 and m.dtype == np.uint8 and np.isin(m, (0, 255)).all()
        rel = float((np.abs(d.astype(np.float64) - ref["diff" + key]) / (1.0 + ref["diff" + key])).max())
        bd = band(ref, key)
        differ = (m != ref["occ" + key]) & ~bd
        print(what, key or "_fwd", "rel", rel, "band", int(bd.sum()), "of", n, "occluded", float((ref["occ" + key] != 0).mean()),
              "masks differ outside the band", int(differ.sum()))
        assert rel <= DIFF_REL
        assert bd.sum() <= BAND_SHARE * n
        assert not differ.any()
        unknown = ~ref["known" + key]
        assert not d[unknown].any() and not m[unknown].any()


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("H,W", SIZES + [(480, 854)])
def test_parity_with_the_restatement(H, W):
    fwd, bwd, ref = scene_case(H, W, 0)
    rc, got = _occ(fwd, bwd)
    assert rc == 0
    _compare(got, ref, f"{H}x{W}")
    assert ref["occ"].any() and ref["occ_bwd"].any()


def test_parity_of_a_batch_of_two_pairs():
    cases = [scene_case(97, 131, 1), scene_case(97, 131, 2)]
    assert not np.array_equal(cases[0][0], cases[1][0])
    rc, got = _occ(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
    assert rc == 0
    for p, c in enumerate(cases):
        _compare({k: v[p] for k, v in got.items()}, c[2], f"pair {p}")
        alone = _occ(c[0], c[1])[1]                               # a pair's outputs do not depend on its place in a batch
        assert all(np.array_equal(got[k][p], alone[k]) for k in OUTPUTS)


# ------------------------------------------------------------------------------------------------------ edge behaviour
def test_known_answer_constant_flow_exactly():
    H, W = 9, 12
    fwd, bwd = constant_pair(H, W, (3.0, -2.0))
    rc, got = _occ(fwd, bwd)
    assert rc == 0
    yy, xx = np.mgrid[0:H, 0:W]
    out_f = (xx + 3 > W - 1) | (yy - 2 < 0)
    out_b = (xx - 3 < 0) | (yy + 2 > H - 1)
    assert np.array_equal(got["occ"], np.where(out_f, 255, 0)) and np.array_equal(got["occ_bwd"], np.where(out_b, 255, 0))
    assert not got["diff"][~out_f].any() and not got["diff_bwd"][~out_b].any()
    np.testing.assert_allclose(got["diff"][out_f], np.hypot(3.0, 2.0), rtol=2e-7)
    np.testing.assert_allclose(got["diff_bwd"][out_b], np.hypot(3.0, 2.0), rtol=2e-7)
    _compare(got, R.flow_occlusion(fwd, bwd), "constant")


def test_known_answer_half_pixel_exactly():
    rc, got = _occ(*constant_pair(9, 12, (0.5, 0.0)))
    assert rc == 0
    assert not got["diff"][:, :-1].any() and (got["diff"][:, -1] == 0.25).all()
    assert not got["diff_bwd"][:, 1:].any() and (got["diff_bwd"][:, 0] == 0.25).all()
    assert not got["occ"].any() and not got["occ_bwd"].any()


def test_samples_on_the_last_column_and_just_outside():
    """fwd.x = 2 and bwd.x = -2 exactly, the y components fractional: column W - 3 samples exactly column W - 1 (the corner
    at W is outside), W - 2 lands on W and W - 1 on W + 1 (nothing inside); backwards column 2 lands on 0, column 1 on -1
    (only the corner at 0, weight 0) and column 0 on -2."""
    H, W = 7, 70                                                   # (two workgroups across)
    rng = np.random.default_rng(5)
    fwd = np.stack([np.full((H, W), 2.0), rng.uniform(-0.4, 0.4, (H, W))], axis=-1).astype(np.float32)
    bwd = np.stack([np.full((H, W), -2.0), rng.uniform(-0.4, 0.4, (H, W))], axis=-1).astype(np.float32)
    rc, got = _occ(fwd, bwd)
    assert rc == 0
    ref = R.flow_occlusion(fwd, bwd)
    _compare(got, ref, "edges")
    norm = lambda v: np.sqrt(v[..., 0].astype(np.float64) ** 2 + v[..., 1].astype(np.float64) ** 2)
    for d, flow, cols in ((got["diff"], fwd, (W - 2, W - 1)), (got["diff_bwd"], bwd, (1, 0))):
        for c in cols:                                             # nothing sampled: d = |own flow|, and occluded
            np.testing.assert_allclose(d[:, c], norm(flow[:, c]), rtol=3e-7)
    assert (got["occ"][:, W - 2:] == 255).all() and (got["occ_bwd"][:, :2] == 255).all()
    assert (got["diff"][:, W - 3] < 1.0).all() and (got["diff_bwd"][:, 2] < 1.0).all()      # (sampled: the x parts cancel)


def test_huge_and_nan_flows_are_unknown_with_their_poisoned_neighbours():
    fwd, bwd = (f.copy() for f in constant_pair(8, 10, (1.0, 0.0)))
    fwd[3, 4] = (np.nan, 0.0)
    bwd[5, 6] = (1e30, 0.0)
    bwd[0, 9] = (0.0, -np.inf)
    rc, got = _occ(fwd, bwd)
    assert rc == 0
    ref = R.flow_occlusion(fwd, bwd)
    # the NaN and the infinity poison at weight 0 too (0 * inf = NaN), the 1e30 at weight 1 only (0 * 1e30 = 0)
    for key, unknown in (("", [(3, 4), (5, 6), (5, 5), (0, 9), (0, 8), (0, 7)]),
                         ("_bwd", [(3, 4), (3, 5), (2, 4), (2, 5), (5, 6), (0, 9)])):
        want = np.zeros((8, 10), bool)
        want[tuple(zip(*unknown))] = True
        assert np.array_equal(~ref["known" + key], want), key
        assert not got["diff" + key][want].any() and not got["occ" + key][want].any()
        assert np.isfinite(got["diff" + key]).all()
    _compare(got, ref, "unknown")
    # a NaN is read at weight 0 as well: (2, 5) and the row above sample (2, 7) with t = 0
    fwd, bwd = constant_pair(8, 10, (1.0, 0.0))
    bwd = bwd.copy()
    bwd[2, 7] = np.nan
    got = _occ(fwd, bwd)[1]
    for y, x in ((2, 6), (2, 5), (1, 6), (1, 5), (2, 7)):
        assert got["diff"][y, x] == 0 and got["occ"][y, x] == 0
    assert got["diff"][2, 4] == 0 and got["occ"][2, 4] == 0 and got["occ"][3, 6] == 0 and got["occ"][2, 9] == 255
    _compare(got, R.flow_occlusion(fwd, bwd), "nan")


def test_each_output_may_be_null_and_calls_repeat_bit_for_bit():
    fwd, bwd, _ = scene_case(33, 47, 0)
    rc, full = _occ(fwd, bwd)
    assert rc == 0
    rc, again = _occ(fwd, bwd)
    assert rc == 0 and all(np.array_equal(full[k].view(np.uint8), again[k].view(np.uint8)) for k in OUTPUTS)
    for left_out in OUTPUTS:
        rc, part = _occ(fwd, bwd, outputs=tuple(k for k in OUTPUTS if k != left_out))
        assert rc == 0 and sorted(part) == sorted(k for k in OUTPUTS if k != left_out)
        assert all(np.array_equal(part[k], full[k]) for k in part), left_out
    for only in OUTPUTS:
        rc, part = _occ(fwd, bwd, outputs=(only,))
        assert rc == 0 and np.array_equal(part[only], full[only]), only
    assert _occ(fwd, bwd, outputs=())[0] == 0
    # other constants: beta = 0 marks nearly everything, a large beta nothing
    assert (_occ(fwd, bwd, alpha=0.0, beta=0.0)[1]["occ"] == 255).mean() > 0.99
    assert not _occ(fwd, bwd, alpha=0.0, beta=100.0)[1]["occ"].any()
    assert _occ(fwd, bwd, beta=float("nan"))[0] == -1 and _occ(fwd, bwd, alpha=-1.0)[0] == -1


# ------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_shapes_dtypes_and_devices():
    from gflow_amd import occlusion as OC
    fwd, bwd, ref = scene_case(33, 47, 0)
    want = _occ(fwd, bwd)[1]
    one = OC.flow_occlusion(torch.tensor(fwd), bwd.copy(), maps=True)               # (a host tensor and an array)
    assert sorted(one) == sorted(OUTPUTS)
    for k in OUTPUTS:
        assert one[k].is_cuda and tuple(one[k].shape) == (33, 47)
        assert one[k].dtype == (torch.float32 if k.startswith("diff") else torch.uint8)
        assert np.array_equal(one[k].cpu().numpy(), want[k]), k
    masks = OC.flow_occlusion(torch.tensor(fwd, device=DEV), torch.tensor(bwd, device=DEV))
    assert sorted(masks) == ["occ", "occ_bwd"] and all(torch.equal(masks[k], one[k]) for k in masks)
    f2, b2, _ = scene_case(33, 47, 1)
    batch = OC.flow_occlusion(np.stack([fwd, f2]), np.stack([bwd, b2]), maps=True)
    for k in OUTPUTS:
        assert batch[k].is_cuda and tuple(batch[k].shape) == (2, 33, 47) and batch[k].dtype == one[k].dtype
        assert torch.equal(batch[k][0], one[k])
    assert not torch.equal(batch["occ"][1], batch["occ"][0])
    single = OC.flow_occlusion(fwd[None].copy(), bwd[None].copy())
    assert tuple(single["occ"].shape) == (1, 33, 47) and torch.equal(single["occ"][0], one["occ"])
    loose = OC.flow_occlusion(fwd.copy(), bwd.copy(), alpha=0.0, beta=3.0)
    assert loose["occ"].sum() < one["occ"].sum()


def test_clip_occ_masks_fills_the_later_frames():
    from gflow_amd import occlusion as OC
    from gflow_amd import synthetic as S
    sc = S._Scene(48, 64, 0)
    frames = [sc.frame(k) for k in range(3)]
    before = frames[0]["occ_mask"]
    OC.clip_occ_masks(frames, [sc.backward_flow(1), sc.backward_flow(2)])
    assert frames[0]["occ_mask"] is before
    for k in (1, 2):
        m = frames[k]["occ_mask"]
        assert m.dtype == torch.float32 and tuple(m.shape) == (48, 64, 1) and m.device == frames[k]["image"].device
        want = OC.flow_occlusion(frames[k - 1]["flow"], sc.backward_flow(k))["occ_bwd"]
        assert torch.equal(m[..., 0], (want != 0).float().cpu()) and set(m.unique().tolist()) <= {0.0, 1.0}
    untouched = [sc.frame(k) for k in range(3)]
    OC.clip_occ_masks(untouched, [None, sc.backward_flow(2)])
    assert untouched[1]["occ_mask"].dtype == torch.bool and untouched[2]["occ_mask"].dtype == torch.float32


@pytest.mark.parametrize("cam_step,k", SYNTHETIC)
def test_synthetic_occlusion_mask_through_the_kernel(cam_step, k):
    from gflow_amd import occlusion as OC
    fwd, bwd, occ = synthetic_pair(cam_step, k)
    got = OC.flow_occlusion(torch.tensor(fwd), torch.tensor(bwd))["occ_bwd"].cpu().numpy()
    ref = R.flow_occlusion(fwd, bwd)
    score = iou(got, occ)
    print(cam_step, k, "IoU", score, "of the restatement", iou(ref["occ_bwd"], occ))
    assert score >= 0.88
    assert not ((got != ref["occ_bwd"]) & ~band(ref, "_bwd")).any()


# ------------------------------------------------------------------------------------------------------------ round trip
def test_masks_written_by_the_cli_equal_masks_computed_by_the_loader(tmp_path):
    from PIL import Image
    from gflow_amd import io as gio
    from gflow_amd import occlusion as OC
    from gflow_amd import synthetic as S
    sc = S._Scene(48, 64, 0)
    sp = gio.write_sequence([sc.frame(k) for k in range(3)], str(tmp_path / "seq"))
    flows = sp + "_flow_unimatch"
    for k in (1, 2):
        gio.write_flow(os.path.join(flows, f"{k - 1:05d}_pred_bwd.flo"), sc.backward_flow(k).numpy())
    with pytest.raises(SystemExit, match="overwrite"):             # write_sequence's own *_occ_bwd.png are in the way
        OC.main(["--img_dir", sp])
    assert OC.main(["--img_dir", sp + "/", "--overwrite"]) == 0
    assert sorted(f for f in os.listdir(flows) if f.endswith(".png")) == ["00000_occ.png", "00000_occ_bwd.png",
                                                                          "00001_occ.png", "00001_occ_bwd.png"]
    for k in (0, 1):
        want = OC.flow_occlusion(gio.read_flow(os.path.join(flows, f"{k:05d}_pred.flo")), sc.backward_flow(k + 1))
        for key in ("occ", "occ_bwd"):
            im = Image.open(os.path.join(flows, f"{k:05d}_{key}.png"))
            assert im.mode == "L" and np.array_equal(np.asarray(im), want[key].cpu().numpy()), (k, key)
    for resize in (None, 32):
        a = gio.load_sequence(sp, resize=resize, occ_masks="files")
        b = gio.load_sequence(sp, resize=resize, occ_masks="flow")
        assert len(a) == len(b) == 2 and "occ_mask" in a[1] and "occ_mask" not in b[0]
        for fa, fb in zip(a, b):
            assert sorted(fa) == sorted(fb)
            for key in fa:
                same = torch.equal(fa[key], fb[key]) if torch.is_tensor(fa[key]) else fa[key] == fb[key]
                assert same, (resize, key)
        m = b[1]["occ_mask"]
        assert m.dtype == torch.float32 and not m.is_cuda and m.shape[2] == 1 and m.shape[:2] == b[1]["image"].shape[:2]
        assert m.any()
    with pytest.raises(SystemExit, match="overwrite"):             # a second run refuses
        OC.main(["--img_dir", sp])
    other = str(tmp_path / "elsewhere")
    assert OC.main(["--img_dir", sp, "--out", other, "--beta", "0.25"]) == 0 and len(os.listdir(other)) == 4
