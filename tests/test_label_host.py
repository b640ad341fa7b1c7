"""Object propagation without a device ("Object propagation"): the numpy restatement of the two kernels on
cases worked by hand, the shared GPU scene against the restatement alone, the entries' argument checks, the object-mask
reader and loader option, the recorder's refusals and the clip's score."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import flow_ref as FR
from tests import label_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_splats():
    """18 x 18 (2 x 2 tiles), both splats in tile 0, conic [1, 0, 1]: the near one at (8, 8), opacity 0.8, label 1; the far
    one at (10, 8), opacity 0.5, label 2"""
    rec = np.zeros((2, LR.REC), np.float32)
    rec[0, 0:6] = [8, 8, 1, 0, 1, 0.8]
    rec[1, 0:6] = [10, 8, 1, 0, 1, 0.5]
    rec[:, 9] = [1, 2]
    tr = np.zeros((4, 2), np.int32)
    tr[0] = (0, 2)
    return rec, np.arange(2, dtype=np.int32), tr


def test_label_frame_ref_on_two_overlapping_splats_worked_by_hand():
    rec, ids, tr = _two_splats()
    r = LR.label_frame_ref(rec, ids, tr, np.array([1, 2], np.uint8), 2, 3, 18, 18, min_weight=0.5)
    g = lambda d2: math.exp(-0.5 * d2)
    # (x, 8): the near splat's alpha is 0.8 g(dx^2), the far one's 0.5 g((x - 10)^2) behind T = 1 - that
    a1, a2 = 0.8, 0.5 * g(4)
    w1, w2 = a1, (1 - a1) * a2
    assert r["label"][8, 8] == 1
    np.testing.assert_allclose([r["acc"][1, 8, 8], r["acc"][2, 8, 8], r["den"][8, 8]], [w1, w2, w1 + w2], rtol=1e-6)
    np.testing.assert_allclose([r["conf"][8, 8], r["margin"][8, 8]], [w1 / (w1 + w2), w1 - w2], rtol=1e-6)
    a1, a2 = 0.8 * g(4), 0.5
    w1, w2 = a1, (1 - a1) * a2
    assert w1 + w2 >= 0.5 and r["label"][8, 10] == 2                  # the far splat wins where it is centred
    np.testing.assert_allclose([r["acc"][1, 8, 10], r["acc"][2, 8, 10]], [w1, w2], rtol=1e-6)
    a1, a2 = 0.8 * g(1), 0.5 * g(1)
    assert r["label"][8, 9] == 1
    np.testing.assert_allclose(r["den"][8, 9], a1 + (1 - a1) * a2, rtol=1e-6)
    # (12, 8): the near splat's alpha 0.8 g(16) is below 1 / 255 and skipped; the far one alone stays below min_weight
    assert 0.8 * g(16) < 1 / 255
    assert r["label"][8, 12] == LR.NONE and r["conf"][8, 12] == 0
    np.testing.assert_allclose(r["den"][8, 12], 0.5 * g(4), rtol=1e-6)
    assert r["acc"][0].max() == 0 and (r["label"][:, 16:] == LR.NONE).all() and not r["stopped"].any()
    # the same splats with the near one unlabelled: it adds nothing but still occludes
    u = LR.label_frame_ref(rec, ids, tr, np.array([255, 2], np.uint8), 2, 3, 18, 18, min_weight=0.05)
    np.testing.assert_allclose(u["den"][8, 8], (1 - 0.8) * 0.5 * g(4), rtol=1e-6)
    assert u["label"][8, 10] == 2 and u["acc"][1].max() == 0
    # rows beyond n_labels and labels >= K count as unlabelled
    v = LR.label_frame_ref(rec, ids, tr, np.array([1, 2], np.uint8), 1, 3, 18, 18, min_weight=0.05)
    assert v["acc"][2].max() == 0 and v["label"][8, 8] == 1
    k2 = LR.label_frame_ref(rec, ids, tr, np.array([1, 2], np.uint8), 2, 2, 18, 18, min_weight=0.05)
    assert k2["acc"].shape[0] == 2 and k2["label"][8, 10] == 1


def test_label_frame_ref_stops_before_adding():
    """fifteen splats of alpha 1/2 on one pixel: T = 2^-k exactly; 2^-13 >= T_MIN = 1e-4 is kept, 2^-14 is not -- the walk
    stops at the fourteenth splat without adding it"""
    rec = np.zeros((15, LR.REC), np.float32)
    rec[:, 0:6] = [8, 8, 1, 0, 1, 0.5]
    tr = np.zeros((4, 2), np.int32)
    tr[0] = (0, 15)
    labels = np.array([1] * 13 + [2, 2], np.uint8)
    r = LR.label_frame_ref(rec, np.arange(15, dtype=np.int32), tr, labels, 15, 3, 18, 18)
    assert r["stopped"][8, 8] and r["walked"][8, 8] == 14 and r["acc"][2, 8, 8] == 0 and r["label"][8, 8] == 1
    assert r["acc"][1, 8, 8] == 1 - 2.0 ** -13 and r["conf"][8, 8] == 1
    assert not r["stopped"][8, 12] and r["walked"][8, 12] == 15          # far from the centre nothing stops


def test_label_assign_ref_on_the_edge_rows():
    rec, m, labels, w, h = LR.assign_case()
    got = LR.label_assign_ref(rec, m, w, h, labels)
    want = labels.copy()
    want[13], want[14] = m[2, 3], m[5, 7]                                # (3.6, 2.7) and (7.5, 5.5) truncate, they do not round
    want[15], want[16] = m[7, 10], m[0, 0]
    want[17] = m[h - 2, w - 2]                                           # just inside the far border
    want[18] = m[3, 4]                                                   # a negative depth is not 0
    assert got.tolist() == want.tolist()
    assert (got[:13] == labels[:13]).all()                               # border, outside, NaN, depth 0, labelled, map 255
    assert m[3, 4] not in (3, 0) and got[9] == 3 and got[10] == 0


@pytest.mark.parametrize("K", [2, 5, 16])
def test_the_gpu_scene_holds_its_cases_and_float32_sums_keep_its_labels(K):
    """The scene tests/test_gpu_label.py runs, here through the oracle's front end, float32 class sums against float64 ones:
    what the GPU comparison may leave out, and that every case it asserts is in the scene."""
    s = LR.label_scene()
    fe = FR.front_end(s["xyz"], s["scale"], s["rotate"], s["opacity"], s["intr"], s["extr"], LR.W, LR.H)
    lab, n_labels = LR.scene_labels(len(fe["rec"]), K)
    args = (fe["rec"], fe["ids"], fe["tile_range"], lab, n_labels, K, LR.W, LR.H)
    r64 = LR.label_frame_ref(*args)
    r32 = LR.label_frame_ref(*args, dtype=np.float32)
    LR.compare(r32["label"], r32["conf"], r64, what=f"float32 sums, K = {K}")
    assert np.abs(r32["acc"] - r64["acc"]).max() < 2e-6
    lengths = fe["tile_range"][:, 1] - fe["tile_range"][:, 0]
    assert lengths.max() > 256 and r64["walked"].max() > 256            # a live pixel crosses the staging batch
    assert set(np.unique(r64["label"])) == set(range(K)) | {LR.NONE}
    assert r64["stopped"].sum() > 20 and (fe["depth"] == 0).sum() >= 5
    assert n_labels < len(fe["rec"]) and (lab == LR.NONE).sum() > 20 and ((lab >= K) & (lab != LR.NONE)).sum() >= 1
    uv = fe["rec"][:, 0:2]
    assert ((uv[:, 0] < 0) | (uv[:, 0] > LR.W) | (uv[:, 1] < 0) | (uv[:, 1] > LR.H))[fe["depth"] != 0].sum() >= 5


def test_entries_reject_bad_arguments_without_a_gpu():
    from gflow_amd import _lib
    lib = _lib.load()
    n, W, H = 4, 40, 24
    rec = torch.zeros(n, 12)                                             # (host memory: nothing is launched)
    ids, tr = torch.zeros(8, dtype=torch.int32), torch.zeros(6, 2, dtype=torch.int32)
    lab, out = torch.zeros(n, dtype=torch.uint8), torch.zeros(H, W, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert rec.data_ptr() % 16 == 0
    call = lambda **kw: lib.gfl_label_frame(*[{**dict(rec=p(rec), n=n, ids=p(ids), tr=p(tr), lab=p(lab), n_labels=n, K=3, W=W, H=H,
                                                      mw=0.5, unknown=255, out=p(out), conf=None, stream=None), **kw}[k]
                                              for k in ("rec", "n", "ids", "tr", "lab", "n_labels", "K", "W", "H", "mw", "unknown",
                                                        "out", "conf", "stream")])
    for bad in (dict(K=1), dict(K=17), dict(mw=0.0), dict(mw=1.5), dict(mw=float("nan")), dict(n_labels=n + 1),
                dict(n_labels=-1), dict(out=None), dict(W=0), dict(H=0), dict(W=16 * 16385, H=1), dict(n=-1, n_labels=0),
                dict(rec=None), dict(ids=None), dict(tr=None), dict(lab=None), dict(unknown=256),
                dict(rec=ctypes.c_void_p(rec.data_ptr() + 4))):
        assert call(**bad) == -1, bad
    assert lib.gfl_label_assign(None, 3, p(out), W, H, p(lab), None) == -1
    assert lib.gfl_label_assign(p(rec), 3, None, W, H, p(lab), None) == -1
    assert lib.gfl_label_assign(p(rec), 3, p(out), W, H, None, None) == -1
    assert lib.gfl_label_assign(p(rec), -1, p(out), W, H, p(lab), None) == -1
    assert lib.gfl_label_assign(p(rec), 3, p(out), 0, H, p(lab), None) == -1
    assert lib.gfl_label_assign(None, 0, None, W, H, None, None) == 0   # nothing to do is not an error
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert "object labels through a clip fit (additive within 312" in hdr
    assert "gfl_label_frame" in hdr[hdr.index("300 (round 5)"):hdr.index("#define GFL_VERSION")]      # the version comment


def _write_masks(tmp_path):
    from PIL import Image
    ids = np.zeros((20, 30), np.uint8)
    ids[2:9, 3:14], ids[10:19, 12:29] = 1, 2
    pal = Image.fromarray(ids, mode="P")
    pal.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * (253 * 3))
    pal.save(tmp_path / "pal.png")
    Image.fromarray((ids * 100).astype(np.uint8)).save(tmp_path / "grey.png")
    rgb = np.zeros((20, 30, 3), np.uint8)
    rgb[..., 2] = ids * 90                                               # set in one channel only
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    return ids


def test_read_object_mask(tmp_path):
    from gflow_amd import io as gio
    ids = _write_masks(tmp_path)
    got = gio.read_object_mask(tmp_path / "pal.png")
    assert got.dtype == torch.uint8 and got.shape == (20, 30) and np.array_equal(got.numpy(), ids)
    for name in ("grey.png", "rgb.png"):
        got = gio.read_object_mask(tmp_path / name)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), (ids > 0).astype(np.uint8)), name
        assert np.array_equal(got.numpy() > 0, gio.read_mask(tmp_path / name).numpy())
    for name, allowed in (("pal.png", {0, 1, 2}), ("grey.png", {0, 1}), ("rgb.png", {0, 1})):
        for resize in (10, 33):
            got = gio.read_object_mask(tmp_path / name, resize=resize)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (resize, int(resize * 30 / 20))
            assert set(np.unique(got.numpy())) == allowed, (name, resize)     # nearest neighbour: no id is invented
            assert tuple(got.shape) == tuple(gio.read_mask(tmp_path / name, resize=resize).shape)
    half = gio.read_object_mask(tmp_path / "pal.png", resize=10).numpy()
    assert half[2, 4] == 1 and half[7, 10] == 2 and half[0, 0] == 0


def test_write_id_maps_round_trip(tmp_path):
    """what --propagate-out writes: the prompt file's palette if it had one, grey ids otherwise, unknown pixels as 0"""
    from PIL import Image
    from gflow_amd import io as gio
    from gflow_amd import propagation as PG
    ids = _write_masks(tmp_path)
    maps = np.stack([ids, ids])
    maps[1, 0, 0:3] = PG.UNKNOWN
    palette = Image.open(tmp_path / "pal.png").getpalette()
    paths = PG.write_id_maps(str(tmp_path / "out" / "clip_0"), maps, ["00000", "00001"], palette)
    assert [os.path.basename(p) for p in paths] == ["00000.png", "00001.png"]
    first = Image.open(paths[0])
    assert first.mode == "P" and first.getpalette()[:9] == palette[:9]
    assert np.array_equal(gio.read_object_mask(paths[0]).numpy(), ids)
    want = np.where(maps[1] == PG.UNKNOWN, 0, maps[1])
    assert np.array_equal(gio.read_object_mask(paths[1]).numpy(), want)
    grey = PG.write_id_maps(str(tmp_path / "grey"), maps, ["a", "b"])
    assert Image.open(grey[1]).mode == "L" and np.array_equal(np.asarray(Image.open(grey[1])), want)


def test_load_sequence_object_masks(tmp_path):
    from PIL import Image
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    frames = S.make_clip(3, 48, 80, seed=2)
    seq = gio.write_sequence(frames, str(tmp_path / "clip"))
    os.makedirs(seq + "_mask")
    want = []
    for i in range(2):                                                   # the third frame has no annotation
        ids = np.zeros((48, 80), np.uint8)
        ids[5 + i:20, 10:30], ids[25:40, 40 + i:70] = 1, 2
        img = Image.fromarray(ids, mode="P")
        img.putpalette([0, 0, 0, 255, 0, 0, 0, 255, 0] + [0] * (253 * 3))
        img.save(os.path.join(seq + "_mask", f"{i:05d}.png"))
        want.append(ids)
    assert len(gio.sequence_paths(seq, frame_range=3)["objects"]) == 2
    plain = gio.load_sequence(seq, frame_range=3)
    assert len(plain) == 3 and all("object_mask" not in fr for fr in plain)
    none = gio.load_sequence(seq, frame_range=3, object_masks="none")
    assert [sorted(fr) for fr in none] == [sorted(fr) for fr in plain]
    back = gio.load_sequence(seq, frame_range=3, object_masks="files")
    assert [sorted(set(b) - set(a)) for a, b in zip(plain, back)] == [["object_mask"]] * 3
    for i in range(2):
        assert back[i]["object_mask"].dtype == torch.uint8 and np.array_equal(back[i]["object_mask"].numpy(), want[i])
    assert back[2]["object_mask"] is None
    for a, b in zip(plain, back):
        assert all(torch.equal(a[k], b[k]) for k in ("image", "depth", "flow", "move_mask"))
    small = gio.load_sequence(seq, frame_range=3, object_masks="files", resize=24)
    assert tuple(small[0]["object_mask"].shape) == tuple(small[0]["image"].shape[:2]) == (24, 40)
    assert set(np.unique(small[0]["object_mask"].numpy())) == {0, 1, 2}
    assert gio.load_sequence(seq, frame_range=1, object_masks="files")[0]["object_mask"] is not None
    with pytest.raises(ValueError, match="object_masks"):
        gio.load_sequence(seq, object_masks="palette")


def test_object_recorder_refuses_before_it_touches_a_device():
    from gflow_amd import propagation as PG
    ok = np.zeros((24, 40), np.int64)
    ok[3:9, 4:20] = 2
    make = lambda prompt=ok, **kw: PG.ObjectRecorder(**{**dict(n_frames=3, H=24, W=40, device="cuda", prompt=prompt), **kw})
    for prompt, message in ((np.where(ok > 0, 16, 0), "ids up to 15"), (ok[:, :39], "must be"), (np.zeros_like(ok), "no object"),
                            (ok.astype(np.float32), "integer ids"), (torch.from_numpy(ok)[None], "must be"), (-ok, r"\[0, 255\]")):
        with pytest.raises(ValueError, match=message):
            make(prompt)
    for kw in (dict(min_weight=0.0), dict(min_weight=1.5), dict(n_frames=0), dict(H=0)):
        with pytest.raises(ValueError):
            make(**kw)
    with pytest.raises(ValueError, match="16384 tiles"):
        make(np.ones((16, 16 * 16385), np.uint8), H=16, W=16 * 16385)
    from gflow_amd.clip_fit import fit_clips_concurrent
    with pytest.raises(ValueError, match="propagate needs one entry per clip"):
        fit_clips_concurrent([[], []], "cuda", propagate=[ok])


def test_evaluate_on_hand_made_counts():
    from gflow_amd import propagation as PG
    from gflow_amd import segmentation as SG
    from gflow_amd.clip_reduce import reduce_davis
    # (inter, uni, n_fg, n_gt, fg_match, gt_match) per (frame, object): frame 0 carries the prompt and is not scored
    counts = np.zeros((3, 2, 6), np.int64)
    counts[1, 0] = (50, 100, 10, 10, 5, 10)          # J 0.5, p 0.5, r 1   -> F 2/3
    counts[1, 1] = (30, 30, 8, 8, 8, 8)              # J 1,   F 1
    counts[2, 0] = (70, 100, 10, 20, 10, 10)         # J 0.7, p 1, r 0.5   -> F 2/3
    counts[2, 1] = (0, 40, 0, 12, 0, 0)              # J 0,   no predicted boundary: p 1, r 0 -> F 0
    J, F, JF = (a.reshape(3, 2) for a in SG.scores_from_counts(counts.reshape(-1, 6)))
    scored = np.array([False, True, True])
    J[0], F[0], JF[0] = 0, 0, 0
    res = dict(J=J, F=F, JF=JF, scored=scored, counts=counts,
               flat=dict(J=J.reshape(-1), F=F.reshape(-1), JF=JF.reshape(-1), valid=np.repeat(scored, 2)))
    ev = PG.evaluate(res)
    assert ev["frames_scored"] == 2 and ev["pairs_scored"] == 4
    assert ev["J"] == pytest.approx((0.5 + 1 + 0.7 + 0) / 4) and ev["F"] == pytest.approx((2 / 3 + 1 + 2 / 3 + 0) / 4)
    assert ev["J&F"] == pytest.approx((ev["J"] + ev["F"]) / 2)
    assert ev["per_object"][0]["J"] == pytest.approx(0.6) and ev["per_object"][1]["J"] == pytest.approx(0.5)
    assert ev["per_object"][0]["F"] == pytest.approx(2 / 3) and ev["per_object"][1]["J&F"] == pytest.approx(0.5)
    # the flattened form is what the clip reduction already takes
    flat = SG.evaluate(res["flat"])
    assert flat["frames_scored"] == 4 and flat["J"] == pytest.approx(ev["J"]) and flat["J&F"] == pytest.approx(ev["J&F"])
    line = reduce_davis({0: res["flat"]})
    assert line["J"] == pytest.approx(ev["J"]) and line["clips"] == 1
    empty = PG.evaluate(dict(J=np.zeros((2, 1)), F=np.zeros((2, 1)), JF=np.zeros((2, 1)), scored=np.zeros(2, bool)))
    assert empty["frames_scored"] == 0 and math.isnan(empty["J"]) and math.isnan(empty["per_object"][0]["F"])
