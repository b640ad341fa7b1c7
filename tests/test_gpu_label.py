"""Object propagation on the device (``-m gpu``; INTEGRATION.md, "Object propagation"): gfl_label_frame against its float64
restatement (tests/label_ref.py) on the shared 40 x 24 scene, gfl_label_assign exactly, and the masks of one and of two
objects through a three-frame clip fit on both paths."""
import functools

import numpy as np
import pytest
import torch

from tests import flow_ref as FR
from tests import label_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = LR.W, LR.H


# --------------------------------------------------------------------------------------------------------- the kernel
@functools.lru_cache(maxsize=None)
def _state():
    """the shared scene through the five operators on the device: (rec, n, ids, tile_range) tensors and host copies"""
    from gflow_amd import flow as FL
    s = LR.label_scene()
    d = lambda k: s[k].to(DEV)
    group = [d("xyz"), d("scale"), d("rotate"), d("opacity"), d("rgb"), d("intr"), d("extr"), 0.0, W, H]
    with torch.no_grad():
        rec, n, ids, tr = FL.operator_state(group)
    return dict(rec=rec, n=n, ids=ids.contiguous(), tr=tr.contiguous(), rec_h=rec.cpu().numpy(), ids_h=ids.cpu().numpy(),
                tr_h=tr.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _reference(K):
    st = _state()
    lab, n_labels = LR.scene_labels(st["n"], K)
    return lab, n_labels, LR.label_frame_ref(st["rec_h"], st["ids_h"], st["tr_h"], lab, n_labels, K, W, H)


def _label_frame(rec, n, ids, tr, lab, n_labels, K, conf=True, unknown=LR.NONE, min_weight=0.5):
    from gflow_amd import _lib as L
    out = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    cf = torch.full((H, W), -1.0, dtype=torch.float32, device=DEV) if conf else None
    labels = None if lab is None else torch.from_numpy(np.asarray(lab, np.uint8)).to(DEV)
    L.check(L.load().gfl_label_frame(L.ptr(rec), n, L.ptr(ids), L.ptr(tr), L.ptr(labels), n_labels, K, W, H, min_weight, unknown,
                                     L.ptr(out), L.ptr(cf), L.stream()), "label frame")
    return out.cpu().numpy(), None if cf is None else cf.cpu().numpy()


@pytest.mark.parametrize("K", [2, 5, 16])
def test_label_frame_matches_the_float64_restatement(K):
    st = _state()
    lab, n_labels, ref = _reference(K)
    # the scene holds its cases: every class and unknown pixels in the map, pixels at the T_MIN stop, a list that crosses the
    # staging batch with pixels still walking, rows outside the image and behind the camera, unlabelled rows of every kind
    assert st["n"] == LR.N_FAINT + LR.N_OPAQUE + LR.N_REST
    assert set(np.unique(ref["label"])) == set(range(K)) | {LR.NONE}
    assert ref["stopped"].sum() > 20 and ref["walked"].max() > 256
    assert (st["rec_h"][:, 9] == 0).sum() >= 5 and n_labels < st["n"]
    assert (lab == LR.NONE).sum() > 20 and ((lab >= K) & (lab != LR.NONE)).sum() >= 1
    got, conf = _label_frame(st["rec"], st["n"], st["ids"], st["tr"], lab, n_labels, K)
    LR.compare(got, conf, ref, what=f"K = {K}")
    assert ((conf == 0) == (got == LR.NONE)).all() and conf.max() <= 1.0
    # the same inputs give the same bytes, with and without the confidence map
    again, conf2 = _label_frame(st["rec"], st["n"], st["ids"], st["tr"], lab, n_labels, K)
    alone, _ = _label_frame(st["rec"], st["n"], st["ids"], st["tr"], lab, n_labels, K, conf=False)
    assert got.tobytes() == again.tobytes() == alone.tobytes() and conf.tobytes() == conf2.tobytes()


def test_label_frame_with_the_lists_anywhere_in_ids():
    K = 5
    st = _state()
    lab, n_labels, ref = _reference(K)
    ids2, tr2 = FR.shuffled_lists(st["ids_h"], st["tr_h"], seed=4)
    assert len(ids2) > 2 * len(st["ids_h"]) and (tr2 != st["tr_h"]).any()
    got, conf = _label_frame(st["rec"], st["n"], torch.from_numpy(ids2).to(DEV), torch.from_numpy(tr2).to(DEV), lab, n_labels, K)
    LR.compare(got, conf, ref, what="relocated lists")
    straight, conf_s = _label_frame(st["rec"], st["n"], st["ids"], st["tr"], lab, n_labels, K)
    assert got.tobytes() == straight.tobytes() and conf.tobytes() == conf_s.tobytes()


def test_label_frame_without_splats_and_with_another_unknown():
    st = _state()
    got, conf = _label_frame(None, 0, None, None, None, 0, 3)
    assert (got == LR.NONE).all() and (conf == 0).all()
    got, _ = _label_frame(None, 0, None, None, None, 0, 3, unknown=9, conf=False)
    assert (got == 9).all()
    # no labelled row at all: the splats occlude, nobody votes
    got, conf = _label_frame(st["rec"], st["n"], st["ids"], st["tr"], None, 0, 2)
    assert (got == LR.NONE).all() and (conf == 0).all()
    # min_weight moves pixels between a label and unknown exactly as the restatement says
    lab, n_labels, ref = _reference(5)
    lo = LR.label_frame_ref(st["rec_h"], st["ids_h"], st["tr_h"], lab, n_labels, 5, W, H, min_weight=0.05)
    got, conf = _label_frame(st["rec"], st["n"], st["ids"], st["tr"], lab, n_labels, 5, min_weight=0.05)
    LR.compare(got, conf, lo, min_weight=0.05, what="min_weight 0.05")
    assert (lo["label"] != LR.NONE).sum() > (ref["label"] != LR.NONE).sum()


def test_label_assign_matches_the_restatement_exactly():
    from gflow_amd import _lib as L
    rec, m, labels, w, h = LR.assign_case()
    want = LR.label_assign_ref(rec, m, w, h, labels)
    assert (want != labels).sum() == 6
    d = lambda a: torch.from_numpy(a).to(DEV)
    rec_d, m_d, lab_d = d(rec), d(m), d(labels)
    L.check(L.load().gfl_label_assign(L.ptr(rec_d), len(rec), L.ptr(m_d), w, h, L.ptr(lab_d), L.stream()), "label assign")
    assert lab_d.cpu().numpy().tolist() == want.tolist()
    # more than one workgroup, rows of the shared scene on a map of its size; only the first n rows are touched
    st = _state()
    n = st["n"]
    rng = np.random.default_rng(2)
    big_map = rng.integers(0, 6, (H, W)).astype(np.uint8)
    big_map[rng.random((H, W)) < 0.1] = LR.NONE
    before = rng.integers(0, 6, n + 7).astype(np.uint8)
    before[rng.random(n + 7) < 0.6] = LR.NONE
    want = np.concatenate([LR.label_assign_ref(st["rec_h"][:n], big_map, W, H, before[:n]), before[n:]])
    assert 50 < (want != before).sum() < n
    lab_d = d(before)
    L.check(L.load().gfl_label_assign(L.ptr(st["rec"]), n, L.ptr(d(big_map)), W, H, L.ptr(lab_d), L.stream()), "label assign")
    assert lab_d.cpu().numpy().tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------------ through a fit
FH, FW, N0 = 96, 128, 1500
# the stage settings of test_mask_prompt_points_and_their_propagation_match_the_restatement (tests/test_gpu_frame_state.py)
CFG = dict(num_points=N0, iterations_first=40, lr=4e-3, lambda_var=10.0, densify_interval=15, densify_times=1,
           iterations_camera=15, lr_camera_after=5e-4, iterations_after=30, lr_after=1e-3, lambda_still=10.0, lambda_flow=0.01,
           densify_interval_after=20, densify_times_after=1, lambda_depth=1e-2)


def _halves(move_mask):
    """the disc split at its centroid column: ids 1 (left) and 2 (right), (H, W) uint8"""
    m = np.asarray(move_mask, bool)
    cols = np.nonzero(m)[1]
    x = np.arange(m.shape[1])[None, :]
    return np.where(m, np.where(x < cols.mean(), 1, 2), 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _fit(fused, objects):
    """(frames, truth per frame, fit_clip's dict) of the three-frame clip; ``objects`` 0: no propagation"""
    from gflow_amd import synthetic as S
    from gflow_amd.fit_video import fit_clip
    frames = S.make_clip(3, FH, FW, seed=3)
    truth = [fr["move_mask"].numpy().astype(np.uint8) if objects < 2 else _halves(fr["move_mask"].numpy()) for fr in frames]
    if objects:
        for fr, t in zip(frames, truth):
            fr["object_mask"] = torch.from_numpy(t)
    out = fit_clip(frames, DEV, CFG, fused=fused, seed=0, propagate=torch.from_numpy(truth[0]) if objects else None)
    torch.cuda.synchronize()
    return frames, truth, out


def _check_shapes(p, K):
    T = 3
    n = len(p["labels"])
    assert p["maps"].shape == (T, FH, FW) and p["maps"].dtype == np.uint8 and p["labels"].dtype == np.uint8
    assert p["n_objects"] == K - 1 and p["rows"].tolist() == sorted(p["rows"].tolist()) and p["rows"][-1] == n
    assert set(np.unique(p["maps"])) <= set(range(K)) | {255} and set(np.unique(p["labels"])) <= set(range(K)) | {255}
    assert p["counts"].shape == (T, K - 1, 6) and p["counts"].dtype == np.int64
    for k in ("J", "F", "JF"):
        assert p[k].shape == (T, K - 1) and (p[k] >= 0).all() and (p[k] <= 1).all()
        assert p["flat"][k].shape == (T * (K - 1),) and (p[k][0] == 0).all()
    assert p["scored"].tolist() == [False, True, True] and p["flat"]["valid"].tolist() == [False] * (K - 1) + [True] * (2 * (K - 1))
    assert (p["counts"][0] == 0).all() and (p["counts"][1:, :, 1] > 0).all()
    # the label vector has grown with the densification events, and appended rows have inherited labels
    assert p["rows"][0] >= N0 and n > p["rows"][0]
    assert (p["labels"][p["rows"][0]:] != 255).sum() > 0


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "operators"])
def test_one_object_follows_the_disc_through_a_fit(fused):
    from gflow_amd import propagation as PG
    frames, truth, out = _fit(fused, 1)
    p = out["propagation"]
    _check_shapes(p, 2)
    for i in (1, 2):
        seg, gt = p["maps"][i] == 1, truth[i] > 0
        inside, outside = seg[gt].mean(), seg[~gt].mean()
        print(f"frame {i} ({'fused' if fused else 'operators'}): object covers {inside:.3f} of the disc, {outside:.3f} of the rest; "
              f"J {p['J'][i, 0]:.3f} F {p['F'][i, 0]:.3f}; unknown {float((p['maps'][i] == 255).mean()):.3f}")
        assert inside > 0.6 and outside < 0.15, (i, inside, outside)
    ev = PG.evaluate(p)
    assert ev["frames_scored"] == 2 and 0 <= ev["J&F"] <= 1 and len(ev["per_object"]) == 1
    # the prompt frame's own map reproduces the prompt (kept, not scored)
    assert (p["maps"][0] == 1)[truth[0] > 0].mean() > 0.6


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "operators"])
def test_two_objects_keep_their_halves_through_a_fit(fused):
    frames, truth, out = _fit(fused, 2)
    p = out["propagation"]
    _check_shapes(p, 3)
    assert (p["labels"] == 1).sum() > 0 and (p["labels"] == 2).sum() > 0
    for i in (1, 2):
        m = p["maps"][i]
        for own, other in ((1, 2), (2, 1)):
            half = truth[i] == own
            share_own, share_other = (m[half] == own).mean(), (m[half] == other).mean()
            print(f"frame {i}, half {own}: own id {share_own:.3f}, the other id {share_other:.3f}")
            assert share_own > share_other, (i, own, share_own, share_other)
        seg, gt = (m == 1) | (m == 2), truth[i] > 0
        assert seg[gt].mean() > 0.6 and seg[~gt].mean() < 0.15, (i, seg[gt].mean(), seg[~gt].mean())


def test_a_fit_without_propagate_has_no_such_key():
    _, _, out = _fit(True, 0)
    assert "propagation" not in out
    _, _, with_it = _fit(True, 1)
    assert sorted(set(with_it) - set(out)) == ["propagation"]
    # the option adds one forward per frame on the second engine and no iteration
    assert with_it["iterations"] == out["iterations"] and with_it["rasterisations"] == out["rasterisations"] + 3
