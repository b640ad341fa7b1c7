"""CPU: the TAP-Vid metric, the query extraction and the nearest-centre restatement against fixtures captured from the
reference (tests/golden/tapvid.npz, make_tapvid_golden.py); the frame-loop restatement on a hand-worked case; the
synthetic ground truth; query validation; the tracking.pkl round trip; fit_video.reduce_tapvid over clips."""
import math
import os

import numpy as np
import pytest
import torch

from gflow_amd import fit_video as FV
from gflow_amd import synthetic as S
from gflow_amd import tracking as TK
from tests import tracking_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tapvid.npz")
KEYS = ["occlusion_accuracy"] + [f"pts_within_{t}" for t in (1, 2, 4, 8, 16)] + [f"jaccard_{t}" for t in (1, 2, 4, 8, 16)] \
    + ["average_jaccard", "average_pts_within_thresh"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_tapvid_metrics_match_the_reference(gold):
    n = int(gold["n_metric_cases"])
    assert n == 12
    saw_nan = False
    for c in range(n):
        p = f"m{c}_"
        mode = "first" if int(gold[p + "mode"]) == 0 else "strided"
        m = TK.tapvid_metrics(gold[p + "query_points"], gold[p + "gt_occluded"], gold[p + "gt_tracks"],
                              gold[p + "pred_occluded"], gold[p + "pred_tracks"], mode, trackwise=bool(gold[p + "trackwise"]))
        assert sorted(m) == sorted(KEYS)
        for k in KEYS:
            want = gold[p + "out_" + k]
            assert m[k].shape == want.shape, (c, k)
            np.testing.assert_allclose(m[k], want, rtol=0, atol=1e-12, equal_nan=True, err_msg=f"case {c} {k}")
            assert (np.isnan(m[k]) == np.isnan(want)).all()
            saw_nan |= bool(np.isnan(want).any())
    assert saw_nan                                  # (the no-visible-point video)
    with pytest.raises(ValueError):
        TK.tapvid_metrics(gold["m0_query_points"], gold["m0_gt_occluded"], gold["m0_gt_tracks"], gold["m0_pred_occluded"],
                          gold["m0_pred_tracks"], "every")


def test_first_visible_queries_match_the_reference(gold):
    pts, occ, want = gold["fv_points"], gold["fv_occluded"], gold["fv_out"]
    H, W = 480, 854
    q = TK.first_visible_queries(pts, occ, H, W)
    assert q.dtype == np.float64
    ref = want.copy()
    ref[:, 1] = ref[:, 1] * H
    ref[:, 2] = ref[:, 2] * W
    np.testing.assert_array_equal(q, ref)
    assert q[4, 0] == 0 and q[17, 0] == 0           # never visible: frame 0, as np.argmax gives


def test_nearest_centre_restatement_matches_the_reference(gold):
    np.testing.assert_array_equal(R.nearest(gold["fc_uv"], gold["fc_coords"]), gold["fc_index"])
    np.testing.assert_array_equal(R.nearest(gold["fc_uv_nan"], gold["fc_coords"]), gold["fc_index_nan"])
    assert gold["fc_index"][0] == 10                # duplicated rows 10 and 50: the lower index
    assert (gold["fc_index_nan"] == 120).all()      # a NaN distance wins, the first one


def test_frame_loop_restatement_hand_worked():
    # 3 splats, 2 frames, 4 x 4 image.  Splat 2 is culled: (0, 0), depth 0.
    uv0 = np.array([[1.5, 2.5], [3.0, 1.0], [0.0, 0.0]], np.float32)
    d0 = np.array([2.0, 3.0, 0.0], np.float32)
    dm0 = np.full((4, 4), 2.0, np.float32)
    uv1 = np.array([[2.5, -0.6], [3.4, 0.5], [0.0, 0.0]], np.float32)
    d1 = np.array([2.0, 3.0, 0.0], np.float32)
    dm1 = np.full((4, 4), 3.04, np.float32)
    dm1[0, 0] = 0.5
    q = np.array([[0, 2.25, 1.25],      # frame 0 at (x 1.25, y 2.25): splat 0, shift (-0.25, -0.25)
                  [1, 0.0, 3.5],        # frame 1 at (3.5, 0): splat 1 (3.4, 0.5)
                  [0, 0.1, 0.1]])       # frame 0 at (0.1, 0.1): the culled splat 2
    out = R.track_loop(q, [(uv0, d0, dm0), (uv1, d1, dm1)])
    np.testing.assert_array_equal(out["anchor"], [0, 1, 2])
    np.testing.assert_array_equal(out["shift"][0], [1.25 - 1.5, 2.25 - 2.5])
    # frame 0: splat 0 at (1.5, 2.5) rounds (half to even) to pixel (2, 2): depth_map 2.0 == depth 2.0 -> visible
    assert not out["occluded"][0, 0]
    np.testing.assert_array_equal(out["tracks"][0, 0], [1.25, 2.25])
    # query 1 is not anchored in frame 0: (0, 0), occluded
    np.testing.assert_array_equal(out["tracks"][1, 0], [0, 0])
    assert out["occluded"][1, 0]
    # frame 1: splat 0 at (2.5, -0.6) rounds to (2, -1): outside the image -> occluded
    assert out["occluded"][0, 1]
    np.testing.assert_array_equal(out["tracks"][0, 1], np.float32([np.float64(np.float32(2.5)) - 0.25,
                                                                   np.float64(np.float32(-0.6)) - 0.25]))
    # splat 1 at (3.4, 0.5) rounds to (3, 0): |3.04 - 3.0| <= 0.05 -> visible
    assert not out["occluded"][1, 1]
    # the culled anchor sits at (0, 0) with depth 0: depth_map 2.0 in frame 0 -> occluded; 0.5 in frame 1 -> occluded
    assert out["occluded"][2, 0] and out["occluded"][2, 1]
    np.testing.assert_array_equal(out["tracks"][2, 1], np.float32([0.1, 0.1]))


def test_make_clip_tracks_is_self_consistent():
    H, W, T = 96, 128, 8
    g = S.make_clip_tracks(T, H, W, seed=3, n_queries=80, query_seed=1)
    pts, occ, k, disc = g["points"], g["occluded"], g["sample_frame"], g["on_disc"]
    assert pts.shape == (80, T, 2) and occ.shape == (80, T)
    assert disc.any() and (~disc).any()
    sc = S._Scene(H, W, 3)
    x, y = pts[..., 0] * W, pts[..., 1] * H
    for i in range(80):
        # the sampled pixel is visible at its frame and at least 3 px inside the image
        assert not occ[i, k[i]]
        assert 3 <= x[i, k[i]] <= W - 4 and 3 <= y[i, k[i]] <= H - 4
        if disc[i]:
            cen = np.array([sc.obj_centre(j) for j in range(T)])
            off = np.stack([x[i] - cen[:, 0], y[i] - cen[:, 1]], -1)
            np.testing.assert_allclose(off, np.broadcast_to(off[k[i]], off.shape), atol=1e-9)
        else:
            a_k = sc.surface_param(torch.tensor([x[i, k[i]]]), torch.tensor([y[i, k[i]]]), int(k[i]))
            for j in range(T):
                a_j = sc.surface_param(torch.tensor([x[i, j]]), torch.tensor([y[i, j]]), j)
                assert abs(float(a_j - a_k)) < 1e-9
            np.testing.assert_array_equal(y[i], np.full(T, y[i, 0]))
    # the first-visible queries spread over more than one frame
    q = TK.first_visible_queries(pts, occ, H, W)
    assert len(np.unique(q[:, 0])) > 1


def test_disc_samples_sit_on_the_disc_texture():
    H, W, T = 96, 128, 6
    g = S.make_clip_tracks(T, H, W, seed=0, n_queries=64, query_seed=2)
    sc = S._Scene(H, W, 0)
    d = np.where(g["on_disc"])[0]
    assert len(d)
    x, y = g["points"][d, :, 0] * W, g["points"][d, :, 1] * H
    cols = []
    for j in range(T):
        cx, cy = sc.obj_centre(j)
        cols.append(sc.obj_tex(torch.tensor(x[:, j] - cx), torch.tensor(y[:, j] - cy)).numpy())
    for j in range(1, T):
        np.testing.assert_allclose(cols[j], cols[0], atol=1e-9)


def test_query_validation():
    ok = np.array([[0, 1.0, 2.0], [3, 4.0, 5.0]])
    TK.check_queries(ok, 4)
    for bad in ([[4, 1.0, 2.0]], [[-1, 1.0, 2.0]], [[0.5, 1.0, 2.0]], [[np.nan, 1.0, 2.0]], [[0, np.inf, 2.0]],
                [[0, 1.0, np.nan]], [[0, 1.0]], [0, 1.0, 2.0]):
        with pytest.raises(ValueError):
            TK.check_queries(np.array(bad, dtype=np.float64), 4)
    with pytest.raises(ValueError):
        TK.Tracker(np.array([[5, 1.0, 2.0]]), 4, "cpu")


def test_tapvid_pickle_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 1, (5, 7, 2)).astype(np.float32)
    occ = rng.random((5, 7)) < 0.4
    p = tmp_path / "tracking.pkl"
    TK.write_tapvid_pickle(p, pts, occ)
    p2, o2 = TK.read_tapvid_pickle(p)
    np.testing.assert_array_equal(p2, pts)
    np.testing.assert_array_equal(o2, occ)
    assert o2.dtype == bool


def test_evaluate_perfect_prediction_scores_one():
    g = S.make_clip_tracks(6, 96, 128, seed=1, n_queries=40, query_seed=0)
    T = 5
    pred = dict(tracks=(g["points"][:, :T] * [128, 96]).astype(np.float32), occluded=g["occluded"][:, :T])
    m = TK.evaluate(pred, g["points"].astype(np.float32), g["occluded"], 96, 128, T)
    assert m["occlusion_accuracy"] == 1.0
    assert m["average_pts_within_thresh"] == 1.0 and m["average_jaccard"] == 1.0


def test_reduce_tapvid_averages_over_clips():
    H, W, n = 96, 128, 5
    preds, gts, scores = {}, {}, {}
    # clip 0: the ground truth itself; clip 3: 3 px off, every fourth flag flipped; clip 4: 20 px off, never occluded
    for ci, (off, flip) in {0: (0.0, 0), 3: (3.0, 4), 4: (20.0, 0)}.items():
        g = S.make_clip_tracks(n + 1, H, W, seed=ci, n_queries=40, query_seed=0)
        pts, occ = g["points"].astype(np.float32), g["occluded"]
        occluded = occ[:, :n].copy()
        if flip:
            occluded.reshape(-1)[::flip] ^= True
        preds[ci] = dict(tracks=(g["points"][:, :n] * [W, H] + off).astype(np.float32),
                         occluded=occluded if ci != 4 else np.zeros_like(occluded))
        gts[ci] = (pts, occ, H, W)
        scores[ci] = TK.evaluate(preds[ci], pts, occ, H, W, n)
    frames = {ci: n for ci in preds}
    out = FV.reduce_tapvid(preds, gts, frames, 7)
    assert list(out) == list(FV.TAPVID_KEYS) + ["clips", "queries_dropped"]
    assert out["clips"] == 3 and out["queries_dropped"] == 7 and type(out["clips"]) is int and type(out["queries_dropped"]) is int
    for k in FV.TAPVID_KEYS:
        assert out[k] == (scores[0][k] + scores[3][k] + scores[4][k]) / 3, k
        assert scores[0][k] == 1.0 and scores[3][k] < 1.0 and scores[4][k] != scores[3][k]
    one = FV.reduce_tapvid({3: preds[3]}, gts, frames, 0)
    assert {k: one[k] for k in FV.TAPVID_KEYS} == {k: scores[3][k] for k in FV.TAPVID_KEYS} and one["clips"] == 1
    none = FV.reduce_tapvid({}, {}, {}, 2)                                     # no clip: NaN, the dropped queries still counted
    assert none["clips"] == 0 and none["queries_dropped"] == 2
    assert all(type(none[k]) is float and math.isnan(none[k]) for k in FV.TAPVID_KEYS)
