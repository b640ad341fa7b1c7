"""CPU: backward point tracking.  The numpy restatement (tests/tracking_back_ref.py) on a hand-worked case and its
"anchor < N_i => back_anchor == anchor" property on random data; the three entries in the header and the binding, the
arguments they refuse before any launch; TAP-Vid's strided queries and evaluate() on a query set of its own; the options
that are refused on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

from gflow_amd import _lib
from gflow_amd import fit_video as FV
from gflow_amd import tracking as TK
from tests import tracking_back_ref as B
from tests import tracking_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gfl_track_history", "gfl_track_backward_workspace_bytes", "gfl_track_backward")


def _hand_case():
    # 8 x 8 images; rows are only appended: N = 3, 4, 6.  Row 4 is culled in frame 2: (0, 0), depth 0.
    uv0 = np.array([[2, 1], [5, 4], [7, 1]], np.float32)
    uv1 = np.array([[1.5, 1], [4.5, 4], [6.5, 1], [5.25, 5.5]], np.float32)
    uv2 = np.array([[1, 1], [4, 4], [6, 1], [5, 5], [0, 0], [5.5, 6]], np.float32)
    d0 = np.array([2, 2, 2], np.float32)
    d1 = np.array([2, 2, 2, 3], np.float32)
    d2 = np.array([2, 2, 2, 3, 0, 3], np.float32)
    dm0 = np.full((8, 8), 2.0, np.float32)
    dm0[4, 5] = 2.5                          # row 1 of frame 0 sits on pixel (5, 4): |2.5 - 2| > 0.05
    dm1 = np.full((8, 8), 2.0, np.float32)
    dm1[6, 5] = 3.04                         # row 3 of frame 1 at (5.25, 5.5) rounds (half to even) to pixel (5, 6)
    dm2 = np.full((8, 8), 3.0, np.float32)
    q = np.array([[2, 6.25, 5.5],            # frame 2 at (x 5.5, y 6.25): row 5, born in frame 2
                  [1, 4.5, 4.5],             # frame 1 at (4.5, 4.5): row 1, which frame 0 has
                  [0, 1.0, 1.0]])            # frame 0: nothing before it
    return q, [(uv0, d0, dm0), (uv1, d1, dm1), (uv2, d2, dm2)]


def test_restatement_hand_worked():
    q, frames = _hand_case()
    out = B.track_loop(q, frames)
    fwd = R.track_loop(q, frames)
    np.testing.assert_array_equal(out["anchor"], [5, 1, 0])
    # query 0: distances to uv2 are row 5: 0.0625, row 3: 0.25 + 1.5625, row 1: 2.25 + 5.0625, the others farther.
    # Frame 1 has rows 0..3 -> row 3; frame 0 has rows 0..2 -> row 1
    np.testing.assert_array_equal(out["back_anchor"], [[1, 3, -1], [1, -1, -1], [-1, -1, -1]])
    # frame 1: uv1[3] + (xy - uv2[3]) = (5.25, 5.5) + (0.5, 1.25); frame 0: uv0[1] + (xy - uv2[1]) = (5, 4) + (1.5, 2.25)
    np.testing.assert_array_equal(out["tracks"][0, 1], np.float32([5.75, 6.75]))
    np.testing.assert_array_equal(out["tracks"][0, 0], np.float32([6.5, 6.25]))
    # row 3 in frame 1: |3.04 - 3| <= 0.05 -> visible; row 1 in frame 0 on the 2.5 pixel -> occluded
    assert not out["occluded"][0, 1] and out["occluded"][0, 0]
    # query 1: its anchor, row 1, exists in frame 0: the same row; uv0[1] + (xy - uv1[1]) = (5, 4) + (0, 0.5)
    np.testing.assert_array_equal(out["tracks"][1, 0], np.float32([5.0, 4.5]))
    assert out["occluded"][1, 0]
    # the columns i >= t, anchor and shift are the forward loop's; so is all of a frame-0 query
    t = q[:, 0].astype(int)
    for k in range(3):
        np.testing.assert_array_equal(out["tracks"][k, t[k]:], fwd["tracks"][k, t[k]:])
        np.testing.assert_array_equal(out["occluded"][k, t[k]:], fwd["occluded"][k, t[k]:])
    np.testing.assert_array_equal(out["tracks"][0, 2], np.float32([5.5, 6.25]))
    np.testing.assert_array_equal(out["shift"], fwd["shift"])
    np.testing.assert_array_equal(out["tracks"][2], fwd["tracks"][2])
    # what the forward loop alone leaves there
    assert (fwd["tracks"][0, :2] == 0).all() and fwd["occluded"][0, :2].all()
    # every row's flag of frame 2: the culled row 4 at (0, 0) with depth 0 is occluded, the others match the 3.0 plane or not
    np.testing.assert_array_equal(B.row_occlusion(*frames[2]), [True, True, True, False, True, False])


def _random_case(seed):
    rng = np.random.default_rng(seed)
    counts = [5, 9, 9, 14, 30]
    T, n = len(counts), counts[-1]
    base = rng.uniform(0, 16, (n, 2)).astype(np.float32)
    frames = []
    for i, c in enumerate(counts):
        uv = (base + rng.normal(0, 0.4, base.shape).astype(np.float32))[:c].copy()
        if c > 12:
            uv[12] = uv[2]                                   # duplicated rows: the lower index
        if c > 20:
            uv[20] = uv[7]
        if i == T - 1:
            uv[11] = np.nan                                  # a NaN row: first in the last frame's order
        depth = rng.uniform(1, 3, c).astype(np.float32)
        dm = rng.uniform(1, 3, (16, 16)).astype(np.float32)
        frames.append((uv, depth, dm))
    q = np.concatenate([np.stack([rng.integers(0, T, 60).astype(np.float64), rng.uniform(0, 16, 60), rng.uniform(0, 16, 60)], 1),
                        [[3, *frames[3][0][12][::-1]], [4, *frames[4][0][20][::-1]], [4, 3.0, 3.0]]])
    return q, frames, counts


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_keeps_the_forward_anchor_where_it_exists(seed):
    q, frames, counts = _random_case(seed)
    out = B.track_loop(q, frames)
    fwd = R.track_loop(q, frames)
    np.testing.assert_array_equal(out["anchor"], fwd["anchor"])
    t = q[:, 0].astype(int)
    kept = moved = 0
    for k in range(len(q)):
        for i in range(len(frames)):
            b = out["back_anchor"][k, i]
            if i >= t[k]:
                assert b == -1
                np.testing.assert_array_equal(out["tracks"][k, i], fwd["tracks"][k, i])
                assert out["occluded"][k, i] == fwd["occluded"][k, i]
                continue
            assert 0 <= b < counts[i]
            if out["anchor"][k] < counts[i]:
                assert b == out["anchor"][k]
                kept += 1
                # ... and the column is the forward rule's, run on frame i with the same anchor and shift
                uv, depth, dm = frames[i]
                want = (uv[b].astype(np.float64) + out["shift"][k]).astype(np.float32)
                np.testing.assert_array_equal(out["tracks"][k, i], want)
                assert out["occluded"][k, i] == B.row_occlusion(uv, depth, dm)[b]
            else:
                assert b != out["anchor"][k]
                moved += 1
    assert kept and moved
    assert out["anchor"][-3] == 2 and (out["back_anchor"][-3, :3] == 2).all()         # duplicate rows 2, 12: the lower
    assert (out["anchor"][t == 4] == 11).all()                                        # the NaN row wins in its frame,
    assert (out["back_anchor"][t == 4][:, :3] != 11).all()                            # not where it does not exist,
    assert (out["back_anchor"][t == 4][:, 3] == 11).all()                             # and again where it does (N_3 = 14)
    assert np.isnan(out["tracks"][t == 4][:, 3]).all()


def test_abi_entries():
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, code), name
    assert int(re.search(r"^#define GFL_VERSION (\d+)$", hdr, flags=re.M).group(1)) == 312 == _lib.MIN_VERSION
    assert "gfl_track_backward" in hdr[hdr.index("300 (round 5)"):hdr.index("#define GFL_VERSION")]     # the version comment
    lib = _lib.load()
    assert lib.gfl_version() == 312
    for name in NAMES:
        assert len(_lib.SIGNATURES[name][1]) == len(re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1).split(","))


def test_refused_arguments_and_workspace_query():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)      # (any non-null address: nothing is read before the refusal)
    ws_bytes = lib.gfl_track_backward_workspace_bytes
    assert ws_bytes(0, 5) == 0 and ws_bytes(7, 1) == 0 and ws_bytes(-1, 5) == 0
    need = ws_bytes(40, 5)
    assert need >= 12 * 40 * 5 and ws_bytes(80, 5) > need and ws_bytes(40, 10) > need
    hist = lambda **kw: lib.gfl_track_history(*[kw.get(k, v) for k, v in dict(
        uv=one, uv_stride=12, depth=one, depth_stride=12, N=64, depth_map=one, W=24, H=16, thr=0.05, hist_uv=one, hist_occ=one,
        stream=null).items()])
    for bad in (dict(uv=null), dict(depth=null), dict(depth_map=null), dict(hist_uv=null), dict(hist_occ=null), dict(N=-1),
                dict(uv_stride=1), dict(depth_stride=0), dict(W=0), dict(H=0)):
        assert hist(**bad) == -1, bad
    back = lambda **kw: lib.gfl_track_backward(*[kw.get(k, v) for k, v in dict(
        hist_uv=one, hist_occ=one, row_start=one, T=5, query_xy=one, query_frame=one, Q=40, tracks=one, occluded=one,
        back_anchor=one, workspace=one, workspace_bytes=need, stream=null).items()])
    for bad in (dict(hist_uv=null), dict(hist_occ=null), dict(row_start=null), dict(query_xy=null), dict(query_frame=null),
                dict(tracks=null), dict(occluded=null), dict(workspace=null), dict(T=0), dict(T=-3), dict(Q=-1),
                dict(hist_uv=ctypes.c_void_p(260))):
        assert back(**bad) == -1, bad
    assert back(workspace_bytes=need - 1) == -2               # GFL_ERR_WORKSPACE
    assert back(workspace_bytes=0, back_anchor=null) == -2    # (a null back_anchor is allowed: refused for the workspace)
    assert back(Q=0, workspace=null, workspace_bytes=0) == 0 and back(T=1, workspace=null, workspace_bytes=0) == 0


def _three_tracks():
    # 3 tracks, 11 frames, 100 x 200 image: track 0 always visible, track 1 hidden in frame 5, track 2 only visible in 10
    T = 11
    pts = np.zeros((3, T, 2), np.float32)
    for k in range(3):
        pts[k, :, 0] = (0.1 + 0.02 * np.arange(T)) + 0.2 * k      # x / W
        pts[k, :, 1] = 0.25 * (k + 1)                              # y / H
    occ = np.zeros((3, T), bool)
    occ[1, 5] = True
    occ[2, :10] = True
    return pts, occ


def test_strided_queries_hand_worked():
    pts, occ = _three_tracks()
    H, W = 100, 200
    q, src = TK.strided_queries(pts, occ, H, W)
    assert q.dtype == np.float64 and src.dtype == np.int64
    # frames 0, 5, 10; by frame, then by track
    np.testing.assert_array_equal(q[:, 0], [0, 0, 5, 10, 10, 10])
    np.testing.assert_array_equal(src, [0, 1, 0, 0, 1, 2])
    for m in range(len(q)):
        t, k = int(q[m, 0]), src[m]
        assert q[m, 1] == np.float64(pts[k, t, 1]) * H and q[m, 2] == np.float64(pts[k, t, 0]) * W
    fv = TK.first_visible_queries(pts, occ, H, W)
    np.testing.assert_array_equal(q[[0, 1, 5]], fv)                # (where the two protocols meet: the same numbers)
    q3, src3 = TK.strided_queries(pts, occ, H, W, stride=3)        # frames 0, 3, 6, 9
    np.testing.assert_array_equal(q3[:, 0], [0, 0, 3, 3, 6, 6, 9, 9])
    np.testing.assert_array_equal(src3, [0, 1] * 4)
    with pytest.raises(ValueError):
        TK.strided_queries(pts, occ, H, W, stride=0)


def _evaluate_as_before(pred, points, occluded, H, W, n_frames):
    q = TK.first_visible_queries(points, occluded, H, W)
    gt = points[None, :, :n_frames].copy()
    gt[..., 0] = gt[..., 0] * W
    gt[..., 1] = gt[..., 1] * H
    gt[..., 0] = gt[..., 0] / W * 255
    gt[..., 1] = gt[..., 1] / H * 255
    pt = np.asarray(pred["tracks"])[None].copy()
    pt[..., 0] = pt[..., 0] / W * 255
    pt[..., 1] = pt[..., 1] / H * 255
    m = TK.tapvid_metrics(q[None], occluded[None, :, :n_frames], gt, np.asarray(pred["occluded"])[None], pt, "strided")
    return {k: float(v[0]) for k, v in m.items()}


def test_evaluate_with_a_query_set_of_its_own():
    pts, occ = _three_tracks()
    H, W, T = 100, 200, 11
    rng = np.random.default_rng(0)
    # the default path: the same dict as before
    pred = dict(tracks=(pts * [W, H] + rng.normal(0, 2, pts.shape)).astype(np.float32), occluded=occ ^ (rng.random(occ.shape) < 0.2))
    assert TK.evaluate(pred, pts, occ, H, W, T) == _evaluate_as_before(pred, pts, occ, H, W, T)
    assert TK.evaluate(pred, pts, occ, H, W, T, queries=TK.first_visible_queries(pts, occ, H, W), source=np.arange(3)) \
        == _evaluate_as_before(pred, pts, occ, H, W, T)
    # the strided set, hand-worked: 6 queries.  The perfect prediction scores one ...
    q, src = TK.strided_queries(pts, occ, H, W)
    perfect = dict(tracks=(pts[src] * [W, H]).astype(np.float32), occluded=occ[src])
    m = TK.evaluate(perfect, pts, occ, H, W, T, queries=q, source=src)
    assert m["occlusion_accuracy"] == 1.0 and m["average_pts_within_thresh"] == 1.0 and m["average_jaccard"] == 1.0
    # ... and a forward-only tracker ((0, 0), occluded before the query frame) misses exactly the frames before its queries:
    # counted are 10 frames per query; visible in the ground truth 10, 9, 10, 10, 9, 0 of them; before the query frame lie
    # 0, 0, 5, 10, 9 (frame 5 of track 1 is hidden) and 0 visible ones
    fwd = dict(tracks=perfect["tracks"].copy(), occluded=perfect["occluded"].copy())
    for k in range(len(q)):
        fwd["tracks"][k, :int(q[k, 0])] = 0
        fwd["occluded"][k, :int(q[k, 0])] = True
    m = TK.evaluate(fwd, pts, occ, H, W, T, queries=q, source=src)
    assert m["average_pts_within_thresh"] == pytest.approx((48 - 24) / 48, abs=1e-15)
    # occlusion: wrong where the truth is visible before the query (24 frames), right elsewhere (60 counted)
    assert m["occlusion_accuracy"] == pytest.approx((60 - 24) / 60, abs=1e-15)
    with pytest.raises(ValueError):
        TK.evaluate(perfect, pts, occ, H, W, T, queries=q)
    with pytest.raises(ValueError):
        TK.evaluate(perfect, pts, occ, H, W, T, queries=q, source=src[:-1])
    # reduce_tapvid hands the pair through
    out = FV.reduce_tapvid({0: fwd}, {0: (pts, occ, H, W, q, src)}, {0: T}, 0)
    assert out["average_pts_within_thresh"] == m["average_pts_within_thresh"] and out["clips"] == 1


def test_options_refused_on_the_host(capsys):
    with pytest.raises(ValueError, match="track_queries"):
        next(FV.fit_clip_steps([{}], "cpu", track_backward=True))
    with pytest.raises(ValueError, match="track_queries"):
        FV.fit_clips_concurrent([[{}], [{}]], "cpu", track_backward=True)
    with pytest.raises(SystemExit) as e:
        FV.main(["--track-backward"])
    assert e.value.code == 2 and "--track-backward needs --track" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        FV.main(["--track", "--track-queries", "every"])
