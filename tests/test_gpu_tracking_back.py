"""Backward point tracking on the device (``-m gpu``; gfl_track_history / gfl_track_backward, Tracker(backward=True)):
exact properties -- the two entries against the numpy restatement (tests/tracking_back_ref.py) and, at size, against
torch's float64 argmin per prefix; fits with ``track_backward`` against the restatement run on the inputs they recorded,
against the same fit without the option, against each other -- and the score of the frames before the queries on a
deterministic fit (the same bits on every run of a build)."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import tracking_back_ref as B
from tests.score_fit import FIT, H, T, W, clip, queries

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tracks", "occluded", "anchor", "shift", "back_anchor")


# ------------------------------------------------------------------------------------------------------ the two entries
def test_history_kernel_matches_restatement():
    """the edge cases of test_gpu_tracking.py::test_frame_kernel_matches_restatement, for every row of a frame"""
    from gflow_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(2)
    h, w, n = 16, 24, 64
    uv = rng.uniform(-2, 26, (n, 2)).astype(np.float32)
    uv[:10] = np.array([[0.5, 0.5], [1.5, 2.5], [2.5, 3.5], [-0.5, 4.0], [23.5, 15.5], [24.5, 1.0], [3.0, 15.5],
                        [-1.0, 2.0], [0.0, 0.0], [5.5, -0.5]], np.float32)
    uv[10] = [11.0, -0.6]                              # rint above the first row: out
    depth = rng.uniform(1, 3, n).astype(np.float32)
    depth[8] = 0.0                                     # culled
    depth[1] = depth[2] = 0.0
    dm = rng.uniform(1, 3, (h, w)).astype(np.float32)
    dm[2, 2] = np.float32(0.05)                        # |dm - d| exactly 0.05f: (1.5, 2.5) rounds to (2, 2)
    dm[4, 2] = np.nextafter(np.float32(0.05), np.float32(1))      # one ulp above: (2.5, 3.5) rounds to (2, 4)
    want = B.row_occlusion(uv, depth, dm)
    assert not want[1] and want[2]                     # exactly 0.05f apart: not occluded (a strict >); one ulp more: occluded
    assert want[4] and want[5] and want[6] and want[7] and want[10]           # rint out of the image on all four sides
    assert want[8] == (abs(dm[0, 0] - np.float32(0)) > np.float32(0.05))      # the culled row at (0, 0), depth 0
    rec = rng.uniform(-5, 5, (n, 12)).astype(np.float32)
    rec[:, 0:2], rec[:, 9] = uv, depth
    d_dm = torch.from_numpy(dm).to(DEV)
    d_rec, d_uv, d_depth = (torch.from_numpy(x).to(DEV) for x in (rec, uv, depth))
    for src_uv, s_uv, src_d, s_d in ((d_rec, 12, d_rec[:, 9], 12), (d_uv, 2, d_depth, 1)):
        for rows in (n, 37):
            h_uv = torch.full((n + 8, 2), 9.0, device=DEV)
            h_occ = torch.full((n + 8,), 7, dtype=torch.uint8, device=DEV)
            L.check(lib.gfl_track_history(L.ptr(src_uv), s_uv, L.ptr(src_d), s_d, rows, L.ptr(d_dm), w, h, 0.05, L.ptr(h_uv),
                                          L.ptr(h_occ), L.stream()), "track history")
            got_uv, got_occ = h_uv.cpu().numpy(), h_occ.cpu().numpy()
            np.testing.assert_array_equal(got_uv[:rows], uv[:rows])
            np.testing.assert_array_equal(got_occ[:rows], want[:rows].astype(np.uint8))
            assert (got_uv[rows:] == 9.0).all() and (got_occ[rows:] == 7).all()      # behind the slice: untouched
    h_uv = torch.full((4, 2), 9.0, device=DEV)
    h_occ = torch.full((4,), 7, dtype=torch.uint8, device=DEV)
    assert lib.gfl_track_history(L.ptr(d_uv), 2, L.ptr(d_depth), 1, 0, L.ptr(d_dm), w, h, 0.05, L.ptr(h_uv), L.ptr(h_occ),
                                 L.stream()) == 0                                    # no row: nothing
    assert (h_uv.cpu().numpy() == 9.0).all() and (h_occ.cpu().numpy() == 7).all()


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _fma_changes_argmin():
    """Rows (a, b), (b, a) around a query (c, c) on the diagonal (the idea of test_gpu_tracking.py's helper): their distances
    tie when every product and the sum are rounded on their own (-> the lower index), but fma(dx, dx, dy * dy) and
    fma(dy, dy, dx * dx) differ -- whichever way a contracted distance is formed, one of the two row orders then picks the
    higher index.  Here the pair also lies closer to the query than (0, 0), where the culled rows sit."""
    rng = np.random.default_rng(5)
    for _ in range(100000):
        a, b = (float(np.float32(v)) for v in rng.uniform(0, 100, 2))
        c = float(rng.uniform(0, 100))
        dx, dy = a - c, b - c
        if _fma(dx, dx, dy * dy) != _fma(dy, dy, dx * dx) and dx * dx + dy * dy < c * c:
            assert dx * dx + dy * dy == dy * dy + dx * dx
            return np.array([[a, b], [b, a]], np.float32), np.array([c, c])
    raise AssertionError("no FMA-sensitive tie found")


def _backward(frames, q, order=None, with_back_anchor=True):
    """gfl_track_backward on the history of ``frames`` (per frame uv, depth, depth_map) for the queries ``q`` (rows
    [t, y, x]); the outputs start as sentinels (9.0, 7, -7).  Returns host arrays in the order of ``q``."""
    from gflow_amd import _lib as L
    lib = L.load()
    n_t, n_q = len(frames), len(q)
    order = np.arange(n_q) if order is None else order
    hist_uv = torch.from_numpy(np.concatenate([f[0] for f in frames]).astype(np.float32)).to(DEV)
    hist_occ = torch.from_numpy(np.concatenate([B.row_occlusion(*f) for f in frames]).astype(np.uint8)).to(DEV)
    row_start = torch.from_numpy(np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int64)).to(DEV)
    xy = torch.from_numpy(np.ascontiguousarray(q[order][:, [2, 1]])).to(DEV)
    qf = torch.from_numpy(q[order][:, 0].astype(np.int32)).to(DEV)
    tracks = torch.full((n_q, n_t, 2), 9.0, device=DEV)
    occ = torch.full((n_q, n_t), 7, dtype=torch.uint8, device=DEV)
    back = torch.full((n_q, n_t), -7, dtype=torch.int32, device=DEV)
    ws = L.scratch(lib.gfl_track_backward_workspace_bytes(n_q, n_t), DEV)
    L.check(lib.gfl_track_backward(L.ptr(hist_uv), L.ptr(hist_occ), L.ptr(row_start), n_t, L.ptr(xy), L.ptr(qf), n_q,
                                   L.ptr(tracks), L.ptr(occ), L.ptr(back) if with_back_anchor else None, L.ptr(ws), ws.numel(),
                                   L.stream()), "track backward")
    inv = np.empty(n_q, np.int64)
    inv[order] = np.arange(n_q)
    return tracks.cpu().numpy()[inv], occ.cpu().numpy()[inv], back.cpu().numpy()[inv]


COUNTS = [7, 7, 300, 1100, 1100]       # equal counts in consecutive frames, a breakpoint inside an LDS tile, one past 1024


def _small_case(nan_row):
    rng = np.random.default_rng(3)
    n_t, n = len(COUNTS), COUNTS[-1]
    fu, fq = _fma_changes_argmin()
    base = rng.uniform(300, 350, (n, 2)).astype(np.float32)               # (far from the tie pair and from (0, 0))
    frames = []
    for i, c in enumerate(COUNTS):
        uv = (base + rng.normal(0, 0.5, base.shape).astype(np.float32))[:c].copy()
        uv[1:3] = fu if i % 2 else fu[::-1]                               # the FMA-sensitive tie, in both row orders
        uv[5] = 0                                                         # culled rows
        if c > 110:
            uv[100:110] = 0
        if c > 500:
            uv[500] = uv[3]                                               # row 3 again: the prefix keeps 3 everywhere
        if nan_row and i == n_t - 1:
            uv[900] = np.nan                                              # wins where it exists: N_i > 900
        frames.append((uv, rng.uniform(1, 3, c).astype(np.float32), rng.uniform(1, 3, (16, 24)).astype(np.float32)))
    t = np.arange(40) % n_t                                               # t over 0..4, unsorted
    xy = rng.uniform(295, 355, (40, 2))
    q = np.concatenate([t[:, None].astype(np.float64), xy[:, ::-1]], axis=1)
    special = [[4, *frames[4][0][1050][::-1].astype(np.float64)],         # nearest row 1050
               [4, *frames[4][0][3][::-1].astype(np.float64)], [3, *frames[3][0][500][::-1].astype(np.float64)],
               [1, *fq[::-1]], [2, *fq[::-1]], [3, *fq[::-1]], [4, *fq[::-1]],
               [2, 0.25, 0.5], [4, 0.25, 0.5]]                            # on the culled rows: the lowest of them
    q[-len(special):] = np.array(special)
    return q, frames, len(q) - len(special)


@pytest.mark.parametrize("nan_row", [False, True])
def test_backward_kernel_small_matches_restatement(nan_row):
    q, frames, s0 = _small_case(nan_row)
    n_t = len(frames)
    assert sorted(set(q[:, 0])) == [0, 1, 2, 3, 4]
    want = B.backward(q, frames)
    w = want["written"]
    assert w.sum() == sum(int(v) for v in q[:, 0])
    for order in (np.argsort(q[:, 0], kind="stable"), None):              # (as Tracker hands them over; as they come)
        tracks, occ, back = _backward(frames, q, order)
        np.testing.assert_array_equal(back[w], want["back_anchor"][w])
        np.testing.assert_array_equal(tracks[w], want["tracks"][w])
        np.testing.assert_array_equal(occ[w], want["occluded"][w].astype(np.uint8))
        # t == 0 queries and the columns i >= t: untouched
        assert (tracks[~w] == 9.0).all() and (occ[~w] == 7).all() and (back[~w] == -7).all()
    t2, o2, b2 = _backward(frames, q, np.argsort(q[:, 0], kind="stable"), with_back_anchor=False)
    np.testing.assert_array_equal(t2, tracks)
    np.testing.assert_array_equal(o2, occ)
    assert (b2 == -7).all()                                               # a null back_anchor: nothing written there
    # what the case was built for
    if nan_row:
        four = q[:, 0] == 4
        assert (back[four][:, 3] == 900).all() and (back[four][:, :3] != 900).all()
        assert np.isnan(tracks[four][:, 3]).all() and not np.isnan(tracks[four][:, :3]).any()
    else:
        assert back[s0, 3] == 1050 and (back[s0, :3] < 300).all()
        np.testing.assert_array_equal(back[s0 + 1, :4], [3, 3, 3, 3])     # row 500 is row 3 again: the lower index
        np.testing.assert_array_equal(back[s0 + 6, :4], [1, 1, 1, 1])     # the tie: the lower index, in either row order
        np.testing.assert_array_equal(back[s0 + 8, :4], [5, 5, 5, 5])     # the culled rows 5, 100..109: the lowest
    np.testing.assert_array_equal(back[s0 + 2, :3], [3, 3, 3])
    np.testing.assert_array_equal(back[s0 + 3, :1], [1])
    np.testing.assert_array_equal(back[s0 + 4, :2], [1, 1])
    np.testing.assert_array_equal(back[s0 + 5, :3], [1, 1, 1])
    np.testing.assert_array_equal(back[s0 + 7, :2], [5, 5])


def test_backward_kernel_matches_argmin_at_size():
    g = torch.Generator(device=DEV).manual_seed(0)
    n_t, n, n_q = 12, 200000, 2048
    counts = np.linspace(20000, n, n_t).astype(np.int64)
    counts[5] = counts[4]                                                 # (a frame that appends nothing)
    size = torch.tensor([854.0, 480.0], device=DEV)
    base = torch.rand(n, 2, device=DEV, generator=g) * size
    uvs = []
    for c in counts:
        uv = (base[:c] + torch.randn(int(c), 2, device=DEV, generator=g)).float()
        uv[1000:1100] = 0                                                 # culled rows
        uvs.append(uv)
    hist_uv = torch.cat(uvs)
    hist_occ = (torch.rand(hist_uv.shape[0], device=DEV, generator=g) < 0.3).to(torch.uint8)
    row_start = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).to(DEV)
    xy = torch.rand(n_q, 2, device=DEV, generator=g, dtype=torch.float64) * size.double()
    qf = torch.sort(torch.randint(0, n_t, (n_q,), device=DEV, generator=g).int()).values
    xy[-8:] = 0.0                                                         # on the culled rows: the lowest of them
    from gflow_amd import _lib as L
    lib = L.load()
    tracks = torch.full((n_q, n_t, 2), 9.0, device=DEV)
    occ = torch.full((n_q, n_t), 7, dtype=torch.uint8, device=DEV)
    back = torch.full((n_q, n_t), -7, dtype=torch.int32, device=DEV)
    ws = L.scratch(lib.gfl_track_backward_workspace_bytes(n_q, n_t), DEV)
    L.check(lib.gfl_track_backward(L.ptr(hist_uv), L.ptr(hist_occ), L.ptr(row_start), n_t, L.ptr(xy), L.ptr(qf), n_q,
                                   L.ptr(tracks), L.ptr(occ), L.ptr(back), L.ptr(ws), ws.numel(), L.stream()), "track backward")
    want = torch.full((n_q, n_t), -7, dtype=torch.int64, device=DEV)
    for t in range(1, n_t):
        mine = torch.nonzero(qf == t).reshape(-1)
        uv = uvs[t][:counts[t - 1]].double()
        for a in range(0, len(mine), 64):                                 # (separate sub / mul / add kernels: nothing contracts)
            k = mine[a:a + 64]
            d = ((uv[:, None, :] - xy[None, k, :]) ** 2).sum(-1)
            for i in range(t):
                want[k, i] = d[:counts[i]].argmin(dim=0)
    back_h, want_h, qf_h = back.cpu().numpy(), want.cpu().numpy(), qf.cpu().numpy()
    np.testing.assert_array_equal(back_h, want_h)
    assert (back_h[-8:, :n_t - 1] == 1000).all() and qf_h[-1] == n_t - 1
    assert (back_h[qf_h == n_t - 1][:, n_t - 2] > counts[n_t - 3]).any()  # (rows of the last slices are chosen too)
    # tracks and flags from the indices, in numpy
    tr_h, occ_h, xy_h = tracks.cpu().numpy(), occ.cpu().numpy(), xy.cpu().numpy()
    uv_h, ho_h = [u.cpu().numpy() for u in uvs], hist_occ.cpu().numpy()
    rs = np.concatenate([[0], np.cumsum(counts)])
    for i in range(n_t):
        k = np.where(qf_h > i)[0]
        b = back_h[k, i]
        then = np.stack([uv_h[t][bb] for t, bb in zip(qf_h[k], b)]).astype(np.float64) if len(k) else np.zeros((0, 2))
        np.testing.assert_array_equal(tr_h[k, i], (uv_h[i][b].astype(np.float64) + (xy_h[k] - then)).astype(np.float32))
        np.testing.assert_array_equal(occ_h[k, i], ho_h[rs[i] + b])
        rest = np.where(qf_h <= i)[0]
        assert (tr_h[rest, i] == 9.0).all() and (occ_h[rest, i] == 7).all()


# ------------------------------------------------------------------------------------------------------------ the fits
def sample_queries(n_frames=T, n=96, seed=0):
    """(the clip's ground-truth tracks, a query [t, y, x] per track at the frame the track was sampled in: most t > 0)"""
    g, _ = queries(n_frames=n_frames, n=n, seed=seed)
    k = g["sample_frame"]
    at = g["points"].astype(np.float32)[np.arange(n), k]
    q = np.stack([k.astype(np.float64), at[:, 1].astype(np.float64) * H, at[:, 0].astype(np.float64) * W], axis=1)
    return g, q


def _fit(frames, q, backward=True, fused=True, cfg=FIT, seed=0):
    from gflow_amd.fit_video import fit_clip
    keep = {"record_track_inputs": True}
    out = fit_clip(frames, DEV, cfg, seed=seed, fused=fused, deterministic=True if fused else None, track_queries=q,
                   keep=keep, **({"track_backward": True} if backward else {}))
    return out, keep


@pytest.fixture(scope="module")
def back_fit():
    frames = clip()
    g, q = sample_queries()
    assert (q[:, 0] > 0).mean() > 0.5
    out, keep = _fit(frames, q)
    return frames, g, q, out, keep


@pytest.fixture(scope="module")
def plain_fit(back_fit):
    frames, g, q, _, _ = back_fit
    return _fit(frames, q, backward=False)


def _check_against_restatement(q, out, keep):
    inputs = [(u.cpu().numpy(), d.cpu().numpy(), m.cpu().numpy()) for u, d, m in keep["track_inputs"]]
    assert len(inputs) == T
    ref = B.track_loop(q, inputs)
    got = out["tracks"]
    assert sorted(got) == sorted(KEYS) and got["back_anchor"].dtype == np.int32 and got["back_anchor"].shape == (len(q), T)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    counts = [u.shape[0] for u, _, _ in inputs]
    assert counts == sorted(counts) and counts[-1] > counts[0]            # (rows were appended during the clip)
    t = q[:, 0].astype(int)
    moved = 0
    for k in range(len(q)):
        assert (got["back_anchor"][k, t[k]:] == -1).all()
        for i in range(t[k]):
            b = got["back_anchor"][k, i]
            assert 0 <= b < counts[i]
            if got["anchor"][k] < counts[i]:
                assert b == got["anchor"][k]
            else:
                moved += 1
    return moved


def test_fit_equals_the_restatement(back_fit):
    frames, g, q, out, keep = back_fit
    moved = _check_against_restatement(q, out, keep)
    print("columns carried by another splat than the forward anchor:", moved)
    assert moved > 0                                                      # (some anchors were born after frame 0)


def test_fit_equals_the_restatement_operator_path():
    frames = clip()
    _, q = sample_queries()
    out, keep = _fit(frames, q, fused=False)
    _check_against_restatement(q, out, keep)


def test_option_changes_nothing_else(back_fit, plain_fit):
    """the columns i >= t, anchor and shift, and the fit itself (what tests/score_fit.py's assert_same_fit compares)"""
    frames, g, q, out, keep = back_fit
    plain, keep0 = plain_fit
    assert "back_anchor" not in plain["tracks"]
    t = q[:, 0].astype(int)
    after = np.arange(T)[None] >= t[:, None]
    np.testing.assert_array_equal(out["tracks"]["tracks"][after], plain["tracks"]["tracks"][after])
    np.testing.assert_array_equal(out["tracks"]["occluded"][after], plain["tracks"]["occluded"][after])
    np.testing.assert_array_equal(out["tracks"]["anchor"], plain["tracks"]["anchor"])
    np.testing.assert_array_equal(out["tracks"]["shift"], plain["tracks"]["shift"])
    assert (plain["tracks"]["tracks"][~after] == 0).all() and plain["tracks"]["occluded"][~after].all()
    assert (out["tracks"]["tracks"][~after] != 0).any()
    for k in ("psnr_sum", "frames", "iterations", "rasterisations", "splats_final", "void_iterations"):
        assert out[k] == plain[k], k
    ea, eb = keep["trainer"].engine, keep0["trainer"].engine
    assert ea.N == eb.N
    for k in ("params", "adam_m", "adam_v"):
        assert torch.equal(getattr(ea, k)[:ea.N], getattr(eb, k)[:eb.N]), k
    for k in ("pose", "depth_ab", "render"):
        assert torch.equal(getattr(ea, k), getattr(eb, k)), k
    assert torch.equal(torch.stack([p.float() for p in keep["psnr"]]), torch.stack([p.float() for p in keep0["psnr"]]))
    for a, b in zip(keep["track_inputs"], keep0["track_inputs"]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_option_leaves_trajectories_unchanged():
    from gflow_amd.fit_video import fit_clip
    frames = clip(n_frames=4)
    _, q = sample_queries(n_frames=4)
    cfg = dict(FIT, traj_num=50)
    a = fit_clip(frames, DEV, cfg, seed=0, deterministic=True, track_queries=q)
    b = fit_clip(frames, DEV, cfg, seed=0, deterministic=True, track_queries=q, track_backward=True)
    np.testing.assert_array_equal(a["traj"]["images"], b["traj"]["images"])
    np.testing.assert_array_equal(a["traj"]["uv"], b["traj"]["uv"])
    assert a["rasterisations"] == b["rasterisations"] and a["iterations"] == b["iterations"] and a["psnr_sum"] == b["psnr_sum"]
    assert "back_anchor" in b["tracks"] and (b["tracks"]["back_anchor"] >= 0).any()
    with pytest.raises(ValueError):
        fit_clip(frames, DEV, cfg, seed=0, deterministic=True, track_backward=True)


def test_deterministic_fits_give_identical_arrays(back_fit):
    from gflow_amd.fit_video import fit_clips_concurrent
    frames, g, q, out, keep = back_fit
    again, _ = _fit(frames, q)
    for k in KEYS:
        np.testing.assert_array_equal(again["tracks"][k], out["tracks"][k])
    other = clip(seed=1)
    _, q1 = sample_queries(seed=1)
    lone1, _ = _fit(other, q1, seed=1)
    res = fit_clips_concurrent([frames, other], DEV, FIT, seeds=[0, 1], deterministic=True, track_queries=[q, q1],
                               track_backward=True)
    for r, want in zip(res, (out, lone1)):
        for k in KEYS:
            np.testing.assert_array_equal(r["tracks"][k], want["tracks"][k])


def test_tracker_refuses_frames_it_cannot_carry_back():
    from gflow_amd import tracking as TK
    dm = torch.zeros(8, 8, device=DEV)
    rows = lambda n: (torch.zeros(n, 2, device=DEV), 2, torch.zeros(n, device=DEV), 1, dm)
    tk = TK.Tracker(np.array([[1, 2.0, 2.0]]), 3, DEV, backward=True)
    with pytest.raises(ValueError):
        tk.frame(1, *rows(4))                                             # frame 0 comes first
    with pytest.raises(ValueError):
        tk.frame(0, *rows(0))                                             # every frame needs a row
    tk.frame(0, *rows(4))
    with pytest.raises(ValueError):
        tk.frame(1, *rows(3))                                             # rows are only appended
    tk.frame(1, *rows(4))
    out = tk.result()                                                     # (frame 2 never came: its column stays as it was)
    np.testing.assert_array_equal(out["back_anchor"], [[0, -1, -1]])
    np.testing.assert_array_equal(out["tracks"][0], [[2, 2], [2, 2], [0, 0]])
    np.testing.assert_array_equal(out["occluded"][0], [False, False, True])


# ------------------------------------------------------------------------------------------------------------- the score
def _before_query_metrics(pred, g, q):
    """tapvid_metrics over the frames BEFORE each query alone (frames < t), coordinates scaled to 256 x 256 as
    tracking.evaluate scales them: with the time axis reversed these are exactly the frames 'first' counts."""
    from gflow_amd import tracking as TK
    pts, occ = g["points"].astype(np.float32), g["occluded"]
    gt = pts[None, :, :T].copy()
    gt[..., 0] = gt[..., 0] * W / W * 255
    gt[..., 1] = gt[..., 1] * H / H * 255
    pt = np.asarray(pred["tracks"])[None].copy()
    pt[..., 0] = pt[..., 0] / W * 255
    pt[..., 1] = pt[..., 1] / H * 255
    qr = q.copy()
    qr[:, 0] = T - 1 - q[:, 0]
    m = TK.tapvid_metrics(qr[None], occ[None, :, :T][:, :, ::-1], gt[:, :, ::-1], np.asarray(pred["occluded"])[None][:, :, ::-1],
                          pt[:, :, ::-1], "first")
    return {k: float(v[0]) for k, v in m.items()}


QUALITY = dict(apts=0.7795, oa=0.7204)


def test_backward_tracking_quality_on_the_synthetic_clip(back_fit, plain_fit):
    """The frames before each query alone, scored against make_clip_tracks (deterministic fit: the same numbers on every run
    of a build).  Measured on MI355X: average_pts_within_thresh 0.7795, occlusion_accuracy 0.7204, average_jaccard 0.5082;
    the same fit without the option ((0, 0) and occluded there) 0.0, 0.0517 and 0.0; the zero-motion baseline (prediction =
    query position, never occluded) 0.2571, 0.9483 and 0.1771.  Bounds: strictly better than without the option, the measured
    values minus 0.05, and 0.05 above the baseline's position accuracy (as in the forward test, this clip's fit predicts
    occlusion worse than "never occluded" does)."""
    frames, g, q, out, keep = back_fit
    plain, _ = plain_fit
    still = dict(tracks=np.repeat(q[:, None, [2, 1]], T, axis=1).astype(np.float32), occluded=np.zeros((len(q), T), bool))
    m, m_off, m0 = (_before_query_metrics(p, g, q) for p in (out["tracks"], plain["tracks"], still))
    names = ("average_pts_within_thresh", "occlusion_accuracy", "average_jaccard")
    print("backward tracking quality", json.dumps({k: m[k] for k in names}), "without the option",
          json.dumps({k: m_off[k] for k in names}), "zero-motion", json.dumps({k: m0[k] for k in names}))
    assert m["average_pts_within_thresh"] > m_off["average_pts_within_thresh"]
    assert m["average_jaccard"] > m_off["average_jaccard"]
    assert m["occlusion_accuracy"] > m_off["occlusion_accuracy"]
    assert m["average_pts_within_thresh"] >= QUALITY["apts"] - 0.05
    assert m["occlusion_accuracy"] >= QUALITY["oa"] - 0.05
    assert m["average_pts_within_thresh"] >= m0["average_pts_within_thresh"] + 0.05


# --------------------------------------------------------------------------------------------------------------- the CLI
def test_cli_strided_backward_tapvid_block_equals_in_process_evaluate(tmp_path):
    from gflow_amd import io as gio
    from gflow_amd import tracking as TK
    from gflow_amd.fit_video import fit_clip
    n = 7                                              # (the sequence convention fits n - 1 frames: strided queries at 0 and 5)
    frames = clip(n_frames=n)
    seq = gio.write_sequence(frames, str(tmp_path / "clip"))
    g, _ = queries(n_frames=n, n=96)
    pts, occ = g["points"].astype(np.float32), g["occluded"]
    TK.write_tapvid_pickle(os.path.join(seq, "tracking.pkl"), pts, occ)
    args = ["--sequence", seq, "--track", "--track-backward", "--track-queries", "strided", "--deterministic", "--num_points",
            "1500", "--iterations_first", "60", "--iterations_after", "40", "--iterations_camera", "20", "--track-out",
            str(tmp_path / "out")]
    r = subprocess.run([sys.executable, "-m", "gflow_amd.fit_video", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    disk = gio.load_sequence(seq)
    h, w = disk[0]["image"].shape[:2]
    q, src = TK.strided_queries(pts, occ, h, w)
    keep = q[:, 0] < len(disk)
    assert sorted(set(q[keep][:, 0])) == [0, 5]
    cfg = dict(num_points=1500, iterations_first=60, iterations_after=40, iterations_camera=20)
    out = fit_clip(disk, DEV, cfg, seed=0, deterministic=True, track_queries=q[keep], track_backward=True)
    m = TK.evaluate(out["tracks"], pts, occ, h, w, len(disk), queries=q[keep], source=src[keep])
    tv = line["tapvid"]
    assert tv["backward"] is True and tv["clips"] == 1 and tv["queries_dropped"] == int((~keep).sum())
    for k in ("occlusion_accuracy", "average_jaccard", "average_pts_within_thresh"):
        assert tv[k] == m[k], k
    saved = np.load(os.path.join(tmp_path / "out", "clip_0.npz"))
    for k in KEYS:
        np.testing.assert_array_equal(saved[k], out["tracks"][k])
