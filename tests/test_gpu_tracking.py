"""Point tracking on the device (``-m gpu``; gfl_track_anchor / gfl_track_frame, gflow_amd/tracking.py): exact properties
only -- the kernels against np.argmin and the numpy restatement of the reference's frame loop (tests/tracking_ref.py),
fits with queries against the restatement run on the inputs they recorded, deterministic fits against each other --
and bounds on deterministic fits (the same bits on every run of a build)."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import tracking_ref as R
from tests.score_fit import FIT, H, T, W, clip, queries

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _anchor(uv, xy, stride=None):
    """gfl_track_anchor on a float32 uv tensor (rows of ``stride`` floats, (u, v) first) and float64 queries (x, y)"""
    from gflow_amd import _lib as L
    lib = L.load()
    uv = uv.to(DEV).contiguous()
    stride = uv.shape[1] if stride is None else stride
    N = uv.shape[0]
    q = torch.as_tensor(np.asarray(xy, np.float64).reshape(-1, 2)).to(DEV).contiguous()
    n = q.shape[0]
    anchor = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    shift = torch.zeros(n, 2, dtype=torch.float64, device=DEV)
    ws = L.scratch(lib.gfl_track_anchor_workspace_bytes(n, N), DEV)
    L.check(lib.gfl_track_anchor(L.ptr(uv), stride, N, L.ptr(q), n, L.ptr(anchor), L.ptr(shift), L.ptr(ws), ws.numel(),
                                 L.stream()), "track anchor")
    return anchor.long().cpu().numpy(), shift.cpu().numpy()


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _fma_changes_argmin():
    """Rows (a, b), (b, a) around a query on the diagonal: their distances tie when every product and the sum are rounded
    on their own (-> index 0), but fma(dx, dx, dy * dy) and fma(dy, dy, dx * dx) differ -- whichever way a contracted
    distance is formed, one of the two row orders then picks index 1."""
    rng = np.random.default_rng(5)
    for _ in range(100000):
        a, b = (float(np.float32(v)) for v in rng.uniform(0, 100, 2))
        c = float(rng.uniform(0, 100))
        dx, dy = a - c, b - c
        if _fma(dx, dx, dy * dy) != _fma(dy, dy, dx * dx):
            return np.array([[a, b], [b, a]], np.float32), np.array([[c, c]])
    raise AssertionError("no FMA-sensitive tie found")


def test_anchor_matches_argmin_at_size():
    g = torch.Generator(device=DEV).manual_seed(0)
    N, Q = 400000, 4096
    rec = torch.rand(N, 12, device=DEV, generator=g) * torch.tensor([854.0, 480.0] + [1.0] * 10, device=DEV)
    rec[1000:1100, 0:2] = 0                           # culled rows
    xy = (torch.rand(Q, 2, device=DEV, generator=g, dtype=torch.float64) * torch.tensor([854.0, 480.0], device=DEV,
                                                                                          dtype=torch.float64))
    xy[:8] = 0.0                                      # on the culled rows: the lowest of them
    anchor, shift = _anchor(rec, xy.cpu().numpy(), stride=12)
    uv = rec[:, 0:2].double()
    want = []
    for a in range(0, Q, 64):                         # (separate sub / mul / add kernels: nothing can contract)
        d = ((uv[:, None, :] - xy[None, a:a + 64, :]) ** 2).sum(-1)
        want.append(d.argmin(dim=0))
    want = torch.cat(want).cpu().numpy()
    np.testing.assert_array_equal(anchor, want)
    assert (anchor[:8] == 1000).all()
    uvh = rec[:, 0:2].cpu().numpy()
    xyh = xy.cpu().numpy()
    pick = np.arange(0, Q, Q // 64)
    np.testing.assert_array_equal(anchor[pick], R.nearest(uvh, xyh[pick]))
    np.testing.assert_array_equal(shift, xyh - uvh[anchor].astype(np.float64))


def test_anchor_small_cases_match_np_argmin():
    rng = np.random.default_rng(1)
    cases = []
    cases.append((np.array([[3.0, 4.0]], np.float32), np.array([[1.0, 1.0]])))                    # N = 1, Q = 1
    uv = rng.uniform(0, 50, (700, 2)).astype(np.float32)
    uv[[5, 300, 650]] = uv[123]                                                                      # duplicated rows
    uv[400:420] = 0                                                                                  # culled rows
    q = np.concatenate([uv[[123, 410]].astype(np.float64), rng.uniform(-3, 53, (37, 2))])
    cases.append((uv, q))
    uv_nan = uv.copy()
    uv_nan[[333, 600]] = np.nan                                                                      # a NaN row wins
    cases.append((uv_nan, q))
    big = rng.uniform(0, 50, (5000, 2)).astype(np.float32)                                           # ties across slices
    big[4900] = big[7]
    cases.append((big, big[[7, 4900]].astype(np.float64)))
    fu, fq = _fma_changes_argmin()
    cases.append((fu, fq))
    cases.append((fu[::-1].copy(), fq))
    for rows, qs in cases:
        a, s = _anchor(torch.from_numpy(rows), qs)
        want = np.argmin(np.sum((rows[:, None].astype(np.float64) - qs[None]) ** 2, axis=-1), axis=0)
        np.testing.assert_array_equal(a, want)
        np.testing.assert_array_equal(s, qs - rows[a].astype(np.float64))
    a, _ = _anchor(torch.from_numpy(uv), q[:1])
    assert a[0] == 5                                   # (rows 5, 123, 300, 650 are equal: the lowest)
    a, _ = _anchor(torch.from_numpy(uv_nan), q)
    assert (a == 333).all()


def test_frame_kernel_matches_restatement():
    from gflow_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(2)
    h, w, n, q = 16, 24, 64, 40
    uv = rng.uniform(-2, 26, (n, 2)).astype(np.float32)
    uv[:10] = np.array([[0.5, 0.5], [1.5, 2.5], [2.5, 3.5], [-0.5, 4.0], [23.5, 15.5], [24.5, 1.0], [3.0, 15.5],
                        [-1.0, 2.0], [0.0, 0.0], [5.5, -0.5]], np.float32)
    depth = rng.uniform(1, 3, n).astype(np.float32)
    depth[8] = 0.0                                     # culled
    depth[1] = depth[2] = 0.0
    dm = rng.uniform(1, 3, (h, w)).astype(np.float32)
    dm[2, 2] = np.float32(0.05)                        # |dm - d| exactly 0.05f: (1.5, 2.5) rounds to (2, 2)
    dm[4, 2] = np.nextafter(np.float32(0.05), np.float32(1))      # one ulp above: (2.5, 3.5) rounds to (2, 4)
    anchor = np.concatenate([np.arange(10), rng.integers(0, n, q - 10)]).astype(np.int32)
    shift = rng.normal(0, 0.7, (q, 2))
    frames_T, frame, n_anch = 5, 3, 33
    tracks = torch.full((q, frames_T, 2), 9.0, device=DEV)
    occ = torch.full((q, frames_T), 7, dtype=torch.uint8, device=DEV)
    d_uv, d_depth, d_dm = (torch.from_numpy(x).to(DEV) for x in (uv, depth, dm))
    d_anchor, d_shift = torch.from_numpy(anchor).to(DEV), torch.from_numpy(shift).to(DEV)
    L.check(lib.gfl_track_frame(L.ptr(d_uv), 2, L.ptr(d_depth), 1, n, L.ptr(d_dm), w, h, L.ptr(d_anchor), L.ptr(d_shift),
                                n_anch, frame, frames_T, 0.05, L.ptr(tracks), L.ptr(occ), L.stream()), "track frame")
    tr, oc = tracks.cpu().numpy(), occ.cpu().numpy()
    # the restatement, one frame with these anchors
    a = anchor[:n_anch]
    want_t = (uv[a].astype(np.float64) + shift[:n_anch]).astype(np.float32)
    ru, rv = np.round(uv[a, 0]), np.round(uv[a, 1])
    inside = (ru >= 0) & (ru < w) & (rv >= 0) & (rv < h)
    want_o = np.ones(n_anch, bool)
    want_o[inside] = np.abs(dm[rv[inside].astype(int), ru[inside].astype(int)] - depth[a][inside]) > np.float32(0.05)
    np.testing.assert_array_equal(tr[:n_anch, frame], want_t)
    np.testing.assert_array_equal(oc[:n_anch, frame], want_o.astype(np.uint8))
    assert (tr[n_anch:] == 9.0).all() and (oc[n_anch:] == 7).all()            # other queries untouched
    assert (np.delete(tr[:n_anch], frame, axis=1) == 9.0).all()              # other frames untouched
    assert not oc[1, frame] and oc[2, frame]          # exactly 0.05f apart: not occluded (a strict >); one ulp more: occluded
    assert oc[4, frame] and oc[5, frame] and oc[6, frame] and oc[7, frame]     # rint out of the image
    np.testing.assert_array_equal(tr[8, frame], np.float32(shift[8]))          # the culled row at (0, 0)


def _fit(frames, q, fused=True, deterministic=True, cfg=FIT, seed=0):
    from gflow_amd.fit_video import fit_clip
    keep = {"record_track_inputs": True}
    out = fit_clip(frames, DEV, cfg, seed=seed, fused=fused, deterministic=deterministic if fused else None,
                   track_queries=q, keep=keep)
    return out, keep


@pytest.fixture(scope="module")
def det_fit():
    frames = clip()
    g, q = queries(n=96)
    out, keep = _fit(frames, q)
    return frames, g, q, out, keep


def _check_against_restatement(q, out, keep):
    inputs = [(u.cpu().numpy(), d.cpu().numpy(), m.cpu().numpy()) for u, d, m in keep["track_inputs"]]
    assert len(inputs) == T
    ref = R.track_loop(q, inputs)
    got = out["tracks"]
    np.testing.assert_array_equal(got["anchor"], ref["anchor"])
    np.testing.assert_array_equal(got["shift"], ref["shift"])
    np.testing.assert_array_equal(got["tracks"], ref["tracks"])
    np.testing.assert_array_equal(got["occluded"], ref["occluded"])
    t = q[:, 0].astype(int)
    for i in range(len(q)):
        assert (got["tracks"][i, :t[i]] == 0).all() and got["occluded"][i, :t[i]].all()
        for j in range(t[i], T):
            assert got["anchor"][i] < inputs[j][0].shape[0]


def test_fit_tracks_equal_the_restatement(det_fit):
    frames, g, q, out, keep = det_fit
    assert len(np.unique(q[:, 0])) > 1
    _check_against_restatement(q, out, keep)


def test_fit_tracks_equal_the_restatement_operator_path():
    frames = clip()
    g, q = queries(n=96)
    out, keep = _fit(frames, q, fused=False)
    _check_against_restatement(q, out, keep)


def test_deterministic_fits_give_identical_tracks(det_fit):
    from gflow_amd.fit_video import fit_clips_concurrent
    frames, g, q, out, keep = det_fit
    again, _ = _fit(frames, q)
    for k in ("tracks", "occluded", "anchor", "shift"):
        np.testing.assert_array_equal(again["tracks"][k], out["tracks"][k])
    other = clip(seed=1)
    _, q1 = queries(n=96, seed=1)
    lone1, _ = _fit(other, q1, seed=1)
    res = fit_clips_concurrent([frames, other], DEV, FIT, seeds=[0, 1], deterministic=True, track_queries=[q, q1])
    for r, want in zip(res, (out, lone1)):
        for k in ("tracks", "occluded", "anchor", "shift"):
            np.testing.assert_array_equal(r["tracks"][k], want["tracks"][k])


def test_queries_leave_trajectories_unchanged():
    from gflow_amd.fit_video import fit_clip
    frames = clip(n_frames=4)
    _, q = queries(n_frames=4, n=96)
    cfg = dict(FIT, traj_num=50)
    a = fit_clip(frames, DEV, cfg, seed=0, deterministic=True)
    b = fit_clip(frames, DEV, cfg, seed=0, deterministic=True, track_queries=q)
    np.testing.assert_array_equal(a["traj"]["images"], b["traj"]["images"])
    np.testing.assert_array_equal(a["traj"]["uv"], b["traj"]["uv"])
    assert a["rasterisations"] == b["rasterisations"] and "tracks" not in a and "tracks" in b
    with pytest.raises(ValueError):
        fit_clip(frames, DEV, cfg, seed=0, deterministic=True, track_queries=np.array([[4, 1.0, 1.0]]))


def test_tracking_quality_on_the_synthetic_clip(det_fit):
    """Scored against make_clip_tracks (deterministic fit: the same numbers on every run of a build).  Measured on MI355X:
    average_pts_within_thresh 0.6624, occlusion_accuracy 0.7039, average_jaccard 0.4273; the zero-motion baseline
    (prediction = query position, never occluded) 0.1708 and 0.9583.  Bounds: the measured values minus 0.05, and 0.05
    above the baseline's position accuracy (this clip's fit predicts occlusion worse than "never occluded" does)."""
    from gflow_amd import tracking as TK
    frames, g, q, out, keep = det_fit
    pts, occ = g["points"].astype(np.float32), g["occluded"]
    m = TK.evaluate(out["tracks"], pts, occ, H, W, T)
    still = dict(tracks=np.repeat(q[:, None, [2, 1]], T, axis=1).astype(np.float32), occluded=np.zeros((len(q), T), bool))
    m0 = TK.evaluate(still, pts, occ, H, W, T)
    print("tracking quality", json.dumps({k: m[k] for k in ("average_pts_within_thresh", "occlusion_accuracy",
                                                            "average_jaccard")}),
          "zero-motion", json.dumps({k: m0[k] for k in ("average_pts_within_thresh", "occlusion_accuracy")}))
    assert m["average_pts_within_thresh"] >= QUALITY["apts"] - 0.05
    assert m["occlusion_accuracy"] >= QUALITY["oa"] - 0.05
    assert m["average_pts_within_thresh"] >= m0["average_pts_within_thresh"] + 0.05


QUALITY = dict(apts=0.6624, oa=0.7039)


def test_cli_tapvid_block_equals_in_process_evaluate(tmp_path):
    from gflow_amd import io as gio
    from gflow_amd import tracking as TK
    from gflow_amd.fit_video import fit_clip
    n = 5                                              # (the sequence convention fits n - 1 frames)
    frames = clip(n_frames=n)
    seq = gio.write_sequence(frames, str(tmp_path / "clip"))
    g, _ = queries(n_frames=n, n=96)
    pts, occ = g["points"].astype(np.float32), g["occluded"]
    TK.write_tapvid_pickle(os.path.join(seq, "tracking.pkl"), pts, occ)
    args = ["--sequence", seq, "--track", "--deterministic", "--num_points", "1500", "--iterations_first", "60",
            "--iterations_after", "40", "--iterations_camera", "20", "--track-out", str(tmp_path / "out")]
    r = subprocess.run([sys.executable, "-m", "gflow_amd.fit_video", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    disk = gio.load_sequence(seq)
    h, w = disk[0]["image"].shape[:2]
    q = TK.first_visible_queries(pts, occ, h, w)
    keep = q[:, 0] < len(disk)
    cfg = dict(num_points=1500, iterations_first=60, iterations_after=40, iterations_camera=20)
    out = fit_clip(disk, DEV, cfg, seed=0, deterministic=True, track_queries=q[keep])
    m = TK.evaluate(out["tracks"], pts[keep], occ[keep], h, w, len(disk))
    tv = line["tapvid"]
    assert tv["clips"] == 1 and tv["queries_dropped"] == int((~keep).sum())
    for k in ("occlusion_accuracy", "average_jaccard", "average_pts_within_thresh"):
        assert tv[k] == m[k], k
    saved = np.load(os.path.join(tmp_path / "out", "clip_0.npz"))
    np.testing.assert_array_equal(saved["tracks"], out["tracks"]["tracks"])
