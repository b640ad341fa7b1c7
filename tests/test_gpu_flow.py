"""The flow score on the device (``-m gpu``; gfl_flow_pair, gflow_amd/flow.py): known answers, parity of the maps against
the float64 restatement on the oracle (tests/flow_ref.py), the 18 sums against the kernel's own maps, repeatability and
the argument contract, and clip fits with ``flow`` against the restatement run on the inputs they recorded."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import flow_ref as R
from tests.score_fit import FIT, H, T, W, clip

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.5


def run_pair(case, gt_flow=None, move_mask=None, min_weight=0.5, pair=0, n_pairs=1, sums=None, maps=True, ws_bytes=None,
             **override):
    """gfl_flow_pair on the numpy inputs of ``case`` (tests/flow_ref.py's dicts): (rc, sums (n_pairs, 3, 6), flow, valid)"""
    from gflow_amd import _lib as L
    lib = L.load()
    Wc, Hc = case["W"], case["H"]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)
    rec = up(case["rec_a"], np.float32).reshape(-1, 12)
    ids, tr = up(case["ids"], np.int32), up(case["tile_range"], np.int32)
    uv_b, depth_b = up(case["uv_b"], np.float32).reshape(-1, 2), up(case["depth_b"], np.float32).reshape(-1)
    gt = up(np.zeros((Hc, Wc, 2)) if gt_flow is None else gt_flow, np.float32)
    mm = None if move_mask is None else up(move_mask, np.uint8)
    if sums is None:
        sums = torch.full((n_pairs, 3, 6), SENTINEL, dtype=torch.float64, device=DEV)
    flow = torch.full((Hc, Wc, 2), SENTINEL, dtype=torch.float32, device=DEV) if maps else None
    valid = torch.full((Hc, Wc), 7, dtype=torch.uint8, device=DEV) if maps else None
    ws = L.scratch(max(lib.gfl_flow_workspace_bytes(Wc, Hc), 64), DEV)
    a = dict(n_a=rec.shape[0], n_b=uv_b.shape[0], uv_b_stride=2, depth_b_stride=1, W=Wc, H=Hc, min_weight=min_weight,
             pair=pair, n_pairs=n_pairs, ws_bytes=ws.numel() if ws_bytes is None else ws_bytes)
    a.update(override)
    rc = lib.gfl_flow_pair(L.ptr(rec) if rec.numel() else None, a["n_a"], L.ptr(ids) if ids.numel() else None, L.ptr(tr),
                           L.ptr(uv_b) if uv_b.numel() else None, a["uv_b_stride"], L.ptr(depth_b) if depth_b.numel() else None,
                           a["depth_b_stride"], a["n_b"], L.ptr(gt), L.ptr(mm), a["W"], a["H"], a["min_weight"], a["pair"],
                           a["n_pairs"], L.ptr(sums), L.ptr(flow), L.ptr(valid), L.ptr(ws), a["ws_bytes"], L.stream())
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy(), None if flow is None else flow.cpu().numpy(), None if valid is None else valid.cpu().numpy()


def _refs(case, gt_flow=None, move_mask=None, min_weight=0.5):
    gt = np.zeros((case["H"], case["W"], 2), np.float32) if gt_flow is None else gt_flow
    args = (case["rec_a"], case["ids"], case["tile_range"], case["uv_b"], case["depth_b"], gt, move_mask, case["W"], case["H"])
    return R.flow_pair(*args, min_weight=min_weight), R.flow_pair(*args, min_weight=min_weight, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(case, float64 reference, float32 reference) of a parity scene: computed once, shared, never written to"""
    if name == "r600":
        case = R.random_pair(600, 70, 45, seed=3)
    elif name == "r1500":
        case = R.random_pair(1500, 70, 45, seed=4, sigma_px=3.0)
    elif name == "pile":
        case = R.pile_pair()
    elif name == "shuffled":
        case = dict(scene("r600")[0])
        case["ids"], case["tile_range"] = R.shuffled_lists(case["ids"], case["tile_range"], seed=1)
    elif name == "9x5":
        case = R.random_pair(60, 9, 5, seed=2)
    elif name == "empty":
        case = dict(scene("r600")[0])
        case["rec_a"] = np.zeros((0, 12), np.float32)
    else:
        raise ValueError(name)
    return (case,) + _refs(case)


# ---------------------------------------------------------------------------------------------------- known answers
def test_one_splat():
    c = R.known_case("one")
    rc, sums, flow, valid = run_pair(c)
    assert rc == 0
    ys, xs = np.nonzero(valid)
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(7, 8), (8, 7), (8, 8), (8, 9), (9, 8)]
    assert set(np.unique(valid)) == {0, 1}
    np.testing.assert_array_equal(flow[valid != 0], np.tile(np.float32(c["d"][0]), (5, 1)))      # (w d) / w is exact for d = 2, -1
    assert (flow[valid == 0] == 0).all()
    assert sums[0, 0, 0] == 18 * 18 and sums[0, 0, 1] == 5
    assert sums[0, 0, 2] == pytest.approx(5 * np.sqrt(5.0), rel=1e-14)
    assert list(sums[0, 0, 3:]) == [0, 5, 5] and (sums[0, 1:] == 0).all()


def test_two_splats_and_a_culled_one():
    c = R.known_case("two")
    o = float(np.float32(0.8))
    rc, _, flow, valid = run_pair(c)
    assert rc == 0 and valid[8, 8] == 1
    want = (o * c["d"][0] + o * (1 - o) * c["d"][1]) / (o + o * (1 - o))
    np.testing.assert_allclose(flow[8, 8], want, rtol=4 * 2.0 ** -24)            # (two products, a sum, a division)
    c = R.known_case("two_culled")
    rc, _, flow, valid = run_pair(c, min_weight=float(np.float32(0.8)))          # den = 0.8 exactly: still valid at 0.8
    assert rc == 0 and valid[8, 8] == 1
    np.testing.assert_array_equal(flow[8, 8], np.float32(c["d"][0]))
    rc, _, flow, valid = run_pair(c, min_weight=float(np.nextafter(np.float32(0.8), np.float32(1))))
    assert rc == 0 and valid[8, 8] == 0 and (flow[8, 8] == 0).all()


def test_uniform_shift_gives_the_shift_where_the_blend_covers():
    """uv_b = uv_a + (dx, dy) for every row.  A row's d is fl(fl(u + dx) - u), a few ulps of u off dx (computed here the
    same way); a pixel's F is a weighted mean of its contributors' d, so it lies between their extremes up to the
    rounding of the two sums and the division, (2 n + 1) 2^-24 |d| for n contributors (n <= the deepest list position
    any pixel reached).  valid is den >= min_weight, and den = sum of alpha T = 1 - final_T as real numbers; in float32 the
    two differ by up to (n + 1) 2^-24 each, so pixels with |1 - final_T - min_weight| below (n + 1) 2^-23 are left out (at
    most 1 % of the image)."""
    from gflow_amd import _lib as L
    lib = L.load()
    case = dict(scene("r600")[0])
    dx, dy = np.float32(1.75), np.float32(-0.625)
    uv_a = case["rec_a"][:, 0:2]
    case["uv_b"] = (uv_a + np.array([dx, dy], np.float32)).astype(np.float32)
    case["depth_b"] = np.ones(uv_a.shape[0], np.float32)
    Wc, Hc = case["W"], case["H"]
    rec = torch.from_numpy(case["rec_a"]).to(DEV)
    uv, conic, op = rec[:, 0:2].contiguous(), rec[:, 2:5].contiguous(), rec[:, 5:6].contiguous()
    ids, tr = torch.from_numpy(case["ids"]).to(DEV), torch.from_numpy(case["tile_range"]).to(DEV)
    out = torch.zeros(1, Hc, Wc, device=DEV)
    final_T = torch.zeros(Hc, Wc, device=DEV)
    n_contrib = torch.zeros(Hc, Wc, dtype=torch.int32, device=DEV)
    L.check(lib.gfl_blend_fwd(L.ptr(uv), L.ptr(conic), L.ptr(op), L.ptr(op), 1, 0, 1, L.ptr(ids), L.ptr(tr), 0.0, Wc, Hc,
                              L.ptr(out), L.ptr(final_T), L.ptr(n_contrib), L.stream()), "blend")
    cover = 1.0 - final_T.cpu().numpy().astype(np.float64)
    n_max = int(n_contrib.max())
    seen = np.unique(case["ids"])
    d = case["uv_b"][seen] - uv_a[seen]                                          # float32, as the kernel subtracts
    tol = (2 * n_max + 1) * 2.0 ** -24 * float(np.abs(d).max())
    # (this scene is covered above 0.5 everywhere with every row kept; at 0.99 about half of it is)
    for mw, lo, hi in ((0.5, 0.9, 1.0), (float(np.float32(0.99)), 0.2, 0.8)):
        rc, _, flow, valid = run_pair(case, min_weight=mw)
        assert rc == 0
        sure = np.abs(cover - mw) >= (n_max + 1) * 2.0 ** -23
        assert (~sure).mean() <= 0.01
        np.testing.assert_array_equal((valid != 0)[sure], (cover >= mw)[sure])
        F = flow[valid != 0].astype(np.float64)
        print(f"uniform shift, min_weight {mw:.2f}: |F - d| max {np.abs(F - [dx, dy]).max():.3g}, rows' d within "
              f"{np.abs(d - [dx, dy]).max():.3g}, tol {tol:.3g}, valid {float((valid != 0).mean()):.3f}")
        assert lo <= (valid != 0).mean() <= hi
        assert (F >= d.min(axis=0) - tol).all() and (F <= d.max(axis=0) + tol).all()


# ---------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", ["r600", "r1500", "pile", "shuffled", "9x5", "empty"])
def test_maps_match_the_float64_restatement(name):
    case, ref64, ref32 = scene(name)
    rc, sums, flow, valid = run_pair(case)
    assert rc == 0
    assert set(np.unique(valid)) <= {0, 1} and (flow[valid == 0] == 0).all()
    R.compare(flow, valid != 0, ref64, ref32, what=name)
    assert sums[0, 0, 0] == case["W"] * case["H"] and sums[0, 0, 1] == (valid != 0).sum()
    if name == "empty":
        assert not valid.any() and (sums.reshape(-1)[1:] == 0).all()
    elif name == "pile":
        tr = case["tile_range"]
        assert (tr[:, 1] - tr[:, 0]).max() >= 700                                # several LDS batches
    elif name == "shuffled":
        _, _, flow0, valid0 = run_pair(scene("r600")[0])
        np.testing.assert_array_equal(flow, flow0)                               # where the lists lie changes nothing
        np.testing.assert_array_equal(valid, valid0)
    else:
        tr = case["tile_range"]
        assert 0.3 < ref64["valid"].mean() < 1.0
        assert case["W"] % 16 and case["H"] % 16                                 # partial edge tiles
        if name != "9x5":                                                        # (empty tiles: the known-answer cases)
            has = np.zeros(case["rec_a"].shape[0], bool)
            has[:len(case["depth_b"])] = case["depth_b"] != 0
            seen = np.unique(case["ids"])
            assert (~has[seen]).any() and has[seen].any()                        # rows without a future are in the lists


# ------------------------------------------------------------------------------------- the sums, from the kernel's maps
@pytest.mark.parametrize("masked", [True, False])
def test_sums_equal_the_host_sums_of_the_returned_maps(masked):
    case, ref64, _ = scene("r600")
    gt, mask = R.test_targets(ref64["flow"], case["W"], case["H"])
    rc, sums, flow, valid = run_pair(case, gt_flow=gt, move_mask=mask if masked else None)
    assert rc == 0
    assert not (valid != 0)[~np.isfinite(gt).all(-1)].any() and (~np.isfinite(gt)).any()
    want = R.sums_from_maps(flow, valid != 0, gt, mask if masked else None)
    ex = flow.astype(np.float64) - gt.astype(np.float64)
    epe = np.sqrt(ex[..., 0] ** 2 + ex[..., 1] ** 2)[valid != 0]
    assert min(np.abs(epe - t).min() for t in (1.0, 3.0, 5.0)) > 1e-9          # no error sits on a threshold
    share = [float((epe < t).mean()) for t in (1.0, 3.0, 5.0)]
    print("sums test: share of errors below 1 / 3 / 5 px", share)
    assert 0 < share[0] < share[1] < share[2] <= 1.0
    got = sums[0]
    np.testing.assert_array_equal(got[:, [0, 1, 3, 4, 5]], want[:, [0, 1, 3, 4, 5]])
    np.testing.assert_allclose(got[:, 2], want[:, 2], rtol=1e-12, atol=0)
    if masked:
        assert got[1, 1] > 0 and got[2, 1] > 0 and got[1, 0] + got[2, 0] == got[0, 0]
    else:
        assert (got[1:] == 0).all()


# --------------------------------------------------------------------------------------- repeatability and contract
def test_two_calls_give_the_same_bits_and_leave_other_rows_alone():
    case, ref64, _ = scene("r1500")
    gt, mask = R.test_targets(ref64["flow"], case["W"], case["H"])
    sums = torch.full((4, 3, 6), SENTINEL, dtype=torch.float64, device=DEV)
    rc, s1, f1, v1 = run_pair(case, gt_flow=gt, move_mask=mask, pair=2, n_pairs=4, sums=sums)
    assert rc == 0
    assert (s1[[0, 1, 3]] == SENTINEL).all() and (s1[2] != SENTINEL).all()
    rc, s2, f2, v2 = run_pair(case, gt_flow=gt, move_mask=mask, pair=2, n_pairs=4)
    assert rc == 0
    np.testing.assert_array_equal(s1[2].view(np.int64), s2[2].view(np.int64))
    np.testing.assert_array_equal(f1.view(np.int32), f2.view(np.int32))
    np.testing.assert_array_equal(v1, v2)
    rc, s3, f3, v3 = run_pair(case, gt_flow=gt, move_mask=mask, maps=False)     # the maps are optional outputs
    assert rc == 0 and f3 is None
    np.testing.assert_array_equal(s3[0].view(np.int64), s1[2].view(np.int64))


@pytest.mark.parametrize("bad", [dict(pair=-1), dict(pair=1), dict(pair=3, n_pairs=3), dict(min_weight=0.0),
                                 dict(min_weight=-0.5), dict(min_weight=1.0001), dict(min_weight=float("nan")),
                                 dict(W=0), dict(H=0), dict(W=-3), dict(W=16 * 16385, H=16), dict(W=16 * 129, H=16 * 128),
                                 dict(uv_b_stride=1), dict(depth_b_stride=0), dict(ws_bytes=5 * 3 * 18 * 8 - 1),
                                 dict(ws_bytes=0)])
def test_invalid_arguments_are_refused(bad):
    case = scene("r600")[0]
    kw = dict(bad)
    n_pairs = kw.pop("n_pairs", 1)
    rc, sums, flow, valid = run_pair(case, n_pairs=n_pairs, **kw)
    assert rc == -1                                                              # GFL_ERR_INVALID
    assert (sums == SENTINEL).all() and (flow == SENTINEL).all() and (valid == 7).all()      # nothing was launched


def test_the_extremes_of_the_valid_ranges_are_accepted():
    case = scene("9x5")[0]
    rc, sums, _, valid = run_pair(case, min_weight=1.0)
    assert rc == 0 and sums[0, 0, 0] == 45
    rc, sums, _, _ = run_pair(case, pair=2, n_pairs=3)
    assert rc == 0 and (sums[2] != SENTINEL).all() and (sums[:2] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------- through the fit
def _fit(frames, fused=True, cfg=FIT, seed=0, flow="maps", record=True):
    from gflow_amd.fit_video import fit_clip
    keep = {"record_flow_inputs": True} if record else {}
    out = fit_clip(frames, DEV, cfg, seed=seed, fused=fused, deterministic=True if fused else None, flow=flow, keep=keep)
    return out, keep


@pytest.fixture(scope="module")
def det_fit():
    frames = clip(load_gt_pose=True)
    out, keep = _fit(frames)
    return frames, out, keep


def _check_fit_against_restatement(frames, out, keep, n_frames):
    fl = out["flow"]
    inputs = keep["flow_inputs"]
    assert len(inputs) == n_frames - 1 and fl["maps"].shape == (n_frames - 1, H, W, 2) and fl["valid"].dtype == bool
    assert fl["sums"].shape == (n_frames - 1, 3, 6) and fl["EPE"].shape == (n_frames - 1, 3)
    for p, x in enumerate(inputs):
        h = {k: (None if v is None else v.cpu().numpy()) for k, v in x.items()}
        np.testing.assert_array_equal(h["gt_flow"], frames[p]["flow"].cpu().numpy().astype(np.float32))
        np.testing.assert_array_equal(h["move_mask"] != 0, frames[p]["move_mask"].cpu().numpy() != 0)
        args = (h["rec_a"], h["ids"], h["tile_range"], h["uv_b"], h["depth_b"], h["gt_flow"], h["move_mask"], W, H)
        ref64, ref32 = R.flow_pair(*args), R.flow_pair(*args, dtype=torch.float32)
        R.compare(fl["maps"][p], fl["valid"][p], ref64, ref32, what=f"fit pair {p}")
        want = R.sums_from_maps(fl["maps"][p], fl["valid"][p], h["gt_flow"], h["move_mask"])
        np.testing.assert_array_equal(fl["sums"][p][:, [0, 1, 3, 4, 5]], want[:, [0, 1, 3, 4, 5]])
        np.testing.assert_allclose(fl["sums"][p][:, 2], want[:, 2], rtol=1e-12, atol=0)
        assert h["uv_b"].shape[0] >= h["rec_a"].shape[0]                          # rows are only ever appended


def test_fit_flow_equals_the_restatement(det_fit):
    frames, out, keep = det_fit
    _check_fit_against_restatement(frames, out, keep, T)


def test_fit_flow_equals_the_restatement_operator_path():
    frames = clip(n_frames=4, load_gt_pose=True)
    out, keep = _fit(frames, fused=False)
    _check_fit_against_restatement(frames, out, keep, 4)


def test_flow_leaves_the_fit_unchanged():
    from gflow_amd.fit_video import fit_clip
    frames = clip(n_frames=4, load_gt_pose=True)
    cfg = dict(FIT, traj_num=50)
    a = fit_clip(frames, DEV, cfg, seed=0, deterministic=True)
    b = fit_clip(frames, DEV, cfg, seed=0, deterministic=True, flow=True)
    assert a["psnr_sum"] == b["psnr_sum"] and a["splats_final"] == b["splats_final"]
    np.testing.assert_array_equal(a["traj"]["images"], b["traj"]["images"])
    np.testing.assert_array_equal(a["traj"]["uv"], b["traj"]["uv"])
    assert a["rasterisations"] == b["rasterisations"]            # the trajectory recorder's forward is shared
    assert "flow" not in a and "maps" not in b["flow"] and b["flow"]["sums"].shape == (3, 3, 6)
    c = fit_clip(frames, DEV, FIT, seed=0, deterministic=True, flow=True)
    d = fit_clip(frames, DEV, FIT, seed=0, deterministic=True)
    assert c["rasterisations"] == d["rasterisations"] + 4        # one forward of its own per frame when there is none
    assert c["psnr_sum"] == d["psnr_sum"] == a["psnr_sum"]
    np.testing.assert_array_equal(c["flow"]["sums"], b["flow"]["sums"])
    one = fit_clip(frames[:1], DEV, FIT, seed=0, deterministic=True, flow="maps")
    assert one["flow"]["sums"].shape == (0, 3, 6) and one["flow"]["maps"].shape == (0, H, W, 2)
    assert one["flow"]["valid"].shape == (0, H, W) and one["flow"]["EPE"].shape == (0, 3)


def test_concurrent_fits_equal_the_lone_fits():
    from gflow_amd.fit_video import fit_clips_concurrent
    clips = [clip(seed=s, n_frames=4, load_gt_pose=True) for s in (0, 1)]
    lone = [_fit(c, seed=s, record=False)[0] for s, c in enumerate(clips)]
    res = fit_clips_concurrent(clips, DEV, FIT, seeds=[0, 1], deterministic=True, flow="maps")
    for r, want in zip(res, lone):
        assert r["psnr_sum"] == want["psnr_sum"]
        for k in ("sums", "maps", "valid"):
            np.testing.assert_array_equal(r["flow"][k], want["flow"][k])


QUALITY = dict(EPE=0.1887)


def test_flow_quality_on_the_synthetic_clip(det_fit):
    """With every frame's ground-truth camera loaded (deterministic fit: the same numbers on every run of a build).  The
    derived bound: predicting no motion at all costs the mean |gt_flow| over the same valid pixels, and the fitted
    splats must do better than that.  Measured on MI355X: EPE 0.1887 px (still 0.1638, moving 0.4120), acc_1px 0.9936,
    acc_3px 1.0, acc_5px 1.0, coverage 0.9972 over 7 pairs; the zero-flow EPE over the same pixels 2.0111 px.  The second
    bound is the measured EPE plus 20 %, room for a later change to the fit."""
    from gflow_amd import flow as FL
    frames, out, keep = det_fit
    fl = out["flow"]
    m = FL.evaluate(fl)
    zero_sum = n = 0.0
    for p in range(T - 1):
        gt = frames[p]["flow"].cpu().numpy().astype(np.float64)
        v = fl["valid"][p]
        zero_sum += np.sqrt((gt[v] ** 2).sum(-1)).sum()
        n += v.sum()
    assert n == fl["sums"][:, 0, 1].sum()
    zero = zero_sum / n
    print("flow quality", json.dumps(m), "zero-flow EPE", zero)
    assert m["pairs"] == T - 1 and m["coverage"] > 0.5
    assert m["EPE"] < zero
    assert m["EPE"] <= 1.2 * QUALITY["EPE"]
